"""The case list of the section-codec GPU tests (tests/section_shapes.py) covers every slicing class it was written for, and the plain
Python restatement of decode_unit / decode_splits agrees with bloomsearch_amd/csrc/crc_slices.h (through tests/crc_slices_check.cpp, the
program tests/test_crc_slices.py builds).  No GPU."""
import os
import subprocess

import pytest

from oracle import oracle as O
from tests import section_shapes as S
from tests.test_crc_slices import ROOT, SIZES

# (mask, words per filter) -> (P, U, n_split, bytes of the last slice): one row per slicing class the case list has to reach
TABLE = [
    (0, (0, 0, 0), (1, 16384, 1, 1)),
    (2, (0, 1, 0), (37, 16384, 1, 37)),
    (2, (0, 4, 0), (61, 16384, 1, 61)),
    (2, (0, 5, 0), (69, 16384, 1, 69)),
    (2, (0, 2044, 0), (16381, 16384, 1, 16381)),
    (3, None, (16385, 16384, 2, 1)),                    # any nw0 + nw1 = 2041
    (2, (0, 2045, 0), (16389, 16384, 2, 5)),
    (2, (0, 2048, 0), (16413, 16384, 2, 29)),
    (2, (0, 2049, 0), (16421, 16384, 2, 37)),
    (5, (1, 0, 2046), (16433, 16384, 2, 49)),
    (3, (2100, 2100, 0), (33657, 16384, 3, 889)),
    (7, (3, 4000, 2500), (52109, 16384, 4, 2957)),
    (2, (0, 10000, 0), (80029, 16384, 5, 14493)),
    (6, (0, 30000, 30001), (480065, 16384, 30, 4929)),
    (2, (0, 65532, 0), (524285, 16384, 32, 16381)),
    (2, (0, 65533, 0), (524293, 16448, 32, 14405)),
    (2, (0, 131072, 0), (1048605, 32832, 32, 30813)),
]


@pytest.mark.parametrize("mask,nws,want", TABLE)
def test_every_row_of_the_table_is_a_case(mask, nws, want):
    hits = [c for c in S.CASES if c.mask == mask and (c.nws == nws if nws is not None else sum(c.nws) == 2041)]
    assert hits, (mask, nws)
    sh = S.classify(hits[0].mask, hits[0].nws)
    assert (sh.P, sh.U, sh.n_split, sh.last_slice) == want
    assert sh.last_slice == sh.P - (sh.n_split - 1) * sh.U
    assert sum(hi - lo for lo, hi in sh.slices) == sh.P


def test_case_list_reaches_every_class():
    shapes = {c.name: S.classify(c.mask, c.nws) for c in S.CASES}
    one = [sh for sh in shapes.values() if sh.n_split == 1]
    # single slice: no granule at all, exactly one, the most a slice of the default unit holds beside a tail, and fewer than 29 bytes
    assert any(sh.G[0] == 0 and sh.tail[0] for sh in one) and any(sh.G[0] == 1 for sh in one)
    assert any(sh.G[0] == 255 and sh.tail[0] == 61 for sh in one)
    assert any(sh.P < 29 for sh in one) and any(sh.P >= 29 and sh.G[0] == 0 for sh in one)
    # every slice count of the default unit's small end, many slices, and all 32 arrival flags on both kinds of unit
    counts = {sh.n_split for sh in shapes.values()}
    assert {1, 2, 3, 4, 5, 30, 32} <= counts
    assert any(sh.n_split == 32 and sh.U == S.DEFAULT_UNIT for sh in shapes.values())
    # full middle slices of the default unit: one granule for each of the 256 threads, no tail
    assert any(sh.n_split >= 3 and sh.U == S.DEFAULT_UNIT and sh.G[1] == 256 and sh.tail[1] == 0 for sh in shapes.values())
    # widened units: 257 granules (thread 0 takes two), 513 (three trips for some threads)
    assert any(sh.U > S.DEFAULT_UNIT and sh.G[0] == 257 for sh in shapes.values())
    assert any(sh.U > S.DEFAULT_UNIT and sh.G[0] == 513 for sh in shapes.values())
    # the last slice: the flags byte alone; ends inside the first length field; ends exactly at word 0; holds word 0 and nothing more
    lasts = {(sh.last_slice, min(sh.w0.values())) for sh in shapes.values() if sh.n_split == 2}
    assert (1, 29) in lasts and (5, 29) in lasts and (29, 29) in lasts and (37, 29) in lasts
    # slice boundaries relative to a filter's words: only residues 0 and 4 exist, by presence count; both must be cut INSIDE a filter
    for sh in shapes.values():
        assert set(sh.cls.values()) <= {0, 4}
        assert all(sh.straddles[c] == (sh.cls[c] == 4) for c in sh.cls if sh.n_split > 1 and _cut_inside(sh, c))
    for kind in range(3):
        # (the last present filter ends at P, so it is always in class 0: the field-token filter never straddles)
        assert kind == 2 or any(sh.cls.get(kind) == 4 and sh.straddles[kind] for sh in shapes.values()), kind
        assert any(sh.cls.get(kind) == 0 and sh.n_split > 1 and _cut_inside(sh, kind) for sh in shapes.values()), kind
    # two filters of different class in one section, each cut; three present with the middle one in class 4
    assert any(sorted(sh.cls.values()) == [0, 4] and all(_cut_inside(sh, c) for c in sh.cls) for sh in shapes.values())
    assert any(len(sh.cls) == 3 and sh.cls[1] == 4 and sh.straddles[1] for sh in shapes.values())
    # all seven presence masks at one three-slice size
    for mask in range(1, 8):
        assert any(c.mask == mask and shapes[c.name].n_split == 3 for c in S.CASES), mask
    assert any(c.mask == 0 for c in S.CASES)


def _cut_inside(sh, c):
    """A slice boundary falls strictly inside filter c's words."""
    nxt = min([w for w in sh.w0.values() if w > sh.w0[c]] + [sh.P + 28]) - 28
    return any(sh.w0[c] < lo < nxt for lo, _ in sh.slices[:-1])


def test_case_list_filter_sizes():
    present = [(c, k) for c in S.CASES for k in range(3) if (c.mask >> k) & 1]
    for c, k in present:
        assert c.nws[k] == (c.ms[k] + 63) // 64 and 1 <= c.ks[k] <= 1024
    for c in S.CASES:
        assert all(c.ms[k] == 0 and c.nws[k] == 0 for k in range(3) if not (c.mask >> k) & 1)
    ragged = [c for c in S.CASES if c.mask and any(c.ms[k] % 64 for k in range(3) if (c.mask >> k) & 1)]
    assert 2 * len(ragged) >= len(S.CASES)
    assert sum(1 for c, k in present if c.ms[k] == 64 * c.nws[k]) >= 2
    assert any(c.ms[k] & (c.ms[k] - 1) == 0 for c, k in present)      # a power of two: the descriptor's magic takes its + 1 branch
    assert len({(c.mask, c.nws) for c in S.CASES}) == len(S.CASES)


def test_restatement_agrees_with_the_header(tmp_path):
    exe = tmp_path / "crc_slices_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "crc_slices_check.cpp")], check=True, timeout=120)
    sizes = sorted(set(SIZES) | {S.classify(c.mask, c.nws).P for c in S.CASES})
    r = subprocess.run([str(exe)] + [str(s) for s in sizes], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert [int(f[0]) for f in lines] == sizes
    for f in lines:
        P = int(f[0])
        assert (int(f[1]), int(f[2])) == (S.decode_unit(P), S.decode_splits(P + 4)), P
    assert [S.decode_splits(n) for n in range(6)] == [1, 1, 1, 1, 1, 1]


def test_header_faults_on_the_oracle():
    """Every malformed section of the GPU header-fault test goes through parseFilterSection's restatement here first: the oracle rejects
    each with the code its construction aims at (the GPU test takes the code from the oracle, not from this table), and ACCEPTS the five
    deviations, m = 0 and k = 0 among them, which the decoder calls a bad filter."""
    faults = S.header_faults()
    assert len({name for name, _, _ in faults}) == len(faults)
    aim = {"first_header": -4, "second_header": -4, "third_header": -4, "flen_one": -4, "flen_2": -5, "bitset_one": -5, "trailing": -6,
           "flag_0x": -3, "len_": -1, "truncated": -4}
    for name, sec, deviation in faults:
        if deviation:
            assert S.oracle_code(sec) == 0, name          # the oracle ACCEPTS these; the decoder's -5 is pinned by the GPU test
            continue
        want = [code for prefix, code in aim.items() if name.startswith(prefix)]
        assert len(want) == 1, name
        if name == "second_header_28_left_flen_24":
            want = [-5]                                   # the length fits exactly; the bitset does not
        assert S.oracle_code(sec) == want[0], name
        if len(sec) >= 5:
            assert O.crc32c(sec[:-4]) == int.from_bytes(sec[-4:], "little"), name
    assert {name for name, _, deviation in faults if deviation} == {"bitset_shorter_than_m", "k_1025", "m_wraps", "m_0_no_words", "k_0"}
    assert len(dict((n, s) for n, s, _ in faults)["m_0_no_words"]) == 29 + 4      # flags + a 28-byte header, no word
    # the speculative first batch is skipped below 29 payload bytes; later headers are read alone with 4 .. 27 bytes left
    assert any(5 <= len(sec) < 33 for _, sec, _ in faults)
    assert sum(1 for name, sec, _ in faults if S.decode_splits(len(sec)) == 3) >= 2
