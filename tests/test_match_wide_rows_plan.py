"""The host arithmetic of bsg_match_rows_wide_rows (no GPU): tests/wide_rows_check.cpp, built with plain g++ against
bloomsearch_amd/csrc/host/wide_plan.hpp, compared with restatements written here from the call's contract (include/bloomgpu.h): a
pair's tag is a function of (c, R) alone, a header sizes its payload, offsets follow from headers, the stitch of a multi-device call
equals "concatenate the parts' bit rows, then tag", and bsg_match_pair_rows_list's arithmetic expands every tag.  Every restatement
records which of its branches ran and the tests assert that all of them did.

One combination the contract cannot produce is stated instead of tested: LIST + LIST -> DENSE.  Parts are cut at set-relative
multiples of 64 rows, so the parts' tiles add up to the set's (T = T_1 + ... + T_k), a LIST part holds c_i <= 2 T_i - 1 rows, and k
LIST parts hold at most 2 T - k < 2 T together: the stitched pair is a LIST again.  What does reach the DENSE scatter of a LIST part
is LIST + DENSE (and LIST + ALL), and those are covered."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ALL, LIST, DENSE = range(4)
OK, NULL, HEADER = range(3)


def build_driver(exe, flags):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "wide_rows_check.cpp")],
                   check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("wide_rows") / "wide_rows_check", ["-O2"])


class Answers:
    def __init__(self, words):
        self.w, self.at = words, 0

    def take(self, n=None):
        if n is None:
            self.at += 1
            return int(self.w[self.at - 1])
        self.at += n
        return [int(x) for x in self.w[self.at - n: self.at]]

    def done(self):
        return self.at == len(self.w)


def run_driver(exe, tmp_path, cases):
    words = np.concatenate([np.asarray([len(cases)], dtype="<u8")] + [np.asarray(c, dtype="<u8") for c in cases])
    words.tofile(tmp_path / "cases.bin")
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return Answers(np.fromfile(tmp_path / "answers.bin", dtype="<u8"))


def tiles(n):
    return -(-n // 64)


# ---- the contract, restated ----
def want_tag(c, R, took):
    if c == 0:
        took.add("none")
        return NONE
    if c == R:
        took.add("all")
        return ALL
    if c < 2 * tiles(R):
        took.add("list")
        return LIST
    took.add("dense")
    return DENSE


def want_size(hdr, R):
    return {NONE: 0, ALL: 0, LIST: hdr & 0x3FFFFFFF, DENSE: 2 * tiles(R)}[hdr >> 30]


def words32(bits):
    """a bit row as the DENSE payload: 2 u32 per 64 rows, low half first, bits past the last row 0"""
    padded = np.zeros(tiles(len(bits)) * 64, dtype=np.uint8)
    padded[: len(bits)] = bits
    return [int(x) for x in np.packbits(padded, bitorder="little").view("<u4")]


def want_pair(bits, base, took):
    """(header, payload) of the rows `bits` of a set that begin at the set's row `base`: a whole set (base 0) or one device's part"""
    c, R = int(bits.sum()), len(bits)
    tag = want_tag(c, R, took)
    if tag == LIST:
        return LIST << 30 | c, [base + int(i) for i in np.flatnonzero(bits)]
    return tag << 30, words32(bits) if tag == DENSE else []


def test_the_header_states_the_tags_and_the_scan_width(driver, tmp_path):
    ans = run_driver(driver, tmp_path, [[0]])
    assert ans.take(4) == [NONE, ALL, LIST, DENSE]
    width, set_bytes = ans.take(2)
    assert ans.done() and set_bytes == 24
    hdr = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    assert "#define BSG_MATCH_PAIR_SCAN_WIDTH %du" % width in hdr
    for name, v in (("NONE", NONE), ("ALL", ALL), ("LIST", LIST), ("DENSE", DENSE)):
        assert "#define BSG_ROW_%-5s %du" % (name, v) in hdr


def test_tag_size_and_header_are_functions_of_c_and_R(driver, tmp_path):
    took, shapes = set(), []
    for R in (0, 1, 63, 64, 65, 128, 129):
        T = tiles(R)
        for c in sorted({0, 1, 2 * T - 1, 2 * T, R - 1, R}):
            if 0 <= c <= R:
                shapes.append((c, R))
    ans = run_driver(driver, tmp_path, [[1, c, R] for c, R in shapes])
    for c, R in shapes:
        tag = want_tag(c, R, took)
        hdr = tag << 30 | (c if tag == LIST else 0)
        assert ans.take(3) == [tag, hdr, want_size(hdr, R)], (c, R)
        assert want_size(hdr, R) <= 2 * tiles(R)                                       # never longer than the bit row
    assert ans.done() and took == {"none", "all", "list", "dense"}
    # the edges by name: R == 0 is NONE; one row is NONE or ALL; 2T - 1 is the longest LIST, 2T the first DENSE; R - 1 of 64 rows is DENSE
    assert want_tag(0, 0, took) == NONE and want_tag(1, 1, took) == ALL and want_tag(3, 65, took) == LIST and want_tag(4, 65, took) == DENSE
    assert want_tag(1, 64, took) == LIST and want_tag(2, 64, took) == DENSE and want_tag(63, 64, took) == DENSE and want_tag(62, 63, took) == DENSE


def test_offsets_follow_from_headers(driver, tmp_path):
    rng = np.random.default_rng(5)
    sizes = [0, 1, 63, 64, 65, 128, 129, 0]
    first = [0] + [int(x) for x in np.cumsum(sizes)]
    poff = [0, 2, 5, 5, 9, 14, 20, 27, 29]                                             # set 2 has no pair; sets 0 and 7 have pairs and no rows
    took, cases, wants = set(), [], []
    for pair0 in (0, 7):                                                               # the call's table, and a part's (its pairs begin at 7)
        hdr, off, at = [], [], 0
        for s, R in enumerate(sizes):
            for _ in range(poff[s], poff[s + 1]):
                c = int(rng.choice([0, 1, 2 * tiles(R) - 1, 2 * tiles(R), R - 1, R]))
                c = min(max(c, 0), R)
                tag = want_tag(c, R, took)
                hdr.append(tag << 30 | (c if tag == LIST else 0))
                off.append(at)
                at += want_size(hdr[-1], R)
        for want_off in (1, 0):
            cases.append([2, len(sizes)] + first + [p + pair0 for p in poff] + hdr + [want_off])
            wants.append([at] + (off + [at] if want_off else []))
    ans = run_driver(driver, tmp_path, cases)
    for w in wants:
        assert ans.take(len(w)) == w
    assert ans.done() and took == {"none", "all", "list", "dense"}


def stitch_case(sizes, sqo, cuts, rows_of_pair, took, combos):
    """One call cut into parts: the driver's input (what each device hands back, restated from the contract) and the wanted result
    ("concatenate the bit rows, then tag": here the bit rows are whole to begin with and the parts are slices of them)."""
    first = [0] + [int(x) for x in np.cumsum(sizes)]
    n_sets = len(sizes)
    case = [3, n_sets] + first + sqo + [len(cuts)] + cuts
    want_sets = []
    pieces_of = {}
    for r0, r1 in zip(cuts, cuts[1:]):
        with_rows = [s for s in range(n_sets) if max(first[s], r0) < min(first[s + 1], r1)]
        sets = list(range(with_rows[0], with_rows[-1] + 1))
        hdrs, payload, table, word0 = [], [], [], 0
        for s in sets:
            a, b = max(first[s], r0) - first[s], min(first[s + 1], r1) - first[s]      # the part's rows of the set, set-relative
            assert a % 64 == 0
            table.append([word0, sqo[s] - sqo[sets[0]], b - a, a // 64])
            word0 += tiles(b - a) * (sqo[s + 1] - sqo[s])
            for p in range(sqo[s], sqo[s + 1]):
                h, pl = want_pair(rows_of_pair[p][a:b], a, took)
                hdrs.append(h)
                payload += pl
                pieces_of.setdefault(p, []).append(h >> 30)
        table.append([word0, sqo[sets[-1] + 1] - sqo[sets[0]], 0, 0])
        case += hdrs + [len(payload)] + payload
        want_sets.append(table)
    want_hdr, want_payload = [], []
    for s in range(n_sets):
        for p in range(sqo[s], sqo[s + 1]):
            h, pl = want_pair(rows_of_pair[p], 0, took)
            want_hdr.append(h)
            want_payload += pl
            combos.add((tuple(pieces_of.get(p, [])), h >> 30))
    return case, want_sets, want_hdr, want_payload


def bits_of(R, rows):
    b = np.zeros(R, dtype=np.uint8)
    b[list(rows)] = 1
    return b


def test_the_stitch_equals_tagging_the_concatenated_bit_rows(driver, tmp_path):
    rng = np.random.default_rng(11)
    took, combos, cases, wants = set(), set(), [], []
    # call 1: a 400-row set (T = 7) cut at its rows 128 and 256 into three parts (2 + 2 + 3 tiles), between two whole sets, one empty
    sizes, sqo = [10, 400, 0, 70], [0, 2, 12, 13, 15]
    designed = [bits_of(400, [0, 5, 127, 128, 200, 255, 256, 300, 399]),               # LIST + LIST + LIST -> LIST (3 + 3 + 3 < 14)
                bits_of(400, [1, 2, 3, 4, 300]),                                       # DENSE (4 of 128 rows) + NONE + LIST -> LIST
                bits_of(400, list(range(128)) + list(range(256, 400))),                # ALL + NONE + ALL -> DENSE
                bits_of(400, range(400)),                                              # ALL + ALL + ALL -> ALL
                bits_of(400, []),                                                      # NONE everywhere
                bits_of(400, [7] + list(range(130, 250, 3)) + [390]),                  # LIST + DENSE + LIST -> DENSE
                bits_of(400, list(range(128)) + [129]),                                # ALL + LIST + NONE -> DENSE
                bits_of(400, range(0, 400, 2)),                                        # DENSE + DENSE + DENSE -> DENSE
                rng.integers(0, 2, size=400, dtype=np.uint8), bits_of(400, rng.choice(400, size=13, replace=False))]
    rows1 = [bits_of(10, [3]), bits_of(10, range(10))] + designed + [np.zeros(0, dtype=np.uint8)] + [bits_of(70, [69]), bits_of(70, range(0, 70, 9))]
    cases.append((sizes, sqo, [0, 10 + 128, 10 + 256, 480], rows1))
    # call 2: two parts.  A 197-row set (T = 4) cut at its row 192: the last part holds 5 rows; a 200-row set cut at 64
    sizes, sqo = [197, 200], [0, 4, 8]
    rows2 = [bits_of(197, range(192, 197)),                                            # NONE + ALL -> LIST (5 < 8)
             bits_of(197, range(192)),                                                 # ALL + NONE -> DENSE
             bits_of(197, [0, 191, 192]), bits_of(197, range(197))]                    # LIST + LIST -> LIST; ALL + ALL -> ALL
    cases.append((sizes, sqo, [0, 192, 397], rows2 + [bits_of(200, [1]), bits_of(200, range(200)), bits_of(200, [])] + [bits_of(200, [0, 1, 2])]))
    sizes, sqo = [200, 0], [0, 4, 5]                                                   # the set without rows at the end lies in no part
    rows3 = [bits_of(200, range(64)),                                                  # ALL + NONE -> DENSE (64 >= 8)
             bits_of(200, [0, 199]), bits_of(200, [5, 64, 65, 66, 67, 68]),            # LIST + LIST -> LIST, and the most two LIST parts hold
             bits_of(200, range(64, 200)), np.zeros(0, dtype=np.uint8)]                # NONE + ALL -> DENSE
    cases.append((sizes, sqo, [0, 64, 200], rows3))
    cases.append((sizes, sqo, [0, 200], rows3))                                        # one part: the stitch is the identity
    built = [stitch_case(s, o, c, r, took, combos) for s, o, c, r in cases]
    ans = run_driver(driver, tmp_path, [b[0] for b in built])
    for _, want_sets, want_hdr, want_payload in built:
        for table in want_sets:
            assert ans.take() == len(table)
            for entry in table:
                assert ans.take(4) == entry
        assert ans.take(len(want_hdr)) == want_hdr
        assert ans.take() == len(want_payload) and ans.take(len(want_payload)) == want_payload
    assert ans.done() and took == {"none", "all", "list", "dense"}
    for combo in [((LIST, LIST, LIST), LIST), ((LIST, LIST), LIST), ((NONE, ALL), LIST), ((ALL, NONE), DENSE), ((NONE, ALL), DENSE),
                  ((ALL, ALL), ALL), ((ALL, ALL, ALL), ALL), ((ALL, NONE, ALL), DENSE), ((DENSE, NONE, LIST), LIST), ((LIST, DENSE, LIST), DENSE),
                  ((ALL, LIST, NONE), DENSE), ((DENSE, DENSE, DENSE), DENSE), ((), NONE), ((NONE, NONE, NONE), NONE)]:
        assert combo in combos, combo
    # what the module's docstring states: no number of LIST parts makes a DENSE pair
    assert not any(set(parts) == {LIST} and tag == DENSE for parts, tag in combos)
    assert int(rows3[2].sum()) == 2 * tiles(200) - 2                                   # (2 T_1 - 1) + (2 T_2 - 1): the most two LIST parts hold


def test_pair_rows_list_expands_every_tag(driver, tmp_path):
    took = set()
    R = 150                                                                            # T = 3: a LIST holds up to 5 rows
    lst, dns = bits_of(R, [0, 63, 64, 149]), bits_of(R, range(0, 150, 7))
    shapes = []
    for bits in (bits_of(R, []), bits_of(R, range(R)), lst, dns, bits_of(1, [0]), bits_of(64, [0, 63]), bits_of(64, range(1, 64))):
        hdr, payload = want_pair(bits, 0, took)
        rows = [int(i) for i in np.flatnonzero(bits)]
        for cap in sorted({len(bits), len(rows), max(len(rows) - 1, 0), 1, 0}):
            shapes.append(([4, hdr, len(bits), cap, 1, len(payload)] + payload, OK, len(rows), rows[:cap]))
    shapes.append(([4, ALL << 30, R, R, 0, 0], OK, R, list(range(R))))                 # NONE / ALL never read the payload
    shapes.append(([4, NONE << 30, 0, 4, 0, 0], OK, 0, []))                            # a set without rows
    l4 = [0, 63, 64, 149]
    bad = [[4, LIST << 30 | 4, R, R, 0, 0], [4, DENSE << 30, R, R, 0, 0],              # a payload is needed and there is none
           [4, LIST << 30 | 6, R, R, 1, 6, 0, 1, 2, 3, 4, 5],                          # 6 = 2T: no LIST
           [4, LIST << 30, R, R, 1, 0], [4, LIST << 30 | 1, 1, 1, 1, 1, 0],            # c == 0 and c == R are no LIST either
           [4, LIST << 30 | 4, R, R, 1, 4, 0, 64, 63, 149], [4, LIST << 30 | 4, R, R, 1, 4, 0, 63, 63, 149],      # not ascending
           [4, LIST << 30 | 4, R, R, 1, 4] + l4[:3] + [150],                           # an index past the set
           [4, ALL << 30 | 3, R, R, 0, 0], [4, NONE << 30 | 1, R, R, 0, 0], [4, ALL << 30, 0, 4, 0, 0],          # counts where none belong
           [4, DENSE << 30, R, R, 1, 6, 0, 0, 0, 0, 0, 1 << 22]]                       # a bit at row 150 of 150
    want_status = [NULL, NULL] + [HEADER] * (len(bad) - 2)
    ans = run_driver(driver, tmp_path, [s[0] for s in shapes] + bad)
    for case, status, n, rows in shapes:
        assert ans.take(3) == [status, n, 1], case[:4]                                 # the full count, and nothing written past cap
        assert ans.take(len(rows)) == rows
    for case, status in zip(bad, want_status):
        assert ans.take(3)[::2] == [status, 1], case
    assert ans.done() and took == {"none", "all", "list", "dense"}


def test_the_driver_is_clean_under_the_sanitizers(tmp_path):
    """the same driver as a stand-alone program under AddressSanitizer and UBSan, over every kind of case"""
    exe = build_driver(tmp_path / "wide_rows_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    took, combos = set(), set()
    rows = [bits_of(200, range(64)), bits_of(200, [0, 199]), bits_of(200, range(200)), bits_of(200, range(0, 200, 3)), bits_of(200, [])]
    stitch = stitch_case([200, 0], [0, 5, 5], [0, 128, 200], rows, took, combos)[0]
    cases = [[0], [1, 3, 65], [1, 4, 65], [2, 2, 0, 65, 65, 0, 2, 3, LIST << 30 | 3, DENSE << 30, NONE, 1], stitch,
             [4, LIST << 30 | 2, 65, 1, 1, 2, 0, 64], [4, DENSE << 30, 65, 1, 1, 4, 3, 0, 1, 0], [4, ALL << 30, 65, 3, 0, 0],
             [4, DENSE << 30, 65, 0, 1, 4, 3, 0, 1, 0]]
    ans = run_driver(exe, tmp_path, cases)
    assert ans.take(4) == [NONE, ALL, LIST, DENSE]
