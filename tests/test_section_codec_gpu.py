"""k_decode_sections / k_encode_payload / k_crc_sections against the oracle, bit for bit, over the slice counts and header faults of
tests/section_shapes.py: sections of 1 to 32 slices on the default and on widened units, every presence mask, slice boundaries that cut a
word in two, mixed runs, chunked delivery, corruption of single slices, and malformed headers under a correct checksum with
parseFilterSection's exact code.  Expected values come from oracle/oracle.py only.  A wrong decoded word is a false negative of the whole
engine, so words are compared WHOLE (bsg_or_reduce over a one-block arena returns that block's words of a kind), not sampled by probes."""
import numpy as np
import pytest

from bloomsearch_amd import query as Q
from bloomsearch_amd.gpu import Context
from oracle import oracle as O
from tests import helpers as H
from tests import section_shapes as S
from tests.helpers import device_ids

pytestmark = pytest.mark.gpu

CASE_IDS = [c.name for c in S.CASES]


def _assert_words(ctx, aid, filters):
    """The arena of ONE block holds exactly `filters`: every present kind's words, whole.  For a kind with no present filter bsg_or_reduce
    is seen to accept any word count and to return zeros (include/bloomgpu.h does not say); that the kind IS nil is shown by the callers'
    probes, which a nil filter lets pass (fail-open)."""
    for kind, f in enumerate(filters):
        if f is None:
            assert not ctx.or_reduce(aid, kind, 4).any(), kind
            continue
        got = ctx.or_reduce(aid, kind, len(f.words))
        if not np.array_equal(got, f.words):
            bad = np.flatnonzero(got != f.words)
            raise AssertionError("kind %d: %d of %d words differ, first at word %d (got %016x, want %016x)"
                                 % (kind, len(bad), len(f.words), bad[0], int(got[bad[0]]), int(f.words[bad[0]])))


class _Queries:
    """300 random expressions over S.VOCAB and the oracle's verdicts for them over any list of blocks."""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.cb = Q.compile_queries([None] + [H.random_expression(rng, S.VOCAB, None) for _ in range(300)])
        self.ops, self.poff, _ = self.cb.arrays()
        self.terms = H.oracle_terms(self.cb)

    def want(self, blocks):
        """blocks: per block [Filter | None] * 3, or None for a block whose filters are all nil."""
        words, desc = S.arena_of(blocks)
        return O.probe_batch(words, desc, self.terms.view(O.TERM_DTYPE), self.ops, self.poff)

    def got(self, ctx, aid, n_blocks):
        return ctx.probe(aid, n_blocks, self.terms, self.ops, self.poff)


@pytest.fixture(scope="module")
def queries():
    return _Queries(404)


# ---- 1. bit-exact decode, one section per arena ----

@pytest.mark.parametrize("name", CASE_IDS)
def test_decode_is_bit_exact(ctx, queries, name):
    """Words whole; the descriptor's m, k and Barrett constant (its + 1 branch where m is a power of two) and the nil kinds through probes:
    a probe reduces every location by the decoded m with the decoded constant, k times, and a nil kind lets every term pass."""
    case = S.BY_NAME[name]
    filters = S.dense_filters(case)
    sec = O.encode_filter_section(filters)
    assert len(sec) == S.classify(case.mask, case.nws).P + 4
    aid, status = ctx.arena_load_sections([sec])
    try:
        assert status.tolist() == [0]
        _assert_words(ctx, aid, filters)
        assert np.array_equal(queries.got(ctx, aid, 1), queries.want([filters]))
    finally:
        ctx.arena_free(aid)


# ---- 2. mixed runs ----

_MIXED = ["five_slices", "tail_only_1w", "last_default_unit", None, "flags_byte_slice", "first_widened_unit", "flags_only", "largest_single",
          "one_mib", "three_slices_m3", None, "last_default_unit", "four_slices_m7", "first_widened_unit", "one_granule_5w", "thirty_slices_m6",
          "one_mib", "last_word0_only", "flags_only", "last_default_unit", "five_slices", "first_widened_unit", "mask7_three_slices", "one_mib",
          "two_slices_m5", "thirty_slices_m6", "one_mib", "tail_only_4w"]


class _Mixed:
    """One file of 28 blocks built from entries (the oracle's build; caller-chosen m so the sizes hit the classes), its queries and the
    oracle's verdicts.  Computed once, shared, never modified."""

    def __init__(self):
        self.specs = [S.BY_NAME[n] if n else None for n in _MIXED]
        self.n_blocks = len(self.specs)
        self.blob, self.off, self.fstart, self.desc, self.n_words, self.strings = S.entry_plan(self.specs, seed=2024)
        self.words = O.build_many(self.blob, self.off, self.fstart, self.desc, self.n_words)
        self.sections = S.sections_from_words(self.specs, self.words, self.desc)
        assert [len(s) for s in self.sections] == [0 if c is None else S.classify(c.mask, c.nws).P + 4 for c in self.specs]
        rng = np.random.default_rng(77)
        self.cb = Q.compile_queries([None] + [H.random_expression(rng, S.VOCAB, None) for _ in range(300)])
        self.ops, self.poff, _ = self.cb.arrays()
        self.terms = H.oracle_terms(self.cb)
        # every inserted entry as its own query, remembered with the block it must survive on
        own, self.own_block = [], []
        for b, (fields, toks, pairs) in enumerate(self.strings):
            for e in [Q.Field(f) for f in fields] + [Q.Token(t) for t in toks] + [Q.FieldToken(f, t) for f, t in pairs]:
                own.append(e)
                self.own_block.append(b)
        self.own_block = np.asarray(self.own_block)
        self.own_cb = Q.compile_queries(own)
        self.own_ops, self.own_poff, _ = self.own_cb.arrays()
        self.own_terms = H.oracle_terms(self.own_cb)

    def want(self, blocks=None, nil=()):
        """The oracle's survivors over the blocks listed (all by default), those in `nil` with their filters taken away."""
        blocks = list(range(self.n_blocks)) if blocks is None else list(blocks)
        desc = np.concatenate([self.desc[b * 3: b * 3 + 3] for b in blocks])
        for i in nil:
            desc["m"][i * 3: i * 3 + 3] = 0
        return O.probe_batch(self.words, desc, self.terms.view(O.TERM_DTYPE), self.ops, self.poff)


@pytest.fixture(scope="module")
def mixed():
    return _Mixed()


def _check_mixed(c, mx):
    aid, status = c.arena_load_sections(mx.sections)
    try:
        assert not status.any(), status.tolist()
        assert np.array_equal(c.probe(aid, mx.n_blocks, mx.terms, mx.ops, mx.poff), mx.want())
        # no false negative, stated directly: an entry survives its own query on its own block
        got = c.probe(aid, mx.n_blocks, mx.own_terms, mx.own_ops, mx.own_poff)
        q = np.arange(len(mx.own_block))
        alive = (got[q, mx.own_block >> 6] >> (mx.own_block & 63).astype(np.uint64)) & np.uint64(1)
        assert alive.all(), [(int(mx.own_block[i]), int(i)) for i in np.flatnonzero(alive == 0)[:10]]
        assert np.array_equal(got, O.probe_batch(mx.words, mx.desc, mx.own_terms.view(O.TERM_DTYPE), mx.own_ops, mx.own_poff))
    finally:
        c.arena_free(aid)


def test_mixed_run_build_matches_oracle(ctx, mixed):
    """The words the sections are made of are the oracle's; the library's own build of the same entries gives the same."""
    assert np.array_equal(ctx.build(mixed.blob, mixed.off, mixed.fstart, mixed.desc, mixed.n_words), mixed.words)


def test_mixed_run(ctx, mixed):
    """Grid x = the run's largest split count with most workgroups returning early; slots indexed first + blockIdx.y."""
    _check_mixed(ctx, mixed)


@pytest.mark.parametrize("pieces", [1, 64])
def test_mixed_run_in_pieces(ctx, mixed, pieces):
    """The region decoded behind one copy, and in as many pieces as its size allows (sections straddle the pieces)."""
    ctx.set_lab(4, pieces)
    try:
        _check_mixed(ctx, mixed)
    finally:
        ctx.set_lab(4, 4)


def test_mixed_run_two_devices(mixed):
    with Context(device_ids(2)) as c2:
        _check_mixed(c2, mixed)


# ---- 3. stream delivery of multi-slice sections ----

_STREAM_A = [0, 1, 2, 3, 4, 5, 6, 9, 15]          # 5 slices, 1, 32 default, none, 2, 32 widened, all-nil, 3, 30
_STREAM_B = [7, 8, 10, 12, 13, 14, 17, 18, 20]    # another region of the same section count


def _file_of(mx, blocks):
    base = 1000
    begin, end, data = [], [], bytearray(np.random.default_rng(5).integers(0, 256, size=base, dtype=np.uint8).tobytes())
    for b in blocks:
        begin.append(len(data))
        data += mx.sections[b]
        end.append(len(data))
    return bytes(data), begin, end


def _stream(ctx, data, begin, end, deliveries):
    sid = ctx.arena_stream_begin(begin, end)
    try:
        for lo, hi in deliveries:
            ctx.arena_stream_append(sid, lo, data[lo:hi])
    except BaseException:
        ctx.arena_stream_abort(sid)
        raise
    return ctx.arena_stream_finish(sid, len(begin))


def _chunks(lo, hi, step):
    return [(o, min(o + step, hi)) for o in range(lo, hi, step)]


@pytest.mark.parametrize("how", ["small_chunks", "boundary_in_32_slices", "tail_before_head"])
def test_stream_delivery(ctx, mixed, how):
    data, begin, end = _file_of(mixed, _STREAM_A)
    n = len(data)
    if how == "small_chunks":                      # chunks smaller than a slice
        deliveries = _chunks(0, n, 5000)
    elif how == "boundary_in_32_slices":           # block 2 of the file (32 slices) is cut in two by a chunk boundary, block 5 likewise
        cut = begin[2] + 200_001
        assert begin[2] < cut < end[2]
        deliveries = [(0, cut)] + _chunks(cut, n, 300_000)
        assert any(begin[5] < lo < end[5] for lo, _ in deliveries)
    else:                                          # the tail half of the widened 32-slice section, and all behind it, before its head
        mid = (begin[5] + end[5]) // 2 + 3
        deliveries = [(mid, n), (0, mid)]
    aid, status = _stream(ctx, data, begin, end, deliveries)
    try:
        assert not status.any(), status.tolist()
        assert np.array_equal(ctx.probe(aid, len(begin), mixed.terms, mixed.ops, mixed.poff), mixed.want(_STREAM_A))
    finally:
        ctx.arena_free(aid)


def test_second_load_starts_from_clean_accumulators(ctx, mixed):
    """The same region twice, then another of the same section count: a slot's checksum accumulator and arrival flags start from zero."""
    for blocks in (_STREAM_A, _STREAM_A, _STREAM_B, _STREAM_A):
        aid, status = ctx.arena_load_sections([mixed.sections[b] for b in blocks])
        try:
            assert not status.any(), (blocks, status.tolist())
            assert np.array_equal(ctx.probe(aid, len(blocks), mixed.terms, mixed.ops, mixed.poff), mixed.want(blocks))
        finally:
            ctx.arena_free(aid)


# ---- 4. corruption of sliced sections ----

class _Dense:
    """Dense sections between two clean multi-slice neighbours."""

    def __init__(self):
        self.left = S.dense_filters(S.BY_NAME["three_slices_m3"], salt=1)
        self.right = S.dense_filters(S.BY_NAME["mask7_three_slices"], salt=1)
        self.left_sec, self.right_sec = O.encode_filter_section(self.left), O.encode_filter_section(self.right)
        self.mid = {}

    def middle(self, name):
        if name not in self.mid:
            fl = S.dense_filters(S.BY_NAME[name], salt=1)
            self.mid[name] = (fl, O.encode_filter_section(fl))
        return self.mid[name]


@pytest.fixture(scope="module")
def dense():
    return _Dense()


def _corruptions():
    out = []
    for name in ("five_slices", "last_default_unit", "first_widened_unit", "one_mib"):
        sh = S.classify(S.BY_NAME[name].mask, S.BY_NAME[name].nws)
        mid = sh.slices[sh.n_split // 2]
        out += [(name, "slice0_near_end", sh.P - 3), (name, "middle_slice", (mid[0] + mid[1]) // 2), (name, "last_slice", sh.last_slice // 2),
                (name, "last_slice_first_byte", 0), (name, "crc_trailer", sh.P + 1)]
    sh = S.classify(S.BY_NAME["flags_byte_slice"].mask, S.BY_NAME["flags_byte_slice"].nws)
    assert sh.last_slice == 1
    out += [("flags_byte_slice", "flags_byte", 0), ("flags_byte_slice", "first_byte_of_slice0", 1), ("flags_byte_slice", "crc_trailer", sh.P)]
    return out


@pytest.mark.parametrize("name,where,offset", _corruptions(), ids=["%s-%s" % (n, w) for n, w, _ in _corruptions()])
def test_corrupt_slice_is_isolated(ctx, dense, queries, name, where, offset):
    fl, sec = dense.middle(name)
    bad = bytearray(sec)
    bad[offset] ^= 0x04                     # (in the flags byte: still a known flag bit, so only the checksum can tell)
    aid, status = ctx.arena_load_sections([dense.left_sec, bytes(bad), dense.right_sec])
    try:
        assert status.tolist() == [0, -2, 0]
        # the corrupted block's three filters are nil (fail-open); the neighbours answer as the oracle does over their own words
        assert np.array_equal(queries.got(ctx, aid, 3), queries.want([dense.left, None, dense.right]))
    finally:
        ctx.arena_free(aid)
    # and the same section, clean, between the same neighbours
    aid, status = ctx.arena_load_sections([dense.left_sec, sec, dense.right_sec])
    try:
        assert status.tolist() == [0, 0, 0]
        assert np.array_equal(queries.got(ctx, aid, 3), queries.want([dense.left, fl, dense.right]))
    finally:
        ctx.arena_free(aid)


# ---- 5. header faults with exact codes ----

_FAULTS = S.header_faults()


@pytest.mark.parametrize("name,sec,deviation", _FAULTS, ids=[n for n, _, _ in _FAULTS])
def test_header_fault_reports_the_oracles_code(ctx, dense, queries, name, sec, deviation):
    """One malformed payload under a correct checksum between two clean neighbours.  Every one was parsed by the oracle on the CPU first
    (tests/test_section_shapes.py does the same without a GPU); parse_section_header reads the flags byte, 4 bytes of a length where 4 are
    left and 28 where 28 are left, all below the payload's end, so no case reads outside its section."""
    if deviation:
        # bloom/v3 ReadFrom (the oracle) takes m, k and the bitset length as they come and accepts the section; the decoder calls a bitset
        # shorter than m, k > 1 024, an m whose word count wraps (include/bloomgpu.h, deviations) and also m = 0 and k = 0 a bad filter
        assert S.oracle_code(sec) == 0
        code = -5
    else:
        code = S.oracle_code(sec)
        assert code != 0
    aid, status = ctx.arena_load_sections([dense.left_sec, sec, dense.right_sec])
    try:
        assert status.tolist() == [0, code, 0]
        assert np.array_equal(queries.got(ctx, aid, 3), queries.want([dense.left, None, dense.right]))
    finally:
        ctx.arena_free(aid)


# ---- 6. encoder over the same sizes ----

@pytest.mark.parametrize("name", [c.name for c in S.CASES if c.mask])
def test_encode_is_byte_exact_and_decodes_back(ctx, name):
    case = S.BY_NAME[name]
    blob, off, fstart, desc, n_words, _ = S.entry_plan([case], seed=len(name) * 131 + case.mask, n_tokens=2500)
    words = O.build_many(blob, off, fstart, desc, n_words)
    filters = O.block_filters(words, desc, 0)
    want = O.encode_filter_section(filters)
    got = ctx.build_sections(blob, off, fstart, desc.view(H.DESC_DTYPE), n_words)
    assert len(got) == 1 and len(got[0]) == len(want)
    if got[0] != want:
        a, b = np.frombuffer(got[0], dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        bad = np.flatnonzero(a != b)
        raise AssertionError("%d of %d bytes differ, first at %d" % (len(bad), len(want), bad[0]))
    if O.hw_crc32c_fn() is not None:      # the checksum once more, by the CPU's own crc32 instruction
        assert int.from_bytes(got[0][-4:], "little") == O.hw_crc32c(got[0][:-4])
    # device-encoded, device-decoded, equal to the oracle's words
    aid, status = ctx.arena_load_sections(got)
    try:
        assert status.tolist() == [0]
        _assert_words(ctx, aid, filters)
    finally:
        ctx.arena_free(aid)
