"""bsg_or_reduce, bsg_or_reduce_dev and bsg_or_words_dev (k_or_reduce_blocks, k_or_words: the merge path) at the shapes where they
branch, word for word.  Arenas are loaded with bsg_arena_load from words this file writes itself — no build is involved — and the
reference is numpy's OR over the first ceil(m / 64) words of each present filter of the kind.

What a block's filter holds: a witness bit no other block sets ((b * step) % m with step coprime to m) and a second one near the end
(m - 2 - b), both distinct per block wherever m >= n_blocks + 2; bit 0, bit m - 1, and both sides of the 128-bit boundaries nearest to
either end (127 | 128 and the last multiple of 128 below m).  Where m < n_blocks + 2 (the one- and two-word geometries with hundreds of
blocks) the witnesses rotate and several blocks share one: a lost block is then not distinguishable from its partners, only a lost or
invented bit is.  The caller's words behind every filter are all-ones padding: a 16-byte load that reads past an odd last word and is
not masked by `two` would carry them into the result (bsg_arena_load re-lays every filter on a 128-byte boundary with zero padding, so
this guards the library's layout as a whole, not the kernel's mask alone).  Every kind of an arena has a geometry of its own.

The kernel's paths: gridDim.y == 1 stores plainly, more groups merge with atomicOr into a zeroed output; a group is read 16 loads at a
time, so group sizes and block counts that are no multiple of 16 leave a partly filled last trip; BSG_LAB_OR_GROUP (read per call) sets
the group size.  k_or_words walks a grid-stride loop whose second trip needs more than 4 096 x 256 words."""
import ctypes as C
import math

import numpy as np
import pytest

from bloomsearch_amd._lib import BSG_E_INVALID, DESC_DTYPE, BloomGpuError
from bloomsearch_amd.gpu import Context
from tests import helpers as H
from tests.test_configs_gpu import HipMem

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SENTINEL = np.uint64(0x5EA15EA15EA15EA1)
PAD_WORDS = 3
BIG_WORDS = 4096 * 256 + 3                     # one more trip of k_or_words' grid-stride loop, and an odd count
OTHER_GEOMETRIES = ((5 * 64 - 1, 3), (9 * 64 - 30, 5))


def words_of(m):
    return (m + 63) // 64


def bits_of_block(b, m):
    step = next(s for s in (97, 61, 1) if math.gcd(s, m) == 1)
    last128 = (m - 1) // 128 * 128
    bits = {(b * step) % m, (m - 2 - b) % m, 0, m - 1}
    bits |= {p for p in (127, 128, last128 - 1, last128) if 0 <= p < m}
    return sorted(bits)


def filter_words(b, m):
    w = np.zeros(words_of(m), dtype=np.uint64)
    for p in bits_of_block(b, m):
        w[p >> 6] |= np.uint64(1 << (p & 63))
    return w


def make_arena(n_blocks, geometry, nil=frozenset()):
    """geometry: (m, k) per kind; nil: {(block, kind)}.  -> (words, desc): the caller's layout, every filter followed by PAD_WORDS all-ones
    words."""
    desc = np.zeros(n_blocks * 3, dtype=DESC_DTYPE)
    chunks, at = [], 0
    for b in range(n_blocks):
        for kind, (m, k) in enumerate(geometry):
            if (b, kind) in nil:
                continue                                   # m = 0: a nil filter
            w = filter_words(b, m)
            desc[b * 3 + kind] = (at, m, k, 0)
            chunks += [w, np.full(PAD_WORDS, ONES, dtype=np.uint64)]
            at += len(w) + PAD_WORDS
    words = np.concatenate(chunks) if chunks else np.zeros(1, dtype=np.uint64)
    return words, desc


def reference(words, desc, kind, n_words):
    out = np.zeros(n_words, dtype=np.uint64)
    for b in range(len(desc) // 3):
        d = desc[b * 3 + kind]
        if d["m"]:
            assert words_of(int(d["m"])) == n_words
            out |= words[int(d["word_off"]): int(d["word_off"]) + n_words]
    return out


def geometry_for(kind, n_words):
    """the asked kind gets n_words words with a partial last one; the other two kinds the OTHER_GEOMETRIES"""
    g = list(OTHER_GEOMETRIES)
    g.insert(kind, (n_words * 64 - 17, 7))
    return g


def nil_set(spec, n_blocks, kind, group):
    if spec == "first":
        return {(0, kind)}
    if spec == "last":
        return {(n_blocks - 1, kind)}
    if spec == "group":
        return {(b, kind) for b in range(group, 2 * group)}
    if spec == "all":
        return {(b, kind) for b in range(n_blocks)}
    assert spec is None
    return set()


# (n_blocks, n_words, kind, group (None: BSG_LAB_OR_GROUP unset), nil filters)
OR_TABLE = [
    (1, 1, 0, None, None), (2, 2, 1, None, None), (15, 3, 2, None, None), (16, 127, 0, None, None), (17, 128, 1, None, None),
    (33, 129, 2, None, None), (255, 257, 0, None, None), (256, 3, 1, None, None), (257, 2, 2, None, None), (513, 1, 0, None, None),
    (33, 16385, 1, None, None), (2, 16385, 2, 1, None),
    (1, 3, 0, 1, None), (2, 3, 1, 1, None), (17, 2, 2, 1, None), (1, 2, 0, 1, None),
    (16, 3, 1, 16, None), (17, 3, 2, 16, None), (15, 128, 0, 16, None), (33, 128, 1, 16, None),
    (17, 129, 2, 17, None), (33, 127, 0, 17, None), (255, 2, 1, 17, None),
    (256, 257, 2, 256, None), (257, 257, 0, 256, None), (513, 128, 1, 256, None), (255, 1, 2, 256, None),
    (33, 3, 1, 16, "first"), (33, 3, 1, 16, "last"), (33, 129, 0, 16, "group"), (17, 2, 2, 16, "all"), (5, 3, 1, None, "all"),
]


def test_table_reaches_both_store_paths_for_odd_and_even_word_counts():
    with_group = [(nb, nw, g) for nb, nw, _, g, nil in OR_TABLE if g is not None]
    for odd in (0, 1):
        assert any(-(-nb // g) == 1 and nw % 2 == odd for nb, nw, g in with_group), odd        # gridDim.y == 1: plain stores
        assert any(-(-nb // g) > 1 and nw % 2 == odd for nb, nw, g in with_group), odd         # atomicOr into the zeroed output
    assert {c[2] for c in OR_TABLE} == {0, 1, 2} and {c[3] for c in OR_TABLE} == {None, 1, 16, 17, 256}
    assert {c[0] for c in OR_TABLE} >= {1, 2, 15, 16, 17, 33, 255, 256, 257, 513} and {c[1] for c in OR_TABLE} == {1, 2, 3, 127, 128, 129, 257, 16385}
    assert {c[4] for c in OR_TABLE} == {None, "first", "last", "group", "all"} and 28 <= len(OR_TABLE) <= 36
    assert any(nb % g and g % 16 for nb, _, g in with_group)                                  # a last trip of fewer than 16 loads


def set_group(monkeypatch, group):
    if group is None:
        monkeypatch.delenv("BSG_LAB_OR_GROUP", raising=False)
    else:
        monkeypatch.setenv("BSG_LAB_OR_GROUP", str(group))


def device_words(values):
    """memory of device 0 (the session context's) holding `values` (u64).  The current device is set first: freeing an arena of a context
    of several devices leaves the thread on whichever device was visited last."""
    values = np.ascontiguousarray(values, dtype=np.uint64)
    assert C.CDLL("libamdhip64.so").hipSetDevice(0) == 0
    mem = HipMem(values.nbytes)
    assert mem.hip.hipMemcpy(mem.ptr, C.c_void_p(values.ctypes.data), C.c_size_t(values.nbytes), 1) == 0       # hipMemcpyHostToDevice
    return mem


@pytest.mark.parametrize("n_blocks,n_words,kind,group,nil", OR_TABLE, ids=lambda v: "-" if v is None else str(v))
def test_or_reduce_equals_numpy(ctx, monkeypatch, n_blocks, n_words, kind, group, nil):
    geometry = geometry_for(kind, n_words)
    words, desc = make_arena(n_blocks, geometry, nil_set(nil, n_blocks, kind, group))
    want = reference(words, desc, kind, n_words)
    assert want.any() == (nil != "all")
    set_group(monkeypatch, group)
    aid = ctx.arena_load(words, desc)
    try:
        got = ctx.or_reduce(aid, kind, n_words)
        assert np.array_equal(got, want), "words %s differ" % np.flatnonzero(got != want)[:8].tolist()
        for other in range(3):                              # the other kinds of the same arena, each with its own geometry
            if other != kind:
                nw = words_of(geometry[other][0])
                assert np.array_equal(ctx.or_reduce(aid, other, nw), reference(words, desc, other, nw)), other
    finally:
        ctx.arena_free(aid)


@pytest.mark.parametrize("n_blocks,n_words,group", [(16, 129, 16), (33, 129, 16), (17, 3, 256), (17, 3, 1), (5, 16385, None)])
def test_or_reduce_dev_writes_n_words_and_nothing_behind(ctx, monkeypatch, n_blocks, n_words, group):
    """an odd n_words on the gridDim.y == 1 path and on the atomic path: the word behind the last one belongs to somebody else"""
    kind, guard = 1, 5
    words, desc = make_arena(n_blocks, geometry_for(kind, n_words))
    want = reference(words, desc, kind, n_words)
    set_group(monkeypatch, group)
    aid = ctx.arena_load(words, desc)
    mem = device_words(np.full(n_words + guard, SENTINEL, dtype=np.uint64))
    try:
        ctx.or_reduce_dev(aid, kind, mem.ptr.value, n_words)
        got = mem.read()
        assert np.array_equal(got[:n_words], want)
        assert np.array_equal(got[:n_words], ctx.or_reduce(aid, kind, n_words))
        assert (got[n_words:] == SENTINEL).all(), got[n_words:]
    finally:
        mem.free()
        ctx.arena_free(aid)


def test_mixed_geometry_and_wrong_length_are_refused(ctx):
    """BSG_E_INVALID on the host, before any launch"""
    for name, second in (("m", (3 * 64 - 17 + 64, 7)), ("k", (3 * 64 - 17, 8))):
        words, desc = make_arena(4, geometry_for(1, 3))
        desc[2 * 3 + 1]["m"], desc[2 * 3 + 1]["k"] = second
        if name == "m":                                     # a longer filter: give it room behind the arena
            desc[2 * 3 + 1]["word_off"] = len(words)
            words = np.concatenate([words, np.zeros(8, dtype=np.uint64)])
        aid = ctx.arena_load(words, desc)
        try:
            with pytest.raises(BloomGpuError) as err:
                ctx.or_reduce(aid, 1, 3)
            assert err.value.code == BSG_E_INVALID, name
            assert np.array_equal(ctx.or_reduce(aid, 0, words_of(OTHER_GEOMETRIES[0][0])), reference(words, desc, 0, words_of(OTHER_GEOMETRIES[0][0])))
        finally:
            ctx.arena_free(aid)
    words, desc = make_arena(4, geometry_for(1, 3))
    aid = ctx.arena_load(words, desc)
    try:
        for n_words in (2, 4):
            with pytest.raises(BloomGpuError) as err:
                ctx.or_reduce(aid, 1, n_words)
            assert err.value.code == BSG_E_INVALID, n_words
    finally:
        ctx.arena_free(aid)


# ---- contexts of several entries ----

@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(n):
        if n not in made:
            made[n] = Context(H.device_ids(n))
        return made[n]
    yield get
    for c in made.values():
        c.close()


def shard_cases():
    out = [(n, nb, None) for n in (2, 3, 8) for nb in sorted({1, n - 1, n, 2 * n + 1})]
    return out + [(2, 5, "odd-blocks-nil"), (3, 7, "first-shard-nil")]


@pytest.mark.parametrize("n,n_blocks,nil", shard_cases(), ids=lambda v: "-" if v is None else str(v))
def test_or_reduce_over_shards(contexts, monkeypatch, n, n_blocks, nil):
    """block b lies on entry b % n: fewer blocks than entries leave shards without blocks; a shard whose filters of the kind are all nil
    stands beside one that has real ones"""
    kind, n_words = 1, 129
    nil_blocks = {"odd-blocks-nil": {b for b in range(n_blocks) if b % n == 1}, "first-shard-nil": {b for b in range(n_blocks) if b % n == 0}, None: set()}[nil]
    words, desc = make_arena(n_blocks, geometry_for(kind, n_words), {(b, kind) for b in nil_blocks})
    want = reference(words, desc, kind, n_words)
    assert want.any()
    set_group(monkeypatch, None)
    mctx = contexts(n)
    aid = mctx.arena_load(words, desc)
    try:
        got = mctx.or_reduce(aid, kind, n_words)
        assert np.array_equal(got, want), "words %s differ" % np.flatnonzero(got != want)[:8].tolist()
    finally:
        mctx.arena_free(aid)


def test_or_reduce_over_two_shards_takes_k_or_words_second_trip(contexts, monkeypatch):
    """four blocks of 4 096 x 256 + 3 words (32 MiB in all) on two entries: the partials are folded by k_or_words, whose grid of 4 096 x 256
    threads covers the last three words — bit m - 1, the last 128-bit boundary, the tail witnesses — on its second trip only"""
    kind, n_blocks = 1, 4
    m = BIG_WORDS * 64 - 17
    desc = np.zeros(n_blocks * 3, dtype=DESC_DTYPE)
    rng = np.random.default_rng(11)
    words = rng.integers(0, 1 << 63, size=n_blocks * (BIG_WORDS + PAD_WORDS), dtype=np.uint64)
    words &= rng.integers(0, 1 << 63, size=len(words), dtype=np.uint64)
    for b in range(n_blocks):
        at = b * (BIG_WORDS + PAD_WORDS)
        desc[b * 3 + kind] = (at, m, 10, 0)
        words[at + BIG_WORDS - 1] &= np.uint64((1 << (m % 64)) - 1)
        for p in bits_of_block(b, m):
            words[at + (p >> 6)] |= np.uint64(1 << (p & 63))
        words[at + BIG_WORDS: at + BIG_WORDS + PAD_WORDS] = ONES
    want = reference(words, desc, kind, BIG_WORDS)
    assert all(int(want[-1]) >> ((m - 2 - b) & 63) & 1 for b in range(n_blocks))
    set_group(monkeypatch, None)
    mctx = contexts(2)
    aid = mctx.arena_load(words, desc)
    try:
        got = mctx.or_reduce(aid, kind, BIG_WORDS)
        assert np.array_equal(got, want), "words %s differ" % np.flatnonzero(got != want)[:8].tolist()
    finally:
        mctx.arena_free(aid)


# ---- bsg_or_words_dev ----

@pytest.mark.parametrize("n_src", [0, 1, 3])
@pytest.mark.parametrize("n_words", [1, 255, 256, 257, BIG_WORDS])
def test_or_words_dev_accumulates_into_dst(ctx, n_words, n_src):
    rng = np.random.default_rng(n_words * 7 + n_src)
    guard = 4

    def sparse(n):
        return rng.integers(0, 1 << 63, size=n, dtype=np.uint64) & rng.integers(0, 1 << 63, size=n, dtype=np.uint64) & rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    dst = sparse(n_words)
    dst[0] |= np.uint64(1 << 63)
    src = sparse(max(n_src, 1) * n_words)
    want = dst.copy()
    for s in range(n_src):
        want |= src[s * n_words: (s + 1) * n_words]
    d_dst = device_words(np.concatenate([dst, np.full(guard, SENTINEL, dtype=np.uint64)]))
    d_src = device_words(src)
    try:
        ctx.or_words_dev(d_dst.ptr.value, d_src.ptr.value, n_words, n_src)
        got = d_dst.read()
        assert np.array_equal(got[:n_words], want), "words %s differ" % np.flatnonzero(got[:n_words] != want)[:8].tolist()
        assert (got[n_words:] == SENTINEL).all()
        assert np.array_equal(d_src.read()[: len(src)], src)
        assert n_src == 0 or not np.array_equal(want, dst)                    # the sources really add bits
    finally:
        d_dst.free()
        d_src.free()
