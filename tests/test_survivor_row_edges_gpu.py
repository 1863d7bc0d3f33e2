"""k_survivor_rows / k_survivor_rows_packed and DeviceRun::rows_out against the output contract of include/bloomgpu.h, exactly: every row
width the staging tile takes (G = 1 .. 16) and the path without it (G >= 17), both sides of every tag edge, query counts around the
256-query run, calls of more than 64 arenas, and a context of three devices.  The arenas are crafted (tests/survivor_row_shapes.py): the
survivors of every query are known by design and confirmed by the oracle, so every header, every payload byte and every byte the call
must NOT write is pinned by S.check_call; gpu.rows_to_dense, bsg_survivor_rows_list(_packed) and bsg_survivor_row_list then read the same
buffers and must agree with the oracle too."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q
from bloomsearch_amd.gpu import BloomGpuError, Context, packed_headers, rows_to_dense, survivor_row_list
from oracle import oracle as O
from tests import helpers as H
from tests import survivor_row_shapes as S
from tests.helpers import device_ids

pytestmark = pytest.mark.gpu

POISON = 0xA5
TAIL = 64                      # words / headers behind what bsg_survivor_rows_size reports: they must come back untouched
PACKED = _lib.PROBE_ROWS_PACKED

_built = {}                    # block count -> (words, desc, bool [N_BASE][B]: the oracle's survivors of the base queries)


def built(c, B):
    if B not in _built:
        p = S.plan(B)
        words = c.build(p.blob, p.off, p.fstart, p.desc, p.n_words)
        want = S.bits_to_matrix(O.survivors_tree(words, p.desc.view(O.DESC_DTYPE), S.BASE_EXPRS), B)
        assert np.array_equal(want, S.design_matrix(B)), B          # (tests/test_survivor_row_shapes.py shows the same on the oracle's own words)
        _built[B] = (words, p.desc, want)
    return _built[B]


class Call:
    """The arenas loaded, the batch created and both page-locked buffers sized by bsg_survivor_rows_size + TAIL; run() poisons them, makes
    ONE bsg_probe_many_rows call and checks everything it left."""

    def __init__(self, c, nbs, NQ, nd=1):
        self.c, self.nbs, self.NQ, self.nd = c, list(nbs), NQ, nd
        self.aids = [c.arena_load(*built(c, B)[:2]) for B in self.nbs]
        idx = S.stretch(NQ)
        self.want = [built(c, B)[2][idx] for B in self.nbs]
        cb = Q.compile_queries(S.exprs_for(NQ))
        ops, poff, _ = cb.arrays()
        self.bid = c.batch_create(H.gpu_terms(c, cb), ops, poff)
        self.rw, self.hw = c.survivor_rows_size(self.aids, self.bid)
        self.rows = c.pinned_array((self.rw + TAIL) * 8).view(np.uint64)
        self.hdr = c.pinned_array((self.hw + TAIL) * 4).view(np.uint32)

    def poison(self):
        self.rows.view(np.uint8)[:] = POISON
        self.hdr.view(np.uint8)[:] = POISON

    def untouched(self):
        return bool((self.rows.view(np.uint8) == POISON).all() and (self.hdr.view(np.uint8) == POISON).all())

    def run(self, flags):
        c, packed = self.c, bool(flags & PACKED)
        self.poison()
        c.probe_many_rows(self.aids, self.bid, self.rows, self.hdr, flags)
        if flags & _lib.PROBE_ASYNC:
            c.sync()
        S.check_call(self.rows, self.hdr, POISON, self.nbs, self.NQ, self.want, packed, self.nd, self.rw, self.hw)
        self.readers(packed)

    def readers(self, packed):
        c, NQ = self.c, self.NQ
        qs = sorted({q for q in (0, 1, 254, 255, 256, 257, NQ - 1) if q < NQ})
        for j, B in enumerate(self.nbs):
            for q in qs:
                got = c.survivor_rows_list(self.aids, self.bid, self.rows, self.hdr, j, q, B, packed=packed)
                assert np.array_equal(got, np.flatnonzero(self.want[j][q])), (j, B, q, packed)
        for u in S.Layout(self.nbs, NQ, self.nd).units:      # the shard-local readers: device d holds the blocks d, d + nd, ...
            want = self.want[u.i][:, u.d:: self.nd]
            h = packed_headers(self.hdr, u.hdr_at // NQ, NQ) if packed else self.hdr[u.hdr_at: u.hdr_at + NQ]
            r = self.rows[u.row_off: u.row_off + NQ * u.G].reshape(NQ, u.G)
            assert np.array_equal(S.bits_to_matrix(rows_to_dense(h, r, u.nl, packed=packed), u.nl), want), (u, packed)
            if not packed:
                for q in qs:
                    assert np.array_equal(survivor_row_list(int(h[q]), r[q], u.nl), np.flatnonzero(want[q])), (u, q)

    def close(self):
        c = self.c
        c.pinned_free(self.rows.view(np.uint8))
        c.pinned_free(self.hdr.view(np.uint8))
        c.batch_free(self.bid)
        for a in self.aids:
            c.arena_free(a)


def one_call(c, nbs, NQ, flags, nd=1):
    call = Call(c, nbs, NQ, nd)
    try:
        call.run(flags)
    finally:
        call.close()


@pytest.mark.parametrize("flags", [0, PACKED, PACKED | _lib.PROBE_ASYNC], ids=["dense", "packed", "packed-async"])
def test_every_staged_width_in_one_call(ctx, flags):
    """G = 1 .. 16 at 64 (G - 1) + 1, 64 G - 1 and 64 G blocks: the tile's stride G | 1, the 256 / G and 256 % G stepping, the full tile at
    G = 16, the last valid bit of a ragged last word, and a second run of ONE query behind a full one."""
    one_call(ctx, S.WIDTH_BS, S.WIDTH_NQ, flags)


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("NQ", S.QEDGE_NQS)
def test_query_counts_around_the_256_query_run(ctx, NQ, packed):
    one_call(ctx, S.QEDGE_BS, NQ, PACKED if packed else 0)


def test_rows_of_more_than_16_words_take_the_path_without_the_tile(ctx):
    one_call(ctx, S.UNSTAGED_BS, S.UNSTAGED_NQ, 0)


def test_packed_rows_of_more_than_16_words_are_refused_and_nothing_is_written(ctx):
    """BSG_E_UNSUPPORTED before anything is launched: both buffers keep the poison, the part of the 64-block arena the packed form could
    have taken included; and the packed reader gives the same answer for the same arenas."""
    call = Call(ctx, list(S.UNSTAGED_BS) + [64], S.UNSTAGED_NQ)
    try:
        call.poison()
        with pytest.raises(BloomGpuError) as ei:
            ctx.probe_many_rows(call.aids, call.bid, call.rows, call.hdr, PACKED)
        assert ei.value.code == _lib.BSG_E_UNSUPPORTED
        ctx.sync()
        assert call.untouched()
        with pytest.raises(BloomGpuError) as ei:
            ctx.survivor_rows_list(call.aids, call.bid, call.rows, call.hdr, 0, 0, S.UNSTAGED_BS[0], packed=True)
        assert ei.value.code == _lib.BSG_E_UNSUPPORTED
        call.run(0)                                          # the dense layout takes the same call
    finally:
        call.close()


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("n_arenas", S.RUN_ARENAS)
def test_arena_runs_of_the_rows_launch(ctx, n_arenas, packed):
    """rows_out launches in runs of 64 arenas: 63 and 64 arenas take one launch, 65 two, 129 three (i0 = 0, 64, 128)."""
    ctx.set_probe_group(0)
    one_call(ctx, S.run_blocks(n_arenas), S.RUN_NQ, PACKED if packed else 0)


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_129_arenas_in_groups_of_three(ctx, packed):
    """43 dispatches: every group's destination table is indexed through the group's own arena numbers."""
    ctx.set_probe_group(3)
    try:
        one_call(ctx, S.run_blocks(129), S.RUN_NQ, PACKED if packed else 0)
    finally:
        ctx.set_probe_group(0)


def test_three_devices_at_the_packed_limit():
    """3 x 1 024 and 3 x 961 blocks on a context of three devices: every shard at (or at an odd count below) the packed form's limit, each
    written into its device's slice, merged by bsg_survivor_rows_list_packed into global block order.  One block more puts 1 025 on
    device 0: refused for the packed form with nothing written, taken by the dense layout."""
    with Context(device_ids(S.SHARD_ND)) as m:
        call = Call(m, S.SHARD_BS, S.SHARD_NQ, S.SHARD_ND)
        try:
            call.run(PACKED)
            call.run(0)
        finally:
            call.close()
        call = Call(m, list(S.SHARD_BS) + [S.SHARD_REFUSED_B], S.SHARD_NQ, S.SHARD_ND)
        try:
            call.poison()
            with pytest.raises(BloomGpuError) as ei:
                m.probe_many_rows(call.aids, call.bid, call.rows, call.hdr, PACKED)
            assert ei.value.code == _lib.BSG_E_UNSUPPORTED
            m.sync()
            assert call.untouched()
            call.run(0)
        finally:
            call.close()
