"""Thin numpy-facing wrapper over the C-ABI (include/bloomgpu.h).

Test / bench glue only: every method is one call into libbloomgpu.so; no
arithmetic of the hot path is done in Python.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import DESC_DTYPE, TERM_DTYPE, BloomGpuError, IngestStats, Timing
from .tokenizer import c_spec


def pack_entries(entries):
    """list[bytes|str] -> (u8 blob, u32 offsets[n+1]) in the layout bsg_hash_entries / bsg_build take."""
    entries = [e.encode() if isinstance(e, str) else bytes(e) for e in entries]
    off = np.zeros(len(entries) + 1, dtype=np.uint32)
    if entries:
        off[1:] = np.cumsum([len(e) for e in entries], dtype=np.uint64).astype(np.uint32)
    blob = np.frombuffer(b"".join(entries), dtype=np.uint8).copy() if entries else np.zeros(0, dtype=np.uint8)
    return blob, off


def survivor_list(row: np.ndarray, n_blocks: int) -> np.ndarray:
    """bsg_survivor_list: the surviving block indices of one query's survivor row, ascending (host arithmetic)."""
    L = _lib.load()
    row = np.ascontiguousarray(row, dtype=np.uint64)
    n = C.c_uint32()
    out = np.zeros(max(n_blocks, 1), dtype=np.uint32)
    rc = L.bsg_survivor_list(_lib._ptr(row), n_blocks, _lib._ptr(out), len(out), C.byref(n))
    if rc:
        raise BloomGpuError(rc, L.bsg_last_error(None).decode())
    return out[: n.value].copy()


def survivor_row_list(hdr: int, row: np.ndarray, n_blocks: int) -> np.ndarray:
    """bsg_survivor_row_list: the surviving block indices of one row of bsg_probe_many_rows, whatever its tag."""
    L = _lib.load()
    row = np.ascontiguousarray(row, dtype=np.uint64)
    n = C.c_uint32()
    out = np.zeros(max(n_blocks, 1), dtype=np.uint32)
    rc = L.bsg_survivor_row_list(int(hdr), _lib._ptr(row), n_blocks, _lib._ptr(out), len(out), C.byref(n))
    if rc:
        raise BloomGpuError(rc, L.bsg_last_error(None).decode())
    return out[: n.value].copy()


def rows_to_dense(hdr: np.ndarray, rows: np.ndarray, n_blocks: int, packed: bool = False) -> np.ndarray:
    """[n_queries] headers + [n_queries][G] row slots of bsg_probe_many_rows -> the dense [n_queries][G] bitsets of bsg_probe_many
    (numpy; tests and consumers that want the bitset form).  packed: the rows were written with BSG_PROBE_ROWS_PACKED (payloads of
    every run of 256 queries back to back from the run's first slot)."""
    G = (n_blocks + 63) // 64
    flat = np.asarray(rows, dtype=np.uint64).reshape(-1)
    out = np.zeros((len(hdr), G), dtype=np.uint64)
    full = np.full(G, ~np.uint64(0), dtype=np.uint64)
    if n_blocks & 63:
        full[-1] = np.uint64((1 << (n_blocks & 63)) - 1)
    if packed:      # byte headers: tag << 6 | a LIST row's count (hdr: the first len(hdr) BYTES of what was passed, see packed_headers)
        hdr = np.asarray(hdr)
        hb = hdr if hdr.dtype == np.uint8 else hdr.view(np.uint8)[: len(hdr)]          # (a u32 view of the buffer: its first len(hdr) bytes)
        tag, cnt = (hb >> 6).astype(np.uint32), (hb & 63).astype(np.uint32)
    else:
        tag, cnt = np.asarray(hdr, dtype=np.uint32) >> 30, np.asarray(hdr, dtype=np.uint32) & np.uint32(0x3FFFFFFF)
    out[tag == 1] = full
    size = np.where(tag == 2, (cnt.astype(np.int64) + 1) >> 1, np.where(tag == 3, G, 0))           # payload words per row
    if packed:
        start = np.zeros(len(hdr), dtype=np.int64)
        for r0 in range(0, len(hdr), 256):
            s = size[r0: r0 + 256]
            start[r0: r0 + 256] = r0 * G + np.cumsum(s) - s
    else:
        start = np.arange(len(hdr), dtype=np.int64) * G
    for q in np.nonzero(tag == 3)[0]:
        out[q] = flat[start[q]: start[q] + G]
    for q in np.nonzero(tag == 2)[0]:
        ids = flat[start[q]: start[q] + size[q]].view(np.uint32)[: int(cnt[q])].astype(np.int64)
        np.bitwise_or.at(out[q], ids >> 6, np.uint64(1) << (ids & 63).astype(np.uint64))
    return out


def packed_headers(hdr: np.ndarray, index: int, n_queries: int) -> np.ndarray:
    """The n_queries byte headers of arena (or device x arena) number `index` out of the header buffer of a BSG_PROBE_ROWS_PACKED call."""
    return hdr.view(np.uint8)[index * n_queries: (index + 1) * n_queries]


def estimate_parameters(n: int, p: float):
    """bloom/v3 EstimateParameters with New()'s clamps (host arithmetic, no GPU needed)."""
    L = _lib.load()
    m, k = C.c_uint64(), C.c_uint64()
    rc = L.bsg_estimate_parameters(n, p, C.byref(m), C.byref(k))
    if rc:
        raise BloomGpuError(rc, L.bsg_last_error(None).decode())
    return int(m.value), int(k.value)


def wide_pair_bits(words, pair_word_off, pair: int, n_set_rows: int) -> np.ndarray:
    """The bool row of pair `pair` of a Context.match_rows_wide result, over the n_set_rows rows of its set."""
    w = np.ascontiguousarray(words[int(pair_word_off[pair]): int(pair_word_off[pair + 1])])
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n_set_rows].astype(bool)


def pair_rows_list(hdr: int, payload, set_rows: int, cap=None) -> np.ndarray:
    """bsg_match_pair_rows_list (host arithmetic, no GPU needed): one pair of Context.match_rows_wide_rows, whatever its tag, as the
    ascending set-relative indices of its matching rows (at most cap of them; default: all)."""
    L = _lib.load()
    pl = np.ascontiguousarray(payload, dtype=np.uint32)
    out = np.zeros(max(set_rows if cap is None else cap, 1), dtype=np.uint32)
    n = C.c_uint32()
    rc = L.bsg_match_pair_rows_list(int(hdr), pl.ctypes.data if len(pl) else None, set_rows, out.ctypes.data, set_rows if cap is None else cap, C.byref(n))
    if rc:
        raise BloomGpuError(rc, L.bsg_last_error(None).decode())
    return out[: min(n.value, set_rows if cap is None else cap)].copy()


class Context:
    """bsg_ctx: one or more gfx950 devices, per-device streams."""

    def __init__(self, device_ids=(0,)):
        self.L = _lib.load()
        ids = (C.c_int32 * len(device_ids))(*device_ids)
        h = C.c_void_p()
        rc = self.L.bsg_open(ids, len(device_ids), C.byref(h))
        if rc:
            raise BloomGpuError(rc, self.L.bsg_last_error(None).decode())
        self.h = h
        self.n_devices = len(device_ids)
        self._dependents = weakref.WeakSet()     # objects that hold this handle (host.Engine): closed before the context is
        self._minmax_fields = {}                 # ingest id -> number of MinMax fields (the shape ingest_minmax returns)

    def _check(self, rc):
        if rc:
            raise BloomGpuError(rc, self.L.bsg_last_error(self.h).decode())

    def close(self):
        if self.h:
            for dep in list(self._dependents):
                dep.close()
            self.L.bsg_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._check(self.L.bsg_sync(self.h))

    def device_calls(self) -> np.ndarray:
        """Construct / match parts each device of the context has served so far."""
        out = np.zeros(self.n_devices, dtype=np.uint64)
        self._check(self.L.bsg_device_calls(self.h, _lib._ptr(out), len(out)))
        return out

    # ---- construct ----
    def hash_entries(self, blob: np.ndarray, off: np.ndarray) -> np.ndarray:
        n = len(off) - 1
        out = np.zeros((n, 4), dtype=np.uint64)
        self._check(self.L.bsg_hash_entries(self.h, _lib._ptr(blob), _lib._ptr(off), n, _lib._ptr(out)))
        return out

    def hash_strings(self, entries) -> np.ndarray:
        return self.hash_entries(*pack_entries(entries))

    def build(self, blob, off, filter_entry_start, desc, n_words: int, out: np.ndarray = None) -> np.ndarray:
        """out: where the words go (u64, >= n_words); the callee zero-fills what no filter owns."""
        assert desc.dtype == DESC_DTYPE
        if out is None:
            out = np.empty(n_words, dtype=np.uint64)
        assert out.dtype == np.uint64 and len(out) >= n_words and out.flags.c_contiguous
        fs = np.ascontiguousarray(filter_entry_start, dtype=np.uint32)
        self._check(self.L.bsg_build(self.h, _lib._ptr(blob), _lib._ptr(off), len(off) - 1, _lib._ptr(fs),
                                     _lib._ptr(desc), len(desc), _lib._ptr(out), n_words))
        return out

    def build_hashed(self, h, filter_entry_start, desc, n_words: int, out: np.ndarray = None) -> np.ndarray:
        """out: as build's."""
        assert desc.dtype == DESC_DTYPE
        h = np.ascontiguousarray(h, dtype=np.uint64)
        if out is None:
            out = np.empty(n_words, dtype=np.uint64)
        assert out.dtype == np.uint64 and len(out) >= n_words and out.flags.c_contiguous
        fs = np.ascontiguousarray(filter_entry_start, dtype=np.uint32)
        self._check(self.L.bsg_build_hashed(self.h, _lib._ptr(h), len(h), _lib._ptr(fs), _lib._ptr(desc), len(desc),
                                            _lib._ptr(out), n_words))
        return out

    # ---- probe ----
    def arena_load(self, words: np.ndarray, desc: np.ndarray) -> int:
        assert desc.dtype == DESC_DTYPE and len(desc) % 3 == 0
        words = np.ascontiguousarray(words, dtype=np.uint64)
        aid = C.c_uint64()
        self._check(self.L.bsg_arena_load(self.h, _lib._ptr(words), len(words), _lib._ptr(desc), len(desc) // 3,
                                          C.byref(aid)))
        return int(aid.value)

    def arena_load_sections(self, sections):
        """sections: list[bytes] (b"" = block without a section) -> (arena_id, int32 status per block)."""
        off = np.zeros(len(sections) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in sections], dtype=np.uint64)
        region = np.frombuffer(b"".join(sections), dtype=np.uint8)
        status = np.zeros(max(len(sections), 1), dtype=np.int32)
        aid = C.c_uint64()
        self._check(self.L.bsg_arena_load_sections(self.h, _lib._ptr(region), len(region), _lib._ptr(off), len(sections),
                                                   _lib._ptr(status), C.byref(aid)))
        return int(aid.value), status[: len(sections)]

    def arena_stream_begin(self, sec_begin, sec_end) -> int:
        sb = np.ascontiguousarray(sec_begin, dtype=np.uint64)
        se = np.ascontiguousarray(sec_end, dtype=np.uint64)
        sid = C.c_uint64()
        self._check(self.L.bsg_arena_stream_begin(self.h, _lib._ptr(sb), _lib._ptr(se), len(sb), C.byref(sid)))
        return int(sid.value)

    def arena_stream_append(self, stream_id: int, file_offset: int, data: bytes):
        buf = np.frombuffer(data, dtype=np.uint8)
        self._check(self.L.bsg_arena_stream_append(self.h, stream_id, file_offset, _lib._ptr(buf), len(buf)))

    def arena_stream_finish(self, stream_id: int, n_blocks: int):
        status = np.zeros(max(n_blocks, 1), dtype=np.int32)
        aid = C.c_uint64()
        self._check(self.L.bsg_arena_stream_finish(self.h, stream_id, _lib._ptr(status), C.byref(aid)))
        return int(aid.value), status[:n_blocks]

    def arena_stream_abort(self, stream_id: int):
        self._check(self.L.bsg_arena_stream_abort(self.h, stream_id))

    def arena_free(self, arena_id: int):
        self._check(self.L.bsg_arena_free(self.h, arena_id))

    # ---- resident file arenas across queries (cache_api.inc) ----
    def set_arena_budget(self, n_bytes: int):
        self._check(self.L.bsg_set_arena_budget(self.h, int(n_bytes)))

    def file_arena_acquire(self, key: bytes, block_keys):
        """-> (lease, arena_id, rows) when the file's resident arena covers every block key, else (0, 0, None)."""
        bk = np.ascontiguousarray(block_keys, dtype=np.uint64)
        kb = np.frombuffer(key, dtype=np.uint8)
        rows = np.zeros(max(len(bk), 1), dtype=np.uint32)
        lease, aid = C.c_uint64(), C.c_uint64()
        self._check(self.L.bsg_file_arena_acquire(self.h, _lib._ptr(kb), len(kb), _lib._ptr(bk), len(bk), C.byref(lease), C.byref(aid), None, _lib._ptr(rows)))
        return (int(lease.value), int(aid.value), rows[: len(bk)]) if lease.value else (0, 0, None)

    def file_arena_have(self, key: bytes):
        """Block keys and section extents (file offsets) of the file's resident arena: three u64 arrays (empty when there is none)."""
        kb = np.frombuffer(key, dtype=np.uint8)
        n = C.c_uint32()
        self._check(self.L.bsg_file_arena_have(self.h, _lib._ptr(kb), len(kb), None, None, None, 0, C.byref(n)))
        while True:
            cap = int(n.value)
            keys, sb, se = (np.zeros(max(cap, 1), dtype=np.uint64) for _ in range(3))
            rc = self.L.bsg_file_arena_have(self.h, _lib._ptr(kb), len(kb), _lib._ptr(keys), _lib._ptr(sb), _lib._ptr(se), max(cap, 1), C.byref(n))
            if rc == 0 and int(n.value) <= max(cap, 1):
                m = int(n.value)
                return keys[:m], sb[:m], se[:m]
            if int(n.value) <= cap:             # a real failure, not a wider arena published in between
                self._check(rc)

    def file_arena_publish(self, key: bytes, arena_id: int, block_keys, sec_begin, sec_end, status=None):
        """-> (lease, resident): the cache owns the arena from here on."""
        kb = np.frombuffer(key, dtype=np.uint8)
        bk, sb, se = (np.ascontiguousarray(a, dtype=np.uint64) for a in (block_keys, sec_begin, sec_end))
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        lease, res = C.c_uint64(), C.c_int32()
        self._check(self.L.bsg_file_arena_publish(self.h, _lib._ptr(kb), len(kb), arena_id, _lib._ptr(bk), _lib._ptr(sb), _lib._ptr(se), _lib._ptr(st), len(bk),
                                                  C.byref(lease), C.byref(res)))
        return int(lease.value), bool(res.value)

    def file_arena_release(self, lease: int):
        self._check(self.L.bsg_file_arena_release(self.h, lease))

    def file_arena_forget(self, key: bytes):
        kb = np.frombuffer(key, dtype=np.uint8)
        self._check(self.L.bsg_file_arena_forget(self.h, _lib._ptr(kb), len(kb)))

    def arena_cache_stats(self, reset: bool = False) -> dict:
        st = _lib.ArenaCacheStats()
        self._check(self.L.bsg_arena_cache_stats_read(self.h, C.byref(st), 1 if reset else 0))
        return {f: int(getattr(st, f)) for f, _ in st._fields_}

    def batch_create(self, terms: np.ndarray, prog_ops, prog_off) -> int:
        assert terms.dtype == TERM_DTYPE
        ops = np.ascontiguousarray(prog_ops, dtype=np.uint32)
        off = np.ascontiguousarray(prog_off, dtype=np.uint32)
        bid = C.c_uint64()
        self._check(self.L.bsg_batch_create(self.h, _lib._ptr(terms), len(terms), _lib._ptr(ops), _lib._ptr(off),
                                            len(off) - 1, C.byref(bid)))
        return int(bid.value)

    def batch_free(self, batch_id: int):
        self._check(self.L.bsg_batch_free(self.h, batch_id))

    def probe_batch(self, arena_id: int, batch_id: int, n_queries: int, n_blocks: int, flags: int = 0,
                    want_output: bool = True):
        out = np.zeros((n_queries, (n_blocks + 63) // 64), dtype=np.uint64) if want_output else None
        self._check(self.L.bsg_probe_batch(self.h, arena_id, batch_id, flags, _lib._ptr(out)))
        return out

    def probe_many(self, arena_ids, batch_id: int, flags: int = 0, n_queries: int = 0, n_blocks=None):
        """n_blocks (list, one per arena) given => synchronous, returns a list of survivor arrays."""
        ids = np.ascontiguousarray(arena_ids, dtype=np.uint64)
        if n_blocks is None:
            self._check(self.L.bsg_probe_many(self.h, _lib._ptr(ids), len(ids), batch_id, flags, None))
            return None
        sizes = [n_queries * ((nb + 63) // 64) for nb in n_blocks]
        out = np.zeros(max(sum(sizes), 1), dtype=np.uint64)
        self._check(self.L.bsg_probe_many(self.h, _lib._ptr(ids), len(ids), batch_id, flags, _lib._ptr(out)))
        res, o = [], 0
        for sz, nb in zip(sizes, n_blocks):
            res.append(out[o: o + sz].reshape(n_queries, (nb + 63) // 64))
            o += sz
        return res

    def probe_many_dev(self, arena_ids, batch_id: int, d_out_ptr: int, flags: int = 0):
        """Survivors of every arena, back to back, at a device pointer (single-device contexts)."""
        ids = np.ascontiguousarray(arena_ids, dtype=np.uint64)
        self._check(self.L.bsg_probe_many_dev(self.h, _lib._ptr(ids), len(ids), batch_id, flags, C.c_void_p(d_out_ptr)))

    def probe_many_into(self, arena_ids, batch_id: int, out: np.ndarray, flags: int = 0):
        """Synchronous probe of every arena; survivors written back to back into `out` (u64, e.g. pinned memory)."""
        ids = np.ascontiguousarray(arena_ids, dtype=np.uint64)
        self._check(self.L.bsg_probe_many(self.h, _lib._ptr(ids), len(ids), batch_id, flags, C.c_void_p(out.ctypes.data)))

    def probe_many_rows(self, arena_ids, batch_id: int, rows: np.ndarray, hdr: np.ndarray, flags: int = 0):
        """bsg_probe_many_rows: a header per (arena, query) into `hdr` (u32) and, only where the tag needs it, block ids or words into
        the row's dense slot of `rows` (u64) — both PAGE-LOCKED arrays (pinned_array / host_register), written by the device."""
        ids = np.ascontiguousarray(arena_ids, dtype=np.uint64)
        self._check(self.L.bsg_probe_many_rows(self.h, _lib._ptr(ids), len(ids), batch_id, flags, C.c_void_p(rows.ctypes.data),
                                               C.c_void_p(hdr.ctypes.data)))

    def survivor_rows_size(self, arena_ids, batch_id: int):
        """bsg_survivor_rows_size: (row words, headers) bsg_probe_many_rows writes for these arenas and this batch on this context."""
        ids = np.ascontiguousarray(arena_ids, dtype=np.uint64)
        rw, hw = C.c_uint64(), C.c_uint64()
        self._check(self.L.bsg_survivor_rows_size(self.h, _lib._ptr(ids), len(ids), batch_id, C.byref(rw), C.byref(hw)))
        return int(rw.value), int(hw.value)

    def survivor_rows_list(self, arena_ids, batch_id: int, rows: np.ndarray, hdr: np.ndarray, arena_index: int, query: int, n_blocks: int,
                           packed: bool = False) -> np.ndarray:
        """bsg_survivor_rows_list: the ascending GLOBAL block indices of (arena, query) from the rows bsg_probe_many_rows left — on a
        context of several devices the shards' rows merged (global = local * n_devices + device)."""
        ids = np.ascontiguousarray(arena_ids, dtype=np.uint64)
        out = np.zeros(max(n_blocks, 1), dtype=np.uint32)
        n = C.c_uint32()
        fn = self.L.bsg_survivor_rows_list_packed if packed else self.L.bsg_survivor_rows_list
        self._check(fn(self.h, _lib._ptr(ids), len(ids), batch_id, C.c_void_p(rows.ctypes.data), C.c_void_p(hdr.ctypes.data),
                       arena_index, query, C.c_void_p(out.ctypes.data), len(out), C.byref(n)))
        return out[: int(n.value)]

    def set_probe_group(self, max_arenas_per_launch: int):
        self._check(self.L.bsg_set_probe_group(self.h, max_arenas_per_launch))

    def set_ingest_chunk(self, n_bytes: int):
        self._check(self.L.bsg_set_ingest_chunk(self.h, n_bytes))

    def set_lab(self, key: int, value: int):
        self._check(self.L.bsg_set_lab(self.h, key, value))

    def set_spin_wait(self, microseconds: int):
        self._check(self.L.bsg_set_spin_wait(self.h, microseconds))

    def set_fuse_limit(self, max_arenas: int):
        self._check(self.L.bsg_set_fuse_limit(self.h, max_arenas))

    def set_gather_cost(self, bytes_per_probe: int):
        self._check(self.L.bsg_set_gather_cost(self.h, bytes_per_probe))

    def last_probe_route(self) -> int:
        """_lib.ROUTE_STREAM / ROUTE_GATHER: the kernel family of the last k_probe_terms(_many) / k_probe_gather dispatch (ROUTE_NONE: none yet);
        ROUTE_GATHER_CHUNKED: the last group ran in chunks through k_gather_fused (set_lab key 27)."""
        r = C.c_uint32()
        self._check(self.L.bsg_lab_last_probe_route(self.h, C.byref(r)))
        return int(r.value)

    def scope(self):
        """An error scope: an alias of this context with its own last-error slot (bsg_scope_open)."""
        h = C.c_void_p()
        self._check(self.L.bsg_scope_open(self.h, C.byref(h)))
        sc = Context.__new__(Context)
        sc.L, sc.h, sc.n_devices = self.L, h, self.n_devices
        sc._dependents = weakref.WeakSet()
        sc._minmax_fields = self._minmax_fields
        return sc

    def probe(self, arena_id: int, n_blocks: int, terms: np.ndarray, prog_ops, prog_off) -> np.ndarray:
        assert terms.dtype == TERM_DTYPE
        ops = np.ascontiguousarray(prog_ops, dtype=np.uint32)
        off = np.ascontiguousarray(prog_off, dtype=np.uint32)
        nq = len(off) - 1
        out = np.zeros((nq, (n_blocks + 63) // 64), dtype=np.uint64)
        self._check(self.L.bsg_probe(self.h, arena_id, _lib._ptr(terms), len(terms), _lib._ptr(ops), _lib._ptr(off),
                                     nq, _lib._ptr(out)))
        return out

    def query(self, arena_ids, n_blocks, cb, out: np.ndarray = None):
        """bsg_query: one call, strings in -> survivors out.  cb: query.CompiledBatch (term strings + kinds + programs);
        n_blocks: blocks per arena.  -> list of [n_queries, ceil(n_blocks_i / 64)] u64 arrays."""
        ids = np.ascontiguousarray(arena_ids, dtype=np.uint64)
        if not hasattr(cb, "_packed"):
            tb, to = pack_entries(cb.term_strings)
            ops, poff, kinds = cb.arrays()
            cb._packed = (tb, to, np.ascontiguousarray(kinds, dtype=np.uint32), ops, poff)
        tb, to, kinds, ops, poff = cb._packed
        nq = len(poff) - 1
        sizes = [nq * ((nb + 63) // 64) for nb in n_blocks]
        if out is None:
            out = np.zeros(max(sum(sizes), 1), dtype=np.uint64)
        self._check(self.L.bsg_query(self.h, _lib._ptr(ids), len(ids), _lib._ptr(tb), _lib._ptr(to), _lib._ptr(kinds), len(kinds),
                                     _lib._ptr(ops), _lib._ptr(poff), nq, _lib._ptr(out)))
        res, o = [], 0
        for sz, nb in zip(sizes, n_blocks):
            res.append(out[o: o + sz].reshape(nq, (nb + 63) // 64))
            o += sz
        return res

    def query_stats(self, reset: bool = True) -> dict:
        """How the eligible bsg_query calls were served since the last reset (the combiner of concurrent callers)."""
        t = _lib.QueryStats()
        self._check(self.L.bsg_query_stats_read(self.h, C.byref(t), 1 if reset else 0))
        return {f: int(getattr(t, f)) for f, _ in _lib.QueryStats._fields_}

    def timing_read(self, reset: bool = True) -> Timing:
        t = Timing()
        self._check(self.L.bsg_timing_read(self.h, C.byref(t), 1 if reset else 0))
        return t

    def set_timed_stride(self, stride: int):
        self._check(self.L.bsg_set_timed_stride(self.h, stride))

    def last_kernel_ms(self):
        b, h, dc = C.c_float(), C.c_float(), C.c_float()
        self._check(self.L.bsg_last_kernel_ms(self.h, C.byref(b), C.byref(h), C.byref(dc)))
        return float(b.value), float(h.value), float(dc.value)

    # ---- OR-reduce ----
    def or_reduce(self, arena_id: int, kind: int, n_words: int) -> np.ndarray:
        out = np.zeros(n_words, dtype=np.uint64)
        self._check(self.L.bsg_or_reduce(self.h, arena_id, kind, _lib._ptr(out), n_words))
        return out

    def or_reduce_dev(self, arena_id: int, kind: int, d_out_ptr: int, n_words: int):
        self._check(self.L.bsg_or_reduce_dev(self.h, arena_id, kind, C.c_void_p(d_out_ptr), n_words))

    # ---- RCCL OR all-reduce inside the library ----
    @staticmethod
    def comm_unique_id() -> bytes:
        L = _lib.load()
        buf = (C.c_uint8 * 128)()
        rc = L.bsg_comm_unique_id(buf)
        if rc:
            raise BloomGpuError(rc, L.bsg_last_error(None).decode())
        return bytes(buf)

    def comm_init(self, unique_id=None, rank: int = 0, world: int = 0):
        """unique_id None: every device of this (multi-device) context becomes a rank; else join as `rank` of `world`."""
        if unique_id is None:
            self._check(self.L.bsg_comm_init(self.h, None, 0, 0))
        else:
            buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
            self._check(self.L.bsg_comm_init(self.h, buf, rank, world))

    def peer_access(self) -> np.ndarray:
        """[n][n] u8: 1 where device i reaches device j's memory directly (bsg_peer_access)."""
        n = self.n_devices
        m = np.zeros((n, n), dtype=np.uint8)
        self._check(self.L.bsg_peer_access(self.h, _lib._ptr(m), n))
        return m

    def comm_info(self):
        """(ranks, this rank, asked_the_library) as the communicator library itself reports them (ncclCommCount / ncclCommUserRank)."""
        w, r, lib = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self.L.bsg_comm_info(self.h, C.byref(w), C.byref(r), C.byref(lib)))
        return int(w.value), int(r.value), bool(lib.value)

    def comm_destroy(self):
        self._check(self.L.bsg_comm_destroy(self.h))

    def or_allreduce(self, arena_id: int, kind: int, n_words: int) -> np.ndarray:
        out = np.zeros(n_words, dtype=np.uint64)
        self._check(self.L.bsg_or_allreduce(self.h, arena_id, kind, _lib._ptr(out), n_words))
        return out

    def or_allreduce_dev(self, d_ptrs, n_words: int):
        arr = (C.c_void_p * len(d_ptrs))(*d_ptrs)
        self._check(self.L.bsg_or_allreduce_dev(self.h, arr, n_words))

    def last_or_ms(self) -> float:
        v = C.c_float()
        self._check(self.L.bsg_last_or_ms(self.h, C.byref(v)))
        return float(v.value)

    def or_words_dev(self, d_dst_ptr: int, d_src_ptr: int, n_words: int, n_src: int):
        self._check(self.L.bsg_or_words_dev(self.h, C.c_void_p(d_dst_ptr), C.c_void_p(d_src_ptr), n_words, n_src))

    # ---- device ingest (rows -> distinct entries -> counts -> bitsets) ----
    def ingest_rows(self, rows, set_first_row, parent_of_set=None, n_parents: int = 0, slots_hint=None, flags: int = 0,
                    tokenizer=None, minmax_fields=None) -> int:
        """rows: list[bytes] (or (u8 blob, u64 offsets[n+1])); returns the ingest id.  tokenizer: None = bsg_ingest_rows
        (the default tokenizer); a tokenizer.Tokenizer = bsg_ingest_rows_tok under that spec.  minmax_fields: None, or the names
        (str / bytes) of the top-level keys whose per-set MinMax indexes the call computes too (bsg_ingest_rows_minmax; read them
        with ingest_minmax)."""
        if isinstance(rows, tuple):
            blob, off = rows
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
        else:
            off = np.zeros(len(rows) + 1, dtype=np.uint64)
            if rows:
                off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
            blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
        sfr = np.ascontiguousarray(set_first_row, dtype=np.uint32)
        pos = None if parent_of_set is None else np.ascontiguousarray(parent_of_set, dtype=np.uint32)
        hint = None if slots_hint is None else np.ascontiguousarray(slots_hint, dtype=np.uint32)
        out = C.c_uint64()
        if minmax_fields is not None:
            fblob, foff = pack_entries([f.encode() if isinstance(f, str) else bytes(f) for f in minmax_fields])
            self._check(self.L.bsg_ingest_rows_minmax(self.h, _lib._ptr(blob), _lib._ptr(off), len(off) - 1, _lib._ptr(sfr), len(sfr) - 1,
                                                      _lib._ptr(pos), n_parents, _lib._ptr(hint), flags,
                                                      None if tokenizer is None else c_spec(tokenizer), C.byref(out),
                                                      fblob.ctypes.data, foff.ctypes.data, len(foff) - 1))
            self._minmax_fields[int(out.value)] = len(foff) - 1
            return int(out.value)
        if tokenizer is not None:
            self._check(self.L.bsg_ingest_rows_tok(self.h, _lib._ptr(blob), _lib._ptr(off), len(off) - 1, _lib._ptr(sfr), len(sfr) - 1,
                                                   _lib._ptr(pos), n_parents, _lib._ptr(hint), flags, c_spec(tokenizer), C.byref(out)))
            return int(out.value)
        self._check(self.L.bsg_ingest_rows(self.h, _lib._ptr(blob), _lib._ptr(off), len(off) - 1, _lib._ptr(sfr), len(sfr) - 1,
                                           _lib._ptr(pos), n_parents, _lib._ptr(hint), flags, C.byref(out)))
        return int(out.value)

    # streaming ingest: open without rows, append batches whose rows belong to arbitrary sets, then finish / build as above
    def ingest_open(self, n_sets: int, parent_of_set=None, n_parents: int = 0, slots_hint=None, flags: int = 0, tokenizer=None,
                    minmax_fields=None) -> int:
        pos = None if parent_of_set is None else np.ascontiguousarray(parent_of_set, dtype=np.uint32)
        hint = None if slots_hint is None else np.ascontiguousarray(slots_hint, dtype=np.uint32)
        out = C.c_uint64()
        if minmax_fields is not None:         # bsg_ingest_open_minmax: every append folds its batch into the sets' MinMax indexes
            fblob, foff = pack_entries([f.encode() if isinstance(f, str) else bytes(f) for f in minmax_fields])
            self._check(self.L.bsg_ingest_open_minmax(self.h, n_sets, _lib._ptr(pos), n_parents, _lib._ptr(hint), flags,
                                                      None if tokenizer is None else c_spec(tokenizer), C.byref(out),
                                                      fblob.ctypes.data, foff.ctypes.data, len(foff) - 1))
            self._minmax_fields[int(out.value)] = len(foff) - 1
            return int(out.value)
        self._check(self.L.bsg_ingest_open(self.h, n_sets, _lib._ptr(pos), n_parents, _lib._ptr(hint), flags,
                                           None if tokenizer is None else c_spec(tokenizer), C.byref(out)))
        return int(out.value)

    def ingest_add_sets(self, ingest_id: int, parent_of_new_set, slots_hint=None) -> int:
        """len(parent_of_new_set) more sets; returns the index of the first."""
        pos = np.ascontiguousarray(parent_of_new_set, dtype=np.uint32)
        hint = None if slots_hint is None else np.ascontiguousarray(slots_hint, dtype=np.uint32)
        first = C.c_uint32()
        self._check(self.L.bsg_ingest_add_sets(self.h, ingest_id, len(pos), _lib._ptr(pos), _lib._ptr(hint), C.byref(first)))
        return int(first.value)

    def ingest_append_rows(self, ingest_id: int, rows, set_of_row) -> np.ndarray:
        """rows: list[bytes] (or (u8 blob, u64 offsets[n+1])), row r to set set_of_row[r]; returns the batch-local indices
        (ascending) of the rows the host walker must finish."""
        if isinstance(rows, tuple):
            blob, off = rows
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
        else:
            off = np.zeros(len(rows) + 1, dtype=np.uint64)
            if rows:
                off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
            blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
        sor = np.ascontiguousarray(set_of_row, dtype=np.uint32)
        n_rows = len(off) - 1
        assert len(sor) == n_rows
        fb = np.zeros(n_rows, dtype=np.uint32)
        n = C.c_uint32()
        self._check(self.L.bsg_ingest_append_rows(self.h, ingest_id, _lib._ptr(blob), _lib._ptr(off), n_rows, _lib._ptr(sor),
                                                  _lib._ptr(fb), n_rows, C.byref(n)))
        return fb[: n.value].copy()

    # keyed streaming ingest: the device finds every row's set from the text of one top-level member (bloomgpu.h)
    def ingest_open_keyed(self, partition_field, n_parents: int = 0, parent_of_new_sets: int = 0xFFFFFFFF, flags: int = 0, tokenizer=None,
                          minmax_fields=None) -> int:
        name = partition_field.encode() if isinstance(partition_field, str) else bytes(partition_field)
        nbuf = np.frombuffer(name + b"\0", dtype=np.uint8)
        out = C.c_uint64()
        fblob = foff = None
        if minmax_fields is not None:
            fblob, foff = pack_entries([f.encode() if isinstance(f, str) else bytes(f) for f in minmax_fields])
        self._check(self.L.bsg_ingest_open_keyed(self.h, n_parents, parent_of_new_sets, flags, None if tokenizer is None else c_spec(tokenizer),
                                                 C.byref(out), nbuf.ctypes.data, len(name), _lib._ptr(fblob), _lib._ptr(foff),
                                                 0 if foff is None else len(foff) - 1))
        if foff is not None:
            self._minmax_fields[int(out.value)] = len(foff) - 1
        return int(out.value)

    def ingest_append_rows_keyed(self, ingest_id: int, rows, fallback_cap=None):
        """rows: list[bytes] (or (u8 blob, u64 offsets[n+1])).  -> (set_of_row u32 [n], _lib.SET_UNDECIDED where the partitioner handed
        the row back; number of sets the call created; batch-local indices, ascending, of every row handed back)."""
        if isinstance(rows, tuple):
            blob, off = rows
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
        else:
            off = np.zeros(len(rows) + 1, dtype=np.uint64)
            if rows:
                off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
            blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
        n_rows = len(off) - 1
        cap = n_rows if fallback_cap is None else fallback_cap
        sor = np.zeros(max(n_rows, 1), dtype=np.uint32)
        fb = np.zeros(max(cap, 1), dtype=np.uint32)
        n, n_new = C.c_uint32(), C.c_uint32()
        self._check(self.L.bsg_ingest_append_rows_keyed(self.h, ingest_id, _lib._ptr(blob), _lib._ptr(off), n_rows, _lib._ptr(sor), C.byref(n_new),
                                                        _lib._ptr(fb), cap, C.byref(n)))
        return sor[:n_rows].copy(), int(n_new.value), fb[: n.value].copy()

    def ingest_add_sets_keyed(self, ingest_id: int, keys) -> np.ndarray:
        """keys: list[bytes] of partition texts found on the host -> their sets (known texts keep theirs, new ones get the next)."""
        blob, off = pack_entries([k.encode() if isinstance(k, str) else bytes(k) for k in keys])
        out = np.zeros(max(len(off) - 1, 1), dtype=np.uint32)
        self._check(self.L.bsg_ingest_add_sets_keyed(self.h, ingest_id, blob.ctypes.data, off.ctypes.data, len(off) - 1, out.ctypes.data))
        return out[: len(off) - 1].copy()

    def ingest_keys(self, ingest_id: int, first: int = 0) -> list:
        """the partition texts of sets [first, n_sets) of a keyed ingest"""
        n, nb = C.c_uint32(), C.c_uint64()
        self._check(self.L.bsg_ingest_keys(self.h, ingest_id, first, None, 0, None, C.byref(n), C.byref(nb)))
        blob = np.zeros(max(int(nb.value), 1), dtype=np.uint8)
        off = np.zeros(n.value + 1, dtype=np.uint32)
        self._check(self.L.bsg_ingest_keys(self.h, ingest_id, first, blob.ctypes.data, int(nb.value), off.ctypes.data, C.byref(n), C.byref(nb)))
        raw = blob.tobytes()
        return [raw[int(off[i]): int(off[i + 1])] for i in range(n.value)]

    def last_partition_ms(self) -> float:
        v = C.c_float()
        self._check(self.L.bsg_last_partition_ms(self.h, C.byref(v)))
        return float(v.value)

    def ingest_minmax(self, ingest_id: int, n_sets: int):
        """The MinMax indexes of an ingest made with minmax_fields, as the device folded them (the rows it handed back are NOT in:
        fold them in with host.minmax_row): (min i64, max i64, present bool), each of shape (n_sets, n_fields); min = max = 0
        where present is False."""
        nf = self._minmax_fields.get(int(ingest_id), 1)
        rec = np.zeros(max(n_sets * nf, 1), dtype=_lib.MINMAX_DTYPE)
        self._check(self.L.bsg_ingest_minmax(self.h, ingest_id, rec.ctypes.data, len(rec)))
        rec = rec[: n_sets * nf].reshape(n_sets, nf)
        return rec["min"].copy(), rec["max"].copy(), rec["present"] != 0

    def last_minmax_ms(self) -> float:
        v = C.c_float()
        self._check(self.L.bsg_last_minmax_ms(self.h, C.byref(v)))
        return float(v.value)

    def ingest_fallback_rows(self, ingest_id: int) -> np.ndarray:
        n = C.c_uint32()
        self._check(self.L.bsg_ingest_fallback_rows(self.h, ingest_id, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self._check(self.L.bsg_ingest_fallback_rows(self.h, ingest_id, _lib._ptr(out), n.value, C.byref(n)))
        return out

    def ingest_add_entries(self, ingest_id: int, entries, set_of_entry, kind_of_entry):
        blob, off = pack_entries(entries)
        so = np.ascontiguousarray(set_of_entry, dtype=np.uint32)
        ko = np.ascontiguousarray(kind_of_entry, dtype=np.uint32)
        self._check(self.L.bsg_ingest_add_entries(self.h, ingest_id, _lib._ptr(blob), _lib._ptr(off), len(off) - 1,
                                                  _lib._ptr(so), _lib._ptr(ko)))

    def ingest_finish(self, ingest_id: int, n_sets_total: int):
        """-> (counts u64 [n_sets_total, 3], status u32 [n_sets_total])"""
        counts = np.zeros((n_sets_total, 3), dtype=np.uint64)
        status = np.zeros(n_sets_total, dtype=np.uint32)
        self._check(self.L.bsg_ingest_finish(self.h, ingest_id, _lib._ptr(counts), _lib._ptr(status)))
        return counts, status

    def ingest_build(self, ingest_id: int, desc, n_words: int, out: np.ndarray = None) -> np.ndarray:
        """out: where the words go (u64, >= n_words; e.g. a view of pinned_array memory: the copy back is then plain DMA)."""
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        if out is None:
            out = np.empty(n_words, dtype=np.uint64)
        assert out.dtype == np.uint64 and len(out) >= n_words
        self._check(self.L.bsg_ingest_build(self.h, ingest_id, _lib._ptr(desc), _lib._ptr(out), n_words))
        return out

    def sections_size(self, desc) -> int:
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        total = C.c_uint64()
        self._check(self.L.bsg_sections_size(_lib._ptr(desc), len(desc) // 3, C.byref(total)))
        return int(total.value)

    def _split_sections(self, region: np.ndarray, sec_off: np.ndarray):
        raw = region.tobytes()
        return [raw[int(sec_off[i]): int(sec_off[i + 1])] for i in range(len(sec_off) - 1)]

    def build_sections(self, blob, off, filter_entry_start, desc, n_words: int):
        """bsg_build + encodeFilterSection on the device -> list of section bytes (one per block)."""
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        fstart = np.ascontiguousarray(filter_entry_start, dtype=np.uint32)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        region = np.zeros(self.sections_size(desc), dtype=np.uint8)
        sec_off = np.zeros(len(desc) // 3 + 1, dtype=np.uint64)
        self._check(self.L.bsg_build_sections(self.h, _lib._ptr(blob), _lib._ptr(off), len(off) - 1, _lib._ptr(fstart), _lib._ptr(desc),
                                              len(desc), n_words, _lib._ptr(region), len(region), _lib._ptr(sec_off)))
        return self._split_sections(region, sec_off)

    def ingest_build_sections(self, ingest_id: int, desc, arenas: bool = False):
        """-> sections (list of bytes, sets then parents); with arenas=True also (sets_arena_id, parents_arena_id)."""
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        region = np.zeros(self.sections_size(desc), dtype=np.uint8)
        sec_off = np.zeros(len(desc) // 3 + 1, dtype=np.uint64)
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.bsg_ingest_build_sections(self.h, ingest_id, _lib._ptr(desc), _lib._ptr(region), len(region),
                                                     _lib._ptr(sec_off), C.byref(a) if arenas else None, C.byref(b) if arenas else None))
        secs = self._split_sections(region, sec_off)
        return (secs, int(a.value), int(b.value)) if arenas else secs

    def last_encode_ms(self) -> float:
        v = C.c_float()
        self._check(self.L.bsg_last_encode_ms(self.h, C.byref(v)))
        return float(v.value)

    # ---- pinned host memory ----
    def pinned_array(self, n_bytes: int) -> np.ndarray:
        """A u8 numpy view of n_bytes of pinned host memory (freed by pinned_free(array))."""
        p = C.c_void_p()
        self._check(self.L.bsg_pinned_alloc(self.h, n_bytes, C.byref(p)))
        buf = (C.c_uint8 * max(n_bytes, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8, count=n_bytes)
        return arr

    def pinned_free(self, arr: np.ndarray):
        self._check(self.L.bsg_pinned_free(self.h, C.c_void_p(arr.ctypes.data)))

    def host_register(self, arr: np.ndarray):
        self._check(self.L.bsg_host_register(self.h, C.c_void_p(arr.ctypes.data), arr.nbytes))

    def host_unregister(self, arr: np.ndarray):
        self._check(self.L.bsg_host_unregister(self.h, C.c_void_p(arr.ctypes.data)))

    # ---- final row test on the device ----
    def match_rows(self, rows, matcher, tokenizer=None):
        """rows: list[bytes] or (u8 blob, u64 offsets); matcher: query.CompiledMatcher.
        -> (bool array [n_rows], sorted u32 array of rows the host matcher must decide).
        tokenizer: None = bsg_match_rows; a tokenizer.Tokenizer = bsg_match_rows_tok under that spec."""
        return self._match_rows(self.L.bsg_match_rows, rows, matcher, tokenizer)

    def match_rows_regex(self, rows, matcher, tokenizer=None):
        """bsg_match_rows_regex: as match_rows, and the matcher (query.CompiledRowQuery) may hold FieldRegex conditions."""
        return self._match_rows(self.L.bsg_match_rows_regex, rows, matcher, tokenizer)

    def match_rows_substr(self, rows, matcher, tokenizer=None):
        """bsg_match_rows_substr: as match_rows, and the matcher (query.CompiledSubstringQuery) may hold Substring / FieldSubstring
        conditions (raw needles; the call folds them under `tokenizer`, None = the default)."""
        return self._match_rows(None, rows, matcher, tokenizer, tok_fn=self.L.bsg_match_rows_substr)

    def match_rows_range(self, rows, matcher, tokenizer=None):
        """bsg_match_rows_range: as match_rows, and the matcher (query.CompiledRangeQuery) may hold FieldRange conditions.  Rows with an
        exponent literal on a range field come back as fallback rows (host.match_row_range decides them)."""
        return self._match_rows(None, rows, matcher, tokenizer, tok_fn=self.L.bsg_match_rows_range)

    def match_rows_regex_substr(self, rows, matcher, tokenizer=None):
        """bsg_match_rows_regex_substr: as match_rows_substr, and the matcher (query.CompiledRowSubstringQuery) may hold FieldRegex
        conditions in the same table: one walk of the rows decides both kinds."""
        return self._match_rows(None, rows, matcher, tokenizer, tok_fn=self.L.bsg_match_rows_regex_substr)

    def match_rows_regex_substr_range(self, rows, matcher, tokenizer=None):
        """bsg_match_rows_regex_substr_range: as match_rows_regex_substr, and the matcher (query.CompiledRowTextRangeQuery) may hold
        FieldRange conditions in the same table: one walk of the rows decides range, regex and substring conditions."""
        return self._match_rows(None, rows, matcher, tokenizer, tok_fn=self.L.bsg_match_rows_regex_substr_range)

    def _match_rows(self, fn, rows, matcher, tokenizer=None, tok_fn=None):
        if isinstance(rows, tuple):
            blob = np.ascontiguousarray(rows[0], dtype=np.uint8)
            off = np.ascontiguousarray(rows[1], dtype=np.uint64)
        else:
            off = np.zeros(len(rows) + 1, dtype=np.uint64)
            if rows:
                off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
            blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
        n = len(off) - 1
        strings = [s for pair in zip(matcher.fields, matcher.tokens) for s in pair]      # field 0, token 0, field 1, ...
        cblob, coff = pack_entries(strings)
        kinds = np.asarray(matcher.kinds, dtype=np.uint32)
        ops = np.asarray(matcher.prog_ops, dtype=np.uint32)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        fb = np.zeros(max(n, 1), dtype=np.uint32)
        nfb = C.c_uint32()
        if tokenizer is not None or tok_fn is not None:
            self._check((tok_fn or self.L.bsg_match_rows_tok)(self.h, _lib._ptr(blob), _lib._ptr(off), n, _lib._ptr(cblob), _lib._ptr(coff), _lib._ptr(kinds),
                                                  len(kinds), _lib._ptr(ops), len(ops), c_spec(tokenizer), _lib._ptr(bits), _lib._ptr(fb), len(fb),
                                                  C.byref(nfb)))
        else:
            self._check(fn(self.h, _lib._ptr(blob), _lib._ptr(off), n, _lib._ptr(cblob), _lib._ptr(coff), _lib._ptr(kinds), len(kinds),
                           _lib._ptr(ops), len(ops), _lib._ptr(bits), _lib._ptr(fb), len(fb), C.byref(nfb)))
        match = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n].astype(bool)
        return match, fb[: nfb.value].copy()

    def match_rows_many(self, rows, batch, set_first_row=None, masks=None, tokenizer=None):
        """bsg_match_rows_many: rows as match_rows; batch: query.CompiledMatcherBatch (or anything with its kinds / fields / tokens /
        prog_ops / prog_off).  set_first_row [n_sets + 1] and masks [n_sets] (u64, bit q = evaluate query q on the set): both
        None = every query on every row.  -> (bool planes [n_queries, n_rows], sorted u32 array of rows the host matcher must decide)."""
        return self._match_rows_many(self.L.bsg_match_rows_many, rows, batch, set_first_row, masks, tokenizer)

    def match_rows_many_regex(self, rows, batch, set_first_row=None, masks=None, tokenizer=None):
        """bsg_match_rows_many_regex: as match_rows_many, and the batch (query.CompiledRowQueryBatch) may hold FieldRegex conditions."""
        return self._match_rows_many(self.L.bsg_match_rows_many_regex, rows, batch, set_first_row, masks, tokenizer)

    def match_rows_many_substr(self, rows, batch, set_first_row=None, masks=None, tokenizer=None):
        """bsg_match_rows_many_substr: as match_rows_many, and the batch (query.CompiledSubstringQueryBatch) may hold Substring /
        FieldSubstring conditions."""
        return self._match_rows_many(self.L.bsg_match_rows_many_substr, rows, batch, set_first_row, masks, tokenizer)

    def match_rows_many_range(self, rows, batch, set_first_row=None, masks=None, tokenizer=None):
        """bsg_match_rows_many_range: as match_rows_many, and the batch (query.CompiledRangeQueryBatch) may hold FieldRange conditions."""
        return self._match_rows_many(self.L.bsg_match_rows_many_range, rows, batch, set_first_row, masks, tokenizer)

    def match_rows_many_regex_substr(self, rows, batch, set_first_row=None, masks=None, tokenizer=None):
        """bsg_match_rows_many_regex_substr: as match_rows_many, and the batch (query.CompiledRowSubstringQueryBatch) may hold FieldRegex,
        Substring and FieldSubstring conditions in one table."""
        return self._match_rows_many(self.L.bsg_match_rows_many_regex_substr, rows, batch, set_first_row, masks, tokenizer)

    def match_rows_many_regex_substr_range(self, rows, batch, set_first_row=None, masks=None, tokenizer=None):
        """bsg_match_rows_many_regex_substr_range: as match_rows_many, and the batch (query.CompiledRowTextRangeQueryBatch) may hold
        FieldRegex, Substring, FieldSubstring and FieldRange conditions in one table."""
        return self._match_rows_many(self.L.bsg_match_rows_many_regex_substr_range, rows, batch, set_first_row, masks, tokenizer)

    def _match_rows_many(self, fn, rows, batch, set_first_row, masks, tokenizer):
        if isinstance(rows, tuple):
            blob = np.ascontiguousarray(rows[0], dtype=np.uint8)
            off = np.ascontiguousarray(rows[1], dtype=np.uint64)
        else:
            off = np.zeros(len(rows) + 1, dtype=np.uint64)
            if rows:
                off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
            blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
        n = len(off) - 1
        cblob, coff = pack_entries([s for pair in zip(batch.fields, batch.tokens) for s in pair])
        kinds = np.asarray(batch.kinds, dtype=np.uint32)
        ops = np.asarray(batch.prog_ops, dtype=np.uint32)
        poff = np.asarray(batch.prog_off, dtype=np.uint32)
        nq, n_words = len(poff) - 1, (n + 63) // 64
        if (set_first_row is None) != (masks is None):
            raise ValueError("set_first_row and masks go together")
        sfr = None if set_first_row is None else np.ascontiguousarray(set_first_row, dtype=np.uint32)
        msk = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint64)
        if sfr is not None and len(sfr) != len(msk) + 1:
            raise ValueError("set_first_row holds one more entry than masks")
        bits = np.zeros((nq, n_words), dtype=np.uint64)
        fb = np.zeros(max(n, 1), dtype=np.uint32)
        nfb = C.c_uint32()
        self._check(fn(self.h, _lib._ptr(blob), _lib._ptr(off), n, _lib._ptr(cblob), _lib._ptr(coff), _lib._ptr(kinds),
                       len(kinds), _lib._ptr(ops), poff.ctypes.data, nq, _lib._ptr(sfr), _lib._ptr(msk),
                       0 if msk is None else len(msk), None if tokenizer is None else c_spec(tokenizer),
                       _lib._ptr(bits), _lib._ptr(fb), len(fb), C.byref(nfb)))
        planes = np.unpackbits(bits.view(np.uint8).reshape(nq, n_words * 8), axis=1, bitorder="little")[:, :n].astype(bool)
        return planes, fb[: nfb.value].copy()

    def _wide_args(self, rows, batch, set_first_row, set_query_off, set_queries, tokenizer):
        """What bsg_match_rows_wide and bsg_match_rows_wide_rows take up to and including tok -> (the arguments, the arrays they point
        into, n_rows, pair_word_off, total words)."""
        if isinstance(rows, tuple):
            blob = np.ascontiguousarray(rows[0], dtype=np.uint8)
            off = np.ascontiguousarray(rows[1], dtype=np.uint64)
        else:
            off = np.zeros(len(rows) + 1, dtype=np.uint64)
            if rows:
                off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
            blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
        n = len(off) - 1
        cblob, coff = pack_entries([s for pair in zip(batch.fields, batch.tokens) for s in pair])
        kinds = np.asarray(batch.kinds, dtype=np.uint32)
        ops = np.asarray(batch.prog_ops, dtype=np.uint32)
        poff = np.asarray(batch.prog_off, dtype=np.uint32)
        nq = len(poff) - 1
        given = [a is not None for a in (set_first_row, set_query_off, set_queries)]
        if any(given) and not all(given):
            raise ValueError("set_first_row, set_query_off and set_queries go together")
        sfr = sqo = sq = None
        if all(given):
            sfr = np.ascontiguousarray(set_first_row, dtype=np.uint32)
            sqo = np.ascontiguousarray(set_query_off, dtype=np.uint32)
            sq = np.ascontiguousarray(set_queries, dtype=np.uint32)
            if len(sfr) != len(sqo) or len(sfr) < 2:
                raise ValueError("set_first_row and set_query_off hold one entry per set and one more")
        n_sets = 0 if sfr is None else len(sfr) - 1
        pair_word_off, total = self.match_wide_size(sfr, sqo, n, nq)
        if sq is not None and len(sq) != len(pair_word_off) - 1:
            raise ValueError("set_queries holds set_query_off[n_sets] entries")
        spec = None if tokenizer is None else c_spec(tokenizer)
        args = (self.h, _lib._ptr(blob), _lib._ptr(off), n, _lib._ptr(cblob), _lib._ptr(coff), _lib._ptr(kinds), len(kinds), _lib._ptr(ops),
                poff.ctypes.data, nq, _lib._ptr(sfr), _lib._ptr(sqo), None if sq is None else sq.ctypes.data, n_sets, spec)
        return args, (blob, off, cblob, coff, kinds, ops, poff, sfr, sqo, sq, spec), n, pair_word_off, total

    def match_rows_wide(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None):
        """bsg_match_rows_wide: rows as match_rows; batch: query.CompiledWideBatch (or anything with kinds / fields / tokens / prog_ops /
        prog_off), any number of queries.  set_first_row [n_sets + 1], set_query_off [n_sets + 1] and set_queries (CSR: the queries
        evaluated on each set, strictly ascending): all None = one implicit set of all rows with every query.
        -> (u64 words, u64 pair_word_off [n_pairs + 1], sorted u32 array of rows the host matcher must decide): pair p's bit row is
        words[pair_word_off[p]: pair_word_off[p + 1]] (wide_pair_bits unpacks it)."""
        return self._wide_bits(self.L.bsg_match_rows_wide, rows, batch, set_first_row, set_query_off, set_queries, tokenizer)

    def _wide_bits(self, call, rows, batch, set_first_row, set_query_off, set_queries, tokenizer):
        """bsg_match_rows_wide, bsg_match_rows_wide_substr, bsg_match_rows_wide_range, bsg_match_rows_lookup or bsg_match_rows_lookup_regex (one argument list, one result)"""
        args, _keep, n, pair_word_off, total = self._wide_args(rows, batch, set_first_row, set_query_off, set_queries, tokenizer)
        words = np.zeros(total, dtype=np.uint64)
        fb = np.zeros(max(n, 1), dtype=np.uint32)
        nfb = C.c_uint32()
        self._check(call(*args, words.ctypes.data, _lib._ptr(fb), len(fb), C.byref(nfb)))
        return words, pair_word_off, fb[: nfb.value].copy()

    def match_rows_wide_rows(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None, payload_cap=None):
        """bsg_match_rows_wide_rows: the arguments of match_rows_wide; payload_cap (u32 of payload the buffer holds) defaults to the
        bound, 2 per result word.  -> (u32 headers [n_pairs], u64 pair_off [n_pairs + 1], u32 payload [its length], sorted u32 array of
        rows the host matcher must decide): pair p is pair_rows_list(hdr[p], payload[pair_off[p]: pair_off[p + 1]], rows of its set)."""
        return self._wide_rows(self.L.bsg_match_rows_wide_rows, rows, batch, set_first_row, set_query_off, set_queries, tokenizer, payload_cap)

    def _wide_rows(self, call, rows, batch, set_first_row, set_query_off, set_queries, tokenizer, payload_cap):
        """bsg_match_rows_wide_rows, bsg_match_rows_wide_substr_rows, bsg_match_rows_wide_range_rows, bsg_match_rows_lookup_rows or bsg_match_rows_lookup_regex_rows (one argument list, one result)"""
        args, _keep, n, pair_word_off, total = self._wide_args(rows, batch, set_first_row, set_query_off, set_queries, tokenizer)
        n_pairs = len(pair_word_off) - 1
        cap = 2 * total if payload_cap is None else int(payload_cap)
        hdr = np.zeros(n_pairs, dtype=np.uint32)
        pair_off = np.zeros(n_pairs + 1, dtype=np.uint64)
        payload = np.zeros(max(cap, 1), dtype=np.uint32)
        length = C.c_uint64()
        fb = np.zeros(max(n, 1), dtype=np.uint32)
        nfb = C.c_uint32()
        self._check(call(*args, _lib._ptr(hdr), pair_off.ctypes.data, payload.ctypes.data, cap, C.byref(length), _lib._ptr(fb), len(fb), C.byref(nfb)))
        return hdr, pair_off, payload[: length.value].copy(), fb[: nfb.value].copy()

    def match_rows_wide_substr(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None):
        """bsg_match_rows_wide_substr: match_rows_wide's arguments and result, and the batch (query.CompiledRowSubstringQueryBatch, any
        number of queries) may hold FieldRegex, Substring and FieldSubstring conditions in one table."""
        return self._wide_bits(self.L.bsg_match_rows_wide_substr, rows, batch, set_first_row, set_query_off, set_queries, tokenizer)

    def match_rows_wide_substr_rows(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None, payload_cap=None):
        """bsg_match_rows_wide_substr_rows: match_rows_wide_rows' arguments and result over such a table."""
        return self._wide_rows(self.L.bsg_match_rows_wide_substr_rows, rows, batch, set_first_row, set_query_off, set_queries, tokenizer, payload_cap)

    def match_rows_wide_range(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None):
        """bsg_match_rows_wide_range: match_rows_wide's arguments and result, and the batch (query.CompiledWideRangeBatch, any number of
        queries) may hold FieldRange conditions.  A row with an exponent literal on the leaf of a range condition that a listed query
        of the row's set uses comes back as a fallback row."""
        return self._wide_bits(self.L.bsg_match_rows_wide_range, rows, batch, set_first_row, set_query_off, set_queries, tokenizer)

    def match_rows_wide_range_rows(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None, payload_cap=None):
        """bsg_match_rows_wide_range_rows: match_rows_wide_rows' arguments and result over such a table."""
        return self._wide_rows(self.L.bsg_match_rows_wide_range_rows, rows, batch, set_first_row, set_query_off, set_queries, tokenizer, payload_cap)

    def match_rows_wide_regex_substr_range(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None):
        """bsg_match_rows_wide_regex_substr_range: match_rows_wide's arguments and result, and the batch (query.CompiledWideTextRangeBatch,
        any number of queries) may hold all seven condition kinds in one table.  Regex and range conditions are gated by the set's
        queries, needles are not; a row is handed back by the union of match_rows_wide_substr's and match_rows_wide_range's rules."""
        return self._wide_bits(self.L.bsg_match_rows_wide_regex_substr_range, rows, batch, set_first_row, set_query_off, set_queries, tokenizer)

    def match_rows_wide_regex_substr_range_rows(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None, payload_cap=None):
        """bsg_match_rows_wide_regex_substr_range_rows: match_rows_wide_rows' arguments and result over such a table."""
        return self._wide_rows(self.L.bsg_match_rows_wide_regex_substr_range_rows, rows, batch, set_first_row, set_query_off, set_queries, tokenizer, payload_cap)

    def match_rows_wide_hist(self, rows, batch, field, origin: int, width: int, n_buckets: int, set_first_row=None, set_query_off=None,
                             set_queries=None, tokenizer=None):
        """bsg_match_rows_wide_hist: match_rows_wide_regex_substr_range's rows, batch and sets; field (bytes or str): a top-level key
        whose number value buckets a matching row (bucket (floor(v) - origin) // width of n_buckets).
        -> (u32 counts [n_pairs, n_buckets + 3]: the buckets, then below, above and missing; sorted u32 array of rows the host must
        decide, match and bucket both: they are counted in no slot)."""
        args, _keep, n, pair_word_off, _total = self._wide_args(rows, batch, set_first_row, set_query_off, set_queries, tokenizer)
        name = field.encode() if isinstance(field, str) else bytes(field)
        n_pairs = len(pair_word_off) - 1
        slots = _lib.HIST_SLOTS(int(n_buckets))
        counts = np.zeros(max(n_pairs * slots, 1), dtype=np.uint32)
        fb = np.zeros(max(n, 1), dtype=np.uint32)
        nfb = C.c_uint32()
        self._check(self.L.bsg_match_rows_wide_hist(*args, name, len(name), int(origin), int(width), int(n_buckets), counts.ctypes.data,
                                                    _lib._ptr(fb), len(fb), C.byref(nfb)))
        return counts[: n_pairs * slots].reshape(n_pairs, slots), fb[: nfb.value].copy()

    def last_hist_ms(self) -> float:
        """bsg_last_hist_ms: the bucket scanner (summed over chunks) plus the counting pass of the last match_rows_wide_hist"""
        v = C.c_float()
        self._check(self.L.bsg_last_hist_ms(self.h, C.byref(v)))
        return float(v.value)

    def match_rows_lookup(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None):
        """bsg_match_rows_lookup: match_rows_wide's arguments and result over a table of up to 1 024 Field / Token / FieldToken
        conditions (batch: query.CompiledLookupBatch, or anything with kinds / fields / tokens / prog_ops / prog_off)."""
        return self._wide_bits(self.L.bsg_match_rows_lookup, rows, batch, set_first_row, set_query_off, set_queries, tokenizer)

    def match_rows_lookup_rows(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None, payload_cap=None):
        """bsg_match_rows_lookup_rows: match_rows_wide_rows' arguments and result over such a table."""
        return self._wide_rows(self.L.bsg_match_rows_lookup_rows, rows, batch, set_first_row, set_query_off, set_queries, tokenizer, payload_cap)

    def match_rows_lookup_regex(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None):
        """bsg_match_rows_lookup_regex: match_rows_lookup with FieldRegex conditions allowed in the table, at most 16 distinct ones
        (batch: query.CompiledLookupRegexBatch, or anything with kinds / fields / tokens / prog_ops / prog_off)."""
        return self._wide_bits(self.L.bsg_match_rows_lookup_regex, rows, batch, set_first_row, set_query_off, set_queries, tokenizer)

    def match_rows_lookup_regex_rows(self, rows, batch, set_first_row=None, set_query_off=None, set_queries=None, tokenizer=None, payload_cap=None):
        """bsg_match_rows_lookup_regex_rows: match_rows_wide_rows' arguments and result over such a table."""
        return self._wide_rows(self.L.bsg_match_rows_lookup_regex_rows, rows, batch, set_first_row, set_query_off, set_queries, tokenizer, payload_cap)

    def match_wide_size(self, set_first_row, set_query_off, n_rows: int, n_queries: int):
        """bsg_match_wide_size (host arithmetic) -> (u64 pair_word_off [n_pairs + 1], total words); None, None = the implicit set."""
        sfr = None if set_first_row is None else np.ascontiguousarray(set_first_row, dtype=np.uint32)
        sqo = None if set_query_off is None else np.ascontiguousarray(set_query_off, dtype=np.uint32)
        n_sets = 0 if sfr is None else len(sfr) - 1
        n_pairs = n_queries if sqo is None or len(sqo) == 0 else int(sqo[-1])
        pwo = np.zeros(n_pairs + 1, dtype=np.uint64)
        total = C.c_uint64()
        self._check(self.L.bsg_match_wide_size(_lib._ptr(sfr), _lib._ptr(sqo), n_sets, n_rows, n_queries, pwo.ctypes.data, C.byref(total)))
        return pwo, int(total.value)

    def last_match_ms(self) -> float:
        v = C.c_float()
        self._check(self.L.bsg_last_match_ms(self.h, C.byref(v)))
        return float(v.value)

    def ingest_stats(self, ingest_id: int) -> IngestStats:
        st = IngestStats()
        self._check(self.L.bsg_ingest_stats_read(self.h, ingest_id, C.byref(st)))
        return st

    def ingest_free(self, ingest_id: int):
        self._minmax_fields.pop(int(ingest_id), None)
        self._check(self.L.bsg_ingest_free(self.h, ingest_id))
