"""ctypes wrapper over include/bloomsearch_host.h — the C++ host-side mirror of the reference's
tokenizer / walker / entry sets / query algebra / section codec / engine surface.
Test and bench glue only."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _lib
from ._lib import TERM_DTYPE
from .tokenizer import c_spec

HOST_EXPORTS = [
    "bsh_free", "bsh_tokenize", "bsh_tokenize_with", "bsh_entry_sets_new", "bsh_entry_sets_free", "bsh_entry_sets_index_row",
    "bsh_entry_sets_index_row_with",
    "bsh_entry_sets_union_into", "bsh_entry_sets_counts", "bsh_entry_sets_export_sizes", "bsh_entry_sets_export",
    "bsh_batch_new", "bsh_batch_free", "bsh_batch_add_query", "bsh_batch_sizes", "bsh_batch_export", "bsh_match_row", "bsh_match_row_with", "bsh_prune_query", "bsh_match_row_regex",
    "bsh_substring_terms", "bsh_prune_query_sub", "bsh_match_row_substring",
    "bsh_match_row_range", "bsh_prune_query_range",
    "bsh_minmax_row", "bsh_minmax_eval", "bsh_prefilter_eval", "bsh_partition_key", "bsh_hist_row",
    "bsh_regex_match",
    "bsh_section_encode", "bsh_section_parse", "bsh_crc32c",
    "bse_open", "bse_close", "bse_last_error", "bse_stop", "bse_ingest_rows", "bse_flush", "bse_merge", "bse_query", "bse_query_many",
    "bse_describe", "bse_match_calls", "bse_corrupt_section_byte", "bse_section_bytes",
]

_H = None


class HostError(RuntimeError):
    def __init__(self, code, message=""):
        super().__init__(f"host error {code}: {message}")
        self.code = code


def lib():
    global _H
    if _H is not None:
        return _H
    L = _lib.load()
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    pp, pu64 = C.POINTER(vp), C.POINTER(u64)
    L.bsh_free.argtypes = [vp]; L.bsh_free.restype = None
    L.bsh_tokenize.argtypes = [C.c_char_p, u64, pp, pu64]
    L.bsh_entry_sets_new.restype = vp
    L.bsh_entry_sets_free.argtypes = [vp]; L.bsh_entry_sets_free.restype = None
    L.bsh_entry_sets_index_row.argtypes = [vp, C.c_char_p, u64]
    L.bsh_tokenize_with.argtypes = [C.c_char_p, u64, C.POINTER(_lib.Tokenizer), pp, pu64]
    L.bsh_entry_sets_index_row_with.argtypes = [vp, C.c_char_p, u64, C.POINTER(_lib.Tokenizer)]
    L.bsh_entry_sets_union_into.argtypes = [vp, vp]
    L.bsh_entry_sets_counts.argtypes = [vp, pu64]; L.bsh_entry_sets_counts.restype = None
    L.bsh_entry_sets_export_sizes.argtypes = [vp, u32, pu64, pu64]
    L.bsh_entry_sets_export.argtypes = [vp, u32, vp, vp]
    L.bsh_batch_new.restype = vp
    L.bsh_batch_free.argtypes = [vp]; L.bsh_batch_free.restype = None
    L.bsh_batch_add_query.argtypes = [vp, C.c_char_p, u64]
    L.bsh_batch_sizes.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), pu64]; L.bsh_batch_sizes.restype = None
    L.bsh_batch_export.argtypes = [vp, vp, vp, vp, vp, vp]
    L.bsh_match_row.argtypes = [C.c_char_p, u64, C.c_char_p, u64]
    L.bsh_match_row_with.argtypes = [C.c_char_p, u64, C.c_char_p, u64, C.POINTER(_lib.Tokenizer)]
    L.bsh_prune_query.argtypes = [C.c_char_p, u64, C.c_char_p, u64, pp, pu64]
    L.bsh_match_row_regex.argtypes = [C.c_char_p, u64, C.c_char_p, u64]
    L.bsh_regex_match.argtypes = [C.c_char_p, u64, C.c_char_p, u64]
    L.bsh_substring_terms.argtypes = [C.c_char_p, u64, C.POINTER(_lib.Tokenizer), pp, pu64]
    L.bsh_prune_query_sub.argtypes = [C.c_char_p, u64, C.c_char_p, u64, C.c_char_p, u64, C.POINTER(_lib.Tokenizer), pp, pu64]
    L.bsh_match_row_substring.argtypes = [C.c_char_p, u64, C.c_char_p, u64, C.POINTER(_lib.Tokenizer)]
    L.bsh_match_row_range.argtypes = [C.c_char_p, u64, C.c_char_p, u64]
    L.bsh_prune_query_range.argtypes = [C.c_char_p, u64, C.c_char_p, u64, C.c_char_p, u64, C.c_char_p, u64, C.POINTER(_lib.Tokenizer), pp, pu64]
    L.bsh_minmax_row.argtypes = [C.c_char_p, u64, vp, vp, u32, vp]
    L.bsh_partition_key.argtypes = [C.c_char_p, u64, C.c_char_p, u32, vp, u64, C.POINTER(u64)]
    L.bsh_hist_row.argtypes = [C.c_char_p, u64, C.c_char_p, u32, C.c_int64, u64, u32, C.POINTER(u32)]
    L.bsh_minmax_eval.argtypes = [vp, u32, C.c_int64, vp, u32, C.c_int64, C.c_int64]
    L.bsh_prefilter_eval.argtypes = [C.c_char_p, u64, C.c_char_p, u64, vp, vp, u32, vp]
    L.bsh_section_encode.argtypes = [C.POINTER(vp), pu64, pu64, pp, pu64]
    L.bsh_section_parse.argtypes = [C.c_char_p, u64, pu64, pu64, C.POINTER(vp)]
    L.bsh_crc32c.argtypes = [C.c_char_p, u64]; L.bsh_crc32c.restype = u32
    L.bse_open.argtypes = [C.c_char_p, u64, vp, pp]
    L.bse_close.argtypes = [vp]; L.bse_close.restype = None
    L.bse_last_error.argtypes = [vp]; L.bse_last_error.restype = C.c_char_p
    L.bse_stop.argtypes = [vp]
    L.bse_ingest_rows.argtypes = [vp, C.c_char_p, u64]
    L.bse_flush.argtypes = [vp]
    L.bse_merge.argtypes = [vp]
    L.bse_query.argtypes = [vp, C.c_char_p, u64, pp, pu64]
    L.bse_query_many.argtypes = [vp, C.c_char_p, u64, pp, pu64]
    L.bse_describe.argtypes = [vp, pp, pu64]
    L.bse_match_calls.argtypes = [vp, pp, pu64]
    L.bse_corrupt_section_byte.argtypes = [vp, u32, i32, u64]
    L.bse_section_bytes.argtypes = [vp, u32, i32, pp, pu64]
    for n in HOST_EXPORTS:
        f = getattr(L, n)
        if f.restype is C.c_int:
            f.restype = i32
    _H = L
    return L


def _take(L, p, n):
    data = C.string_at(p, n.value)
    L.bsh_free(p)
    return data


def tokenize(text: bytes | str, tokenizer=None, as_bytes: bool = False) -> list:
    """The tokens of `text`.  tokenizer: None = BasicWhitespaceLowerTokenizer through bsh_tokenize; a
    tokenizer.Tokenizer (or its C form) goes through bsh_tokenize_with.  as_bytes: the tokens' exact bytes (a token of a
    spec without lowering may keep an invalid UTF-8 byte) instead of str."""
    L = lib()
    b = text.encode("utf-8", "surrogatepass") if isinstance(text, str) else text
    p, n = C.c_void_p(), C.c_uint64()
    if tokenizer is not None or as_bytes:
        rc = L.bsh_tokenize_with(b, len(b), c_spec(tokenizer), C.byref(p), C.byref(n))
        if rc:
            raise HostError(rc, "invalid tokenizer spec")
        raw = _take(L, p, n)
        out, i = [], 0
        while i < len(raw):
            ln = int.from_bytes(raw[i: i + 4], "little")
            out.append(raw[i + 4: i + 4 + ln])
            i += 4 + ln
        return out if as_bytes else [t.decode("utf-8", "replace") for t in out]
    rc = L.bsh_tokenize(b, len(b), C.byref(p), C.byref(n))
    if rc:
        raise HostError(rc)
    raw = _take(L, p, n)
    return [t.decode("utf-8", "replace") for t in raw.split(b"\n")] if raw else []


class EntrySets:
    """bloomEntrySets (ingest.go:24-123)."""

    def __init__(self):
        self.L = lib()
        self.h = C.c_void_p(self.L.bsh_entry_sets_new())

    def __del__(self):
        if getattr(self, "h", None):
            self.L.bsh_entry_sets_free(self.h)
            self.h = None

    def index_row(self, row: bytes, tokenizer=None):
        """indexRow; tokenizer: None = the default, or a tokenizer.Tokenizer of the separator family."""
        if tokenizer is None:
            rc = self.L.bsh_entry_sets_index_row(self.h, row, len(row))
        else:
            rc = self.L.bsh_entry_sets_index_row_with(self.h, row, len(row), c_spec(tokenizer))
        if rc:
            raise HostError(rc, "row is not valid JSON (or the tokenizer spec is invalid)")

    def union_into(self, dst: "EntrySets"):
        self.L.bsh_entry_sets_union_into(self.h, dst.h)

    def counts(self):
        c = (C.c_uint64 * 3)()
        self.L.bsh_entry_sets_counts(self.h, c)
        return tuple(int(x) for x in c)

    def export(self, kind: int):
        """-> (u8 blob, u32 lengths) in the layout arena.plan_blocks takes."""
        n, nb = C.c_uint64(), C.c_uint64()
        self.L.bsh_entry_sets_export_sizes(self.h, kind, C.byref(n), C.byref(nb))
        blob = np.zeros(nb.value, dtype=np.uint8)
        off = np.zeros(n.value + 1, dtype=np.uint32)
        self.L.bsh_entry_sets_export(self.h, kind, _lib._ptr(blob) or 0, off.ctypes.data)
        return blob, np.diff(off).astype(np.uint32)

    def as_python_sets(self):
        out = []
        for kind in range(3):
            blob, ln = self.export(kind)
            off = np.concatenate([[0], np.cumsum(ln, dtype=np.int64)]).astype(np.int64)
            raw = blob.tobytes()
            out.append({raw[off[i]: off[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(ln))})
        return tuple(out)


class HostBatch:
    """QueryBatch: expression trees (reference JSON shape) lowered to C-ABI terms + programs."""

    def __init__(self, expressions=()):
        self.L = lib()
        self.h = C.c_void_p(self.L.bsh_batch_new())
        for e in expressions:
            self.add_query(e)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.bsh_batch_free(self.h)
            self.h = None

    def add_query(self, expression):
        s = json.dumps(expression).encode()
        rc = self.L.bsh_batch_add_query(self.h, s, len(s))
        if rc:
            raise HostError(rc, "bad expression JSON")

    def export(self):
        nq, nt, no, tb = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self.L.bsh_batch_sizes(self.h, C.byref(nq), C.byref(nt), C.byref(no), C.byref(tb))
        blob = np.zeros(max(tb.value, 1), dtype=np.uint8)
        toff = np.zeros(nt.value + 1, dtype=np.uint32)
        kinds = np.zeros(max(nt.value, 1), dtype=np.uint32)
        ops = np.zeros(max(no.value, 1), dtype=np.uint32)
        poff = np.zeros(nq.value + 1, dtype=np.uint32)
        self.L.bsh_batch_export(self.h, blob.ctypes.data, toff.ctypes.data, kinds.ctypes.data, ops.ctypes.data, poff.ctypes.data)
        raw = blob.tobytes()
        strings = [raw[toff[i]: toff[i + 1]] for i in range(nt.value)]
        return strings, kinds[: nt.value], ops[: no.value], poff


def match_row(expression, row: bytes, tokenizer=None) -> bool:
    """The host RowMatcher; tokenizer: None = the default (bsh_match_row), a tokenizer.Tokenizer = bsh_match_row_with."""
    L = lib()
    s = json.dumps(expression).encode()
    if tokenizer is None:
        rc = L.bsh_match_row(s, len(s), row, len(row))
    else:
        rc = L.bsh_match_row_with(s, len(s), row, len(row), c_spec(tokenizer))
    if rc < 0:
        raise HostError(rc)
    return bool(rc)


def prune_query(bloom_expression, regex_expression):
    """pruneBloomQuery of the host mirror -> expression dict or None."""
    L = lib()
    b = json.dumps(bloom_expression).encode()
    r = json.dumps(regex_expression).encode()
    p, n = C.c_void_p(), C.c_uint64()
    rc = L.bsh_prune_query(b, len(b), r, len(r), C.byref(p), C.byref(n))
    if rc:
        raise HostError(rc)
    return json.loads(_take(L, p, n))


def match_row_regex(regex_expression, row: bytes) -> bool:
    L = lib()
    r = json.dumps(regex_expression).encode()
    rc = L.bsh_match_row_regex(r, len(r), row, len(row))
    if rc < 0:
        raise HostError(rc)
    return bool(rc)


def substring_terms(needle: bytes | str, tokenizer=None, as_bytes: bool = False) -> list:
    """bsh_substring_terms: the pruning terms of one needle under `tokenizer` (None = the default)."""
    L = lib()
    b = needle.encode("utf-8", "surrogatepass") if isinstance(needle, str) else needle
    p, n = C.c_void_p(), C.c_uint64()
    rc = L.bsh_substring_terms(b, len(b), c_spec(tokenizer), C.byref(p), C.byref(n))
    if rc:
        raise HostError(rc, "needle: non-empty valid UTF-8 of at most 64 bytes after folding")
    raw, out, i = _take(L, p, n), [], 0
    while i < len(raw):
        ln = int.from_bytes(raw[i: i + 4], "little")
        out.append(raw[i + 4: i + 4 + ln])
        i += 4 + ln
    return out if as_bytes else [t.decode("utf-8", "replace") for t in out]


def prune_query_sub(bloom_expression, regex_expression, substring_expression, tokenizer=None):
    """bsh_prune_query_sub: And(bloom, regex field guard, substring guard) -> expression dict or None."""
    L = lib()
    b, r, s = (json.dumps(e).encode() for e in (bloom_expression, regex_expression, substring_expression))
    p, n = C.c_void_p(), C.c_uint64()
    rc = L.bsh_prune_query_sub(b, len(b), r, len(r), s, len(s), c_spec(tokenizer), C.byref(p), C.byref(n))
    if rc:
        raise HostError(rc)
    return json.loads(_take(L, p, n))


def match_row_substring(substring_expression, row: bytes, tokenizer=None) -> bool:
    """bsh_match_row_substring: the exact substring test of one row."""
    L = lib()
    s = json.dumps(substring_expression).encode()
    rc = L.bsh_match_row_substring(s, len(s), row, len(row), c_spec(tokenizer))
    if rc < 0:
        raise HostError(rc)
    return bool(rc)


def match_row_range(range_expression, row: bytes) -> bool:
    """bsh_match_row_range: the exact range test of one row (every JSON number literal, exponents included)."""
    L = lib()
    s = json.dumps(range_expression).encode()
    rc = L.bsh_match_row_range(s, len(s), row, len(row))
    if rc < 0:
        raise HostError(rc)
    return bool(rc)


def prune_query_range(bloom_expression, regex_expression, substring_expression, range_expression, tokenizer=None):
    """bsh_prune_query_range: And(bloom, regex field guard, substring guard, range guard) -> expression dict or None."""
    L = lib()
    b, r, s, g = (json.dumps(e).encode() for e in (bloom_expression, regex_expression, substring_expression, range_expression))
    p, n = C.c_void_p(), C.c_uint64()
    rc = L.bsh_prune_query_range(b, len(b), r, len(r), s, len(s), g, len(g), c_spec(tokenizer), C.byref(p), C.byref(n))
    if rc:
        raise HostError(rc)
    return json.loads(_take(L, p, n))


MM_EQ, MM_NE, MM_GT, MM_GE, MM_LT, MM_LE, MM_IN, MM_NOT_IN, MM_BETWEEN, MM_NOT_BETWEEN = range(10)       # bloomsearch_host.h BSH_MM_*
MM_OPS = {"EQ": MM_EQ, "NE": MM_NE, "GT": MM_GT, "GTE": MM_GE, "LT": MM_LT, "LTE": MM_LE, "IN": MM_IN, "NOT_IN": MM_NOT_IN,
          "BETWEEN": MM_BETWEEN, "NOT_BETWEEN": MM_NOT_BETWEEN}


def _pack_names(names):
    names = [f.encode() if isinstance(f, str) else bytes(f) for f in names]
    off = np.zeros(len(names) + 1, dtype=np.uint32)
    if names:
        off[1:] = np.cumsum([len(f) for f in names])
    blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8).copy()
    return blob, off


def minmax_row(row: bytes, fields, index=None) -> np.ndarray:
    """bsh_minmax_row: one row's contributions folded into `index` (an array of _lib.MINMAX_DTYPE, one record per field; None =
    all absent), in place; returns it.  Exact for every number literal.  HostError for a row that is not one valid JSON object."""
    L = lib()
    blob, off = _pack_names(fields)
    if index is None:
        index = np.zeros(len(off) - 1, dtype=_lib.MINMAX_DTYPE)
    assert index.dtype == _lib.MINMAX_DTYPE and len(index) == len(off) - 1 and index.flags.c_contiguous
    rc = L.bsh_minmax_row(row, len(row), blob.ctypes.data, off.ctypes.data, len(off) - 1, index.ctypes.data)
    if rc:
        raise HostError(rc)
    return index


def hist_row(row: bytes, field, origin: int, width: int, n_buckets: int) -> int:
    """bsh_hist_row: the row's slot among n_buckets + 3 (a bucket, then below, above, missing) by the rule of
    bsg_match_rows_wide_hist; exact for every literal.  HostError for a row that is not one valid JSON object or invalid arguments."""
    L = lib()
    field = field.encode() if isinstance(field, str) else bytes(field)
    slot = C.c_uint32()
    rc = L.bsh_hist_row(row, len(row), field, len(field), int(origin), int(width), int(n_buckets), C.byref(slot))
    if rc:
        raise HostError(rc)
    return int(slot.value)


def partition_key(row: bytes, name) -> bytes:
    """bsh_partition_key: the row's partition text under the field `name` (the keyed ingest's rule, exact for every row: escapes
    decoded).  HostError for a row that is not one valid JSON object, or a name of 0 or more than 64 bytes."""
    L = lib()
    name = name.encode() if isinstance(name, str) else bytes(name)
    out = np.zeros(max(len(row), 1), dtype=np.uint8)
    n = C.c_uint64()
    rc = L.bsh_partition_key(row, len(row), name, len(name), out.ctypes.data, len(out), C.byref(n))
    if rc:
        raise HostError(rc)
    return out[: n.value].tobytes()


def minmax_eval(imin: int, imax: int, op, value: int = 0, values=(), lo: int = 0, hi: int = 0) -> bool:
    """bsh_minmax_eval: EvaluateMinMaxCondition on the index (imin, imax).  op: MM_* or the reference's operator name."""
    L = lib()
    rec = np.zeros(1, dtype=_lib.MINMAX_DTYPE)
    rec[0] = (imin, imax, 1, 0)
    vs = np.ascontiguousarray(list(values), dtype=np.int64)
    rc = L.bsh_minmax_eval(rec.ctypes.data, MM_OPS.get(op, op), value, vs.ctypes.data if len(vs) else None, len(vs), lo, hi)
    if rc < 0:
        raise HostError(rc)
    return bool(rc)


def prefilter_eval(expression, partition_id: bytes | str = b"", indexes=None) -> bool:
    """bsh_prefilter_eval: evaluatePrefilterExpression for one block.  indexes: {field name: (min, max)} the block carries."""
    L = lib()
    s = json.dumps(expression).encode()
    pid = partition_id.encode() if isinstance(partition_id, str) else bytes(partition_id)
    names = list(indexes or {})
    blob, off = _pack_names(names)
    rec = np.zeros(max(len(names), 1), dtype=_lib.MINMAX_DTYPE)
    for i, f in enumerate(names):
        rec[i] = (indexes[f][0], indexes[f][1], 1, 0)
    rc = L.bsh_prefilter_eval(s, len(s), pid, len(pid), blob.ctypes.data, off.ctypes.data, len(names), rec.ctypes.data)
    if rc < 0:
        raise HostError(rc)
    return bool(rc)


def crc32c(data: bytes) -> int:
    return int(lib().bsh_crc32c(data, len(data)))


def section_encode(filters) -> bytes:
    """filters: 3 x (m, k, words ndarray) or None."""
    L = lib()
    words = (C.c_void_p * 3)(*[f[2].ctypes.data if f is not None else None for f in filters])
    m = (C.c_uint64 * 3)(*[f[0] if f is not None else 0 for f in filters])
    k = (C.c_uint64 * 3)(*[f[1] if f is not None else 0 for f in filters])
    p, n = C.c_void_p(), C.c_uint64()
    rc = L.bsh_section_encode(words, m, k, C.byref(p), C.byref(n))
    if rc:
        raise HostError(rc)
    return _take(L, p, n)


def section_parse(section: bytes):
    L = lib()
    m, k = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    w = (C.c_void_p * 3)()
    rc = L.bsh_section_parse(section, len(section), m, k, w)
    if rc:
        raise HostError(rc, "parseFilterSection failed")
    out = []
    for c in range(3):
        if not w[c]:
            out.append(None)
            continue
        nw = (m[c] + 63) // 64
        arr = np.frombuffer(C.string_at(w[c], nw * 8), dtype=np.uint64).copy()
        L.bsh_free(w[c])
        out.append((int(m[c]), int(k[c]), arr))
    return out


class Engine:
    """BloomSearchEngine mirror (IngestRows / Flush / Query / Merge) over a gpu.Context."""

    def __init__(self, ctx, **config):
        self.L = lib()
        self.ctx = ctx
        if hasattr(config.get("Tokenizer"), "to_json"):
            config["Tokenizer"] = config["Tokenizer"].to_json()
        cfg = json.dumps(config).encode()
        h = C.c_void_p()
        rc = self.L.bse_open(cfg, len(cfg), ctx.h, C.byref(h))
        if rc:
            raise HostError(rc, "ErrInvalidConfig" if rc == -101 else "")
        self.h = h
        ctx._dependents.add(self)            # an engine that outlives its context (a traceback keeps it) must not call into freed memory

    def close(self):
        if getattr(self, "h", None):
            self.L.bse_close(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc:
            raise HostError(rc, self.L.bse_last_error(self.h).decode())

    def ingest_rows(self, rows):
        """rows: iterable of marshaled-JSON bytes (one object each)."""
        blob = b"\n".join(rows)
        self._check(self.L.bse_ingest_rows(self.h, blob, len(blob)))

    def flush(self):
        self._check(self.L.bse_flush(self.h))

    def merge(self):
        self._check(self.L.bse_merge(self.h))

    def stop(self):
        self._check(self.L.bse_stop(self.h))

    def query(self, bloom_expression=None, regex_expression=None, substring_expression=None, range_expression=None, prefilter=None, histogram=None):
        """prefilter: a tree of query.Partition / MinMax / PrefilterAnd / PrefilterOr over the blocks' partition ids and MinMax indexes
        (config MinMaxIndexes=[...]); None takes exactly the path without one.
        histogram: {"Field", "Origin", "Width", "Buckets"}: the result then holds "rows": [] and "Histogram": {"Counts", "Below", "Above",
        "Missing"} over the matching rows (the bucket rule of bsg_match_rows_wide_hist); its stats are the query's without it."""
        d = {"Bloom": {"Expression": bloom_expression} if bloom_expression is not None else None,
             "Regex": {"Expression": regex_expression} if regex_expression is not None else None}
        if prefilter is not None:
            d["Prefilter"] = {"Expression": prefilter}
        if substring_expression is not None:
            d["Substring"] = substring_expression
        if range_expression is not None:
            d["Range"] = range_expression
        if histogram is not None:
            d["Histogram"] = histogram
        q = json.dumps(d).encode()
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bse_query(self.h, q, len(q), C.byref(p), C.byref(n)))
        return json.loads(_take(self.L, p, n))

    def query_many(self, bloom_expressions, regex_expressions=None, substring_expressions=None, range_expressions=None, prefilters=None, histograms=None):
        """bse_query_many: one pass for a batch of queries -> list of query()'s results, element i for bloom_expressions[i]
        (and regex_expressions[i] / substring_expressions[i] / range_expressions[i] / histograms[i], where given)."""
        rx = list(regex_expressions) if regex_expressions is not None else [None] * len(bloom_expressions)
        sx = list(substring_expressions) if substring_expressions is not None else [None] * len(bloom_expressions)
        gx = list(range_expressions) if range_expressions is not None else [None] * len(bloom_expressions)
        px = list(prefilters) if prefilters is not None else [None] * len(bloom_expressions)
        hx = list(histograms) if histograms is not None else [None] * len(bloom_expressions)
        q = json.dumps([dict({"Bloom": {"Expression": b} if b is not None else None, "Regex": {"Expression": r} if r is not None else None},
                             **({"Substring": s} if s is not None else {}), **({"Range": g} if g is not None else {}),
                             **({"Prefilter": {"Expression": p}} if p is not None else {}), **({"Histogram": h} if h is not None else {}))
                        for b, r, s, g, p, h in zip(bloom_expressions, rx, sx, gx, px, hx)]).encode()
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bse_query_many(self.h, q, len(q), C.byref(p), C.byref(n)))
        return json.loads(_take(self.L, p, n))

    def describe(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bse_describe(self.h, C.byref(p), C.byref(n)))
        return json.loads(_take(self.L, p, n))

    def match_calls(self) -> dict:
        """bse_match_calls: device row-matcher entry point -> how often the engine has called it (the route its queries took)."""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bse_match_calls(self.h, C.byref(p), C.byref(n)))
        return json.loads(_take(self.L, p, n))

    def corrupt_section_byte(self, file_index: int, block_index: int, byte_index: int):
        self._check(self.L.bse_corrupt_section_byte(self.h, file_index, block_index, byte_index))

    def section_bytes(self, file_index: int, block_index: int = -1) -> bytes:
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.bse_section_bytes(self.h, file_index, block_index, C.byref(p), C.byref(n)))
        return _take(self.L, p, n)


def regex_match(pattern: str | bytes, text: str | bytes) -> int:
    """Go regexp MatchString for the device regex subset on the DFA tables: 1 / 0, or _lib.BSG_E_UNSUPPORTED."""
    L = lib()
    p = pattern.encode("utf-8", "surrogatepass") if isinstance(pattern, str) else pattern
    t = text.encode("utf-8", "surrogatepass") if isinstance(text, str) else text
    return int(L.bsh_regex_match(p, len(p), t, len(t)))
