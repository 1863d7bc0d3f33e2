"""Device ingest glue (test / bench): rows -> bsg_ingest_* -> filters, with the host walker finishing
the rows the device walker hands back (include/bloomgpu.h "device ingest").

Mirrors the flush worker's per-partition loop (flush.go:179-254): one set per partition buffer,
one parent per file, (m, k) sized on the host from the exact distinct counts (buildFilters,
ingest.go:127-145: n' = max(count, 1)).
"""
from __future__ import annotations

import numpy as np

from . import host
from ._lib import DESC_DTYPE, MINMAX_DTYPE
from .gpu import Context, estimate_parameters


class IngestResult:
    def __init__(self, counts, status, desc, words, stats, fallback_rows, minmax=None):
        self.counts, self.status, self.desc, self.words, self.stats, self.fallback_rows = counts, status, desc, words, stats, fallback_rows
        self._minmax = minmax

    def minmax(self):
        """(min, max, present), each (n_sets, n_fields): the sets' MinMax indexes (device_ingest(..., minmax_fields=...)), the rows
        the device handed back folded in through host.minmax_row."""
        if self._minmax is None:
            raise ValueError("the ingest was made without minmax_fields")
        return self._minmax

    def filter_words(self, set_index: int, kind: int) -> np.ndarray:
        d = self.desc[set_index * 3 + kind]
        nw = (int(d["m"]) + 63) // 64
        return self.words[int(d["word_off"]): int(d["word_off"]) + nw]


def plan_desc(counts: np.ndarray, fpr: float):
    """counts [n, 3] -> (desc [n*3], n_words): right-sized geometry, filters on 16-byte boundaries."""
    desc = np.zeros(counts.shape[0] * 3, dtype=DESC_DTYPE)
    cursor = 0
    cache: dict = {}
    for i, n in enumerate(counts.reshape(-1)):
        key = max(int(n), 1)
        mk = cache.get(key)
        if mk is None:
            mk = cache[key] = estimate_parameters(key, fpr)
        desc[i]["word_off"], desc[i]["m"], desc[i]["k"] = cursor, mk[0], mk[1]
        cursor += ((mk[0] + 63) // 64 + 1) // 2 * 2
    return desc, max(cursor, 2)


def host_walk_entries(rows, row_ids, set_of_row, tokenizer=None):
    """The host walker (walker.hpp through bsh_entry_sets_*) over the fallback rows ->
    (entries, set_of_entry, kind_of_entry).  tokenizer: the spec the device walked with (None = the default)."""
    by_set: dict = {}
    for r in row_ids:
        by_set.setdefault(int(set_of_row[r]), []).append(rows[int(r)])
    entries, sets, kinds = [], [], []
    for s, rs in by_set.items():
        es = host.EntrySets()
        for row in rs:
            try:
                es.index_row(row, tokenizer)
            except host.HostError:
                pass  # malformed row: what the walker saw before the error stays (entry_sets.hpp)
        for kind in range(3):
            blob, ln = es.export(kind)
            off = np.concatenate([[0], np.cumsum(ln, dtype=np.int64)])
            raw = blob.tobytes()
            for i in range(len(ln)):
                entries.append(raw[off[i]: off[i + 1]])
                sets.append(s)
                kinds.append(kind)
    return entries, sets, kinds


def fold_minmax(index, rows, row_ids, set_of_row, fields):
    """The rows the device handed back, folded into (min, max, present) of ctx.ingest_minmax on the host (bsh_minmax_row).  A row
    the device had decided changes nothing: the values are exact and the fold is idempotent."""
    mn, mx, present = index
    for r in row_ids:
        s = int(set_of_row[int(r)])
        rec = np.zeros(len(fields), dtype=MINMAX_DTYPE)
        rec["min"], rec["max"], rec["present"] = mn[s], mx[s], present[s]
        try:
            host.minmax_row(rows[int(r)], fields, rec)
        except host.HostError:
            continue                          # not a JSON object: it contributes nothing
        mn[s], mx[s], present[s] = rec["min"], rec["max"], rec["present"] != 0
    return mn, mx, present


def device_ingest(ctx: Context, row_sets, fpr: float, parent_of_set=None, n_parents: int = 0, slots_hint=None,
                  keep: bool = False, flags: int = 0, tokenizer=None, minmax_fields=None) -> IngestResult:
    """row_sets: list (one per set) of lists of row bytes.  tokenizer: None = the default tokenizer (bsg_ingest_rows); a
    tokenizer.Tokenizer of the separator family = bsg_ingest_rows_tok, its fallback rows walked by the host with the same spec."""
    rows = [r for rs in row_sets for r in rs]
    first = np.zeros(len(row_sets) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([len(rs) for rs in row_sets])
    ing = ctx.ingest_rows(rows, first, parent_of_set, n_parents, slots_hint, flags, tokenizer=tokenizer, minmax_fields=minmax_fields)
    try:
        fb = ctx.ingest_fallback_rows(ing)
        set_of_row = np.repeat(np.arange(len(row_sets)), np.diff(first.astype(np.int64)))
        minmax = None
        if minmax_fields is not None:
            minmax = fold_minmax(ctx.ingest_minmax(ing, len(row_sets)), rows, fb, set_of_row, list(minmax_fields))
        if len(fb):
            entries, sets, kinds = host_walk_entries(rows, fb, set_of_row, tokenizer)
            if entries:
                ctx.ingest_add_entries(ing, entries, sets, kinds)
        n_total = len(row_sets) + n_parents
        counts, status = ctx.ingest_finish(ing, n_total)
        desc, n_words = plan_desc(counts, fpr)
        words = ctx.ingest_build(ing, desc, n_words)
        stats = ctx.ingest_stats(ing)
        return IngestResult(counts, status, desc, words, stats, fb, minmax)
    finally:
        if not keep:
            ctx.ingest_free(ing)


class IngestStream:
    """A streaming device ingest (bsg_ingest_open / bsg_ingest_add_sets / bsg_ingest_append_rows): batches of rows that belong
    to arbitrary sets are handed to the device as they arrive; finish / build see what bsg_ingest_rows would have left.  Lives
    on one device of the context.  Use as a context manager or call close()."""

    def __init__(self, ctx: Context, ingest_id: int, n_sets: int, n_parents: int, tokenizer=None, minmax_fields=None, partition_field=None):
        self.ctx, self.id, self.n_sets, self.n_parents, self.tokenizer = ctx, ingest_id, n_sets, n_parents, tokenizer
        self.partition_field = partition_field    # a keyed stream (bsg_ingest_open_keyed): append_keyed / add_keys / keys
        self.minmax_fields = None if minmax_fields is None else list(minmax_fields)
        self._handed_back = []                # (row, set) of the rows finish_fallback folded: their MinMax contributions, kept for minmax()

    @classmethod
    def open(cls, ctx: Context, n_sets: int = 0, parent_of_set=None, n_parents: int = 0, slots_hint=None, flags: int = 0,
             tokenizer=None, minmax_fields=None, partition_field=None) -> "IngestStream":
        """partition_field: a KEYED stream — no initial sets; parent_of_set is then the ONE parent index of every set the stream creates
        (None = no parent) and the rows go in through append_keyed."""
        if partition_field is not None:
            if n_sets or slots_hint is not None:
                raise ValueError("a keyed stream starts without sets")
            parent = 0xFFFFFFFF if parent_of_set is None else int(parent_of_set)
            return cls(ctx, ctx.ingest_open_keyed(partition_field, n_parents, parent, flags, tokenizer, minmax_fields), 0, n_parents, tokenizer,
                       minmax_fields, partition_field)
        return cls(ctx, ctx.ingest_open(n_sets, parent_of_set, n_parents, slots_hint, flags, tokenizer, minmax_fields=minmax_fields), n_sets, n_parents,
                   tokenizer, minmax_fields)

    def add_sets(self, parent_of_new_set, slots_hint=None) -> int:
        first = self.ctx.ingest_add_sets(self.id, parent_of_new_set, slots_hint)
        self.n_sets += len(parent_of_new_set)
        return first

    def append(self, rows, set_of_row, finish_fallback: bool = True) -> np.ndarray:
        """rows: list of row bytes (or, with finish_fallback=False, a (u8 blob, u64 offsets) pair), row r to set set_of_row[r].
        Returns the batch-local indices of the rows the device handed
        back; with finish_fallback they have been walked by the host walker and added already."""
        if finish_fallback and isinstance(rows, tuple):
            raise TypeError("IngestStream.append: a (blob, offsets) batch has no row list for the host walker; pass finish_fallback=False")
        fb = self.ctx.ingest_append_rows(self.id, rows, set_of_row)
        if finish_fallback and len(fb):
            entries, sets, kinds = host_walk_entries(rows, fb, set_of_row, self.tokenizer)
            if entries:
                self.ctx.ingest_add_entries(self.id, entries, sets, kinds)
            if self.minmax_fields is not None:
                self._handed_back += [(rows[int(r)], int(set_of_row[int(r)])) for r in fb]
        return fb

    def append_keyed(self, rows, finish_fallback: bool = True):
        """A keyed stream's batch (rows: list of row bytes): the device finds every row's set.  -> (set_of_row, handed-back rows).
        With finish_fallback the rows the partitioner did not decide (set _lib.SET_UNDECIDED) have been given their sets on the host
        (host.partition_key, add_keys) — set_of_row then holds them — and every handed-back row has been walked by the host walker."""
        from . import _lib, host
        sets, n_new, fb = self.ctx.ingest_append_rows_keyed(self.id, rows)
        self.n_sets += n_new
        if finish_fallback and len(fb):
            und = [int(r) for r in fb if sets[int(r)] == _lib.SET_UNDECIDED]
            if und:
                sets[und] = self.add_keys([host.partition_key(rows[r], self.partition_field) for r in und])
            entries, esets, kinds = host_walk_entries(rows, fb, sets, self.tokenizer)
            if entries:
                self.ctx.ingest_add_entries(self.id, entries, esets, kinds)
            if self.minmax_fields is not None:
                self._handed_back += [(rows[int(r)], int(sets[int(r)])) for r in fb]
        return sets, fb

    def add_keys(self, keys) -> np.ndarray:
        """partition texts found on the host -> their sets (bsg_ingest_add_sets_keyed)"""
        out = self.ctx.ingest_add_sets_keyed(self.id, keys)
        self.n_sets = len(self.ctx.ingest_keys(self.id)) if len(out) else self.n_sets
        return out

    def keys(self, first: int = 0) -> list:
        """the partition texts of sets [first, n_sets)"""
        return self.ctx.ingest_keys(self.id, first)

    def minmax(self):
        """(min, max, present), each (n_sets, n_fields), over every append so far; the rows append(finish_fallback=True) got back
        are folded in through host.minmax_row (those of finish_fallback=False appends are the caller's to fold: fold_minmax)."""
        if self.minmax_fields is None:
            raise ValueError("the stream was opened without minmax_fields")
        index = self.ctx.ingest_minmax(self.id, self.n_sets)
        rows = [r for r, _ in self._handed_back]
        return fold_minmax(index, rows, range(len(rows)), [s for _, s in self._handed_back], self.minmax_fields)

    def finish(self):
        """-> (counts u64 [n_sets + n_parents, 3], status u32 [n_sets + n_parents]): sets, then parents"""
        return self.ctx.ingest_finish(self.id, self.n_sets + self.n_parents)

    def build(self, desc, n_words: int) -> np.ndarray:
        return self.ctx.ingest_build(self.id, desc, n_words)

    def build_sections(self, desc, arenas: bool = False):
        return self.ctx.ingest_build_sections(self.id, desc, arenas)

    def stats(self):
        return self.ctx.ingest_stats(self.id)

    def close(self):
        if self.id:
            self.ctx.ingest_free(self.id)
            self.id = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
