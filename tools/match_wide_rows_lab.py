"""One bsg_match_rows_wide_rows call against one bsg_match_rows_wide call PLUS the host's scan of its words to the same row lists:
synth log rows in page-locked memory in 100 sets, every query listed on every set, Q in {64, 256, 1024, 4096}.
  needle  And(level, service, nested.region, nested.az, tags) over the rows' own terms: about 3 matches per pair of a 10 000-row set
  broad   Or(level, service, nested.region): about half the rows (0.475); capped at --broad-max-q queries, the lists themselves
          (32 matches per word) outgrow the host beyond it
Both sides go through the C calls with preallocated outputs and end with the same thing in hand: per pair the ascending
set-relative indices of its matching rows, as one u32 array and per-pair counts.  The bit-row side gets there by scanning its words
(numpy: the non-zero words unpacked), the list side by taking LIST payloads as they are and unpacking DENSE payloads the same way.
The numpy scan stands in for the engine's word loop (host/engine.hpp): it is the same work, not the same code.
Alternating rounds in one session: A, B, A, B, ... reps times each.  Per figure: median (min .. max) of wall ms of the call, wall ms
of the host step, device ms (bsg_last_match_ms), and the bytes each call returns.

    python tools/match_wide_rows_lab.py [n_rows] [repeats] [max_q] [broad_max_q]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import _lib, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context, pack_entries  # noqa: E402

args = sys.argv[1:]
n_rows = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 5
max_q = int(args[2]) if len(args) > 2 else 4096
broad_max_q = int(args[3]) if len(args) > 3 else 256
N_SETS = 100
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
dq = synth.draws(0, max_q)
FT = Q.FieldToken
needle = [Q.And(FT("level", synth.LEVELS[dq["level"][i]]), FT("service", synth.SERVICES[dq["service"][i]]), FT("nested.region", "region-%d" % int(dq["region"][i])),
                FT("nested.az", "az-%d" % int(dq["az"][i])), FT("tags", synth.WORDS[dq["tags"][i][0]])) for i in range(max_q)]
broad = [Q.Or(FT("level", synth.LEVELS[dq["level"][i]]), FT("service", synth.SERVICES[dq["service"][i]]), FT("nested.region", "region-%d" % int(dq["region"][i])))
         for i in range(max_q)]
first = np.asarray([n_rows * s // N_SETS for s in range(N_SETS + 1)], dtype=np.uint32)
print("library %s\nrows %d in %d sets, %.1f MB of row bytes in page-locked memory, %d alternating rounds per figure: median (min .. max)"
      % (_lib.LIB_PATH, n_rows, N_SETS, n_bytes / 1e6, reps))


def fmt(v):
    return "%9.2f (%8.2f .. %8.2f)" % (float(np.median(v)), min(v), max(v))


def unpack(words, word_pair, word_tile):
    """the set bits of `words` (u64; word i is tile word_tile[i] of pair word_pair[i]) -> (set-relative indices, their pairs), in order"""
    idx, pair = [], []
    nz = np.flatnonzero(words)
    for c0 in range(0, len(nz), 1 << 20):
        sel = nz[c0: c0 + (1 << 20)]
        bits = np.unpackbits(words[sel].view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
        r, c = np.nonzero(bits)
        idx.append((word_tile[sel[r]].astype(np.uint32) << 6) + c.astype(np.uint32))
        pair.append(word_pair[sel[r]])
    if not idx:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    return np.concatenate(idx), np.concatenate(pair)


with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    del rows
    ctx.match_rows((blob, off), Q.CompiledMatcher(needle[0]))                      # warm: module load, scratch, lower table
    p = _lib._ptr
    for kind, exprs, q_cap in (("needle", needle, max_q), ("broad", broad, min(max_q, broad_max_q))):
        for nq in [q for q in (64, 256, 1024, 4096) if q <= q_cap]:
            batch = Q.CompiledWideBatch(exprs[:nq])
            cblob, coff = pack_entries([x for pair in zip(batch.fields, batch.tokens) for x in pair])
            kinds, ops, poff = (np.asarray(a, dtype=np.uint32) for a in (batch.kinds, batch.prog_ops, batch.prog_off))
            sqo = np.arange(N_SETS + 1, dtype=np.uint32) * np.uint32(nq)
            sq = np.tile(np.arange(nq, dtype=np.uint32), N_SETS)
            n_pairs = len(sq)
            pwo, total = ctx.match_wide_size(first, sqo, n_rows, nq)
            head = (ctx.h, p(blob), p(off), n_rows, p(cblob), p(coff), p(kinds), len(kinds), p(ops), poff.ctypes.data, nq, p(first), p(sqo), sq.ctypes.data,
                    N_SETS, None)
            words = np.zeros(total, dtype=np.uint64)
            hdr, pair_off, payload = np.zeros(n_pairs, dtype=np.uint32), np.zeros(n_pairs + 1, dtype=np.uint64), np.zeros(2 * total, dtype=np.uint32)
            fb, nfb, plen = np.zeros(n_rows, dtype=np.uint32), C.c_uint32(), C.c_uint64()
            tiles_of_pair = np.diff(pwo).astype(np.int64)
            word_pair = np.repeat(np.arange(n_pairs, dtype=np.uint32), tiles_of_pair)
            word_tile = (np.arange(total, dtype=np.int64) - np.repeat(pwo[:-1].astype(np.int64), tiles_of_pair)).astype(np.uint32)

            def run_bits():
                t0 = time.perf_counter()
                rc = ctx.L.bsg_match_rows_wide(*head, words.ctypes.data, p(fb), len(fb), C.byref(nfb))
                t1 = time.perf_counter()
                assert rc == 0 and nfb.value == 0, rc
                ms = ctx.last_match_ms()
                t2 = time.perf_counter()
                idx, pair = unpack(words, word_pair, word_tile)
                counts = np.bincount(pair, minlength=n_pairs)
                t3 = time.perf_counter()
                return (t1 - t0) * 1e3, (t3 - t2) * 1e3, ms, total * 8, idx, counts

            def run_rows():
                t0 = time.perf_counter()
                rc = ctx.L.bsg_match_rows_wide_rows(*head, hdr.ctypes.data, pair_off.ctypes.data, payload.ctypes.data, len(payload), C.byref(plen), p(fb),
                                                    len(fb), C.byref(nfb))
                t1 = time.perf_counter()
                assert rc == 0 and nfb.value == 0, rc
                ms = ctx.last_match_ms()
                t2 = time.perf_counter()
                tag = hdr >> 30
                counts = np.where(tag == 2, hdr & 0x3FFFFFFF, 0).astype(np.int64)
                set_rows = np.repeat(np.diff(first), nq).astype(np.int64)
                counts[tag == 1] = set_rows[tag == 1]
                if not (tag == 1).any() and not (tag == 3).any():
                    idx = payload[: plen.value]                                     # nothing but LISTs: the payload is the answer
                else:                                                              # DENSE pairs unpacked, ALL pairs counted up, in pair order
                    parts = {}
                    dense = np.flatnonzero(tag == 3)
                    if len(dense):
                        t_d = tiles_of_pair[dense]
                        src = np.repeat(pair_off[dense].astype(np.int64), 2 * t_d) + (np.arange(int(2 * t_d.sum())) - np.repeat(np.cumsum(2 * t_d) - 2 * t_d, 2 * t_d))
                        w = np.ascontiguousarray(payload[src]).view(np.uint64)
                        d_idx, d_pair = unpack(w, np.repeat(dense.astype(np.uint32), t_d), (np.arange(len(w)) - np.repeat(np.cumsum(t_d) - t_d, t_d)).astype(np.uint32))
                        counts[dense] = np.bincount(d_pair, minlength=n_pairs)[dense]
                        starts = np.concatenate([[0], np.cumsum(counts[dense])])
                        for k, pr in enumerate(dense):
                            parts[int(pr)] = d_idx[starts[k]: starts[k + 1]]
                    for pr in np.flatnonzero(tag == 2):
                        parts[int(pr)] = payload[int(pair_off[pr]): int(pair_off[pr + 1])]
                    for pr in np.flatnonzero(tag == 1):
                        parts[int(pr)] = np.arange(set_rows[pr], dtype=np.uint32)
                    idx = np.concatenate([parts[k] for k in sorted(parts)]) if parts else np.zeros(0, dtype=np.uint32)
                t3 = time.perf_counter()
                return (t1 - t0) * 1e3, (t3 - t2) * 1e3, ms, n_pairs * 4 + plen.value * 4, idx, counts

            a, b = run_bits(), run_rows()                                          # warm, and both sides end with the same lists
            assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
            tags = np.bincount(hdr >> 30, minlength=4)
            res = {"bits": [], "rows": []}
            for _ in range(reps):
                res["bits"].append(run_bits()[:4])
                res["rows"].append(run_rows()[:4])
            print("%s Q=%4d pairs %7d  conditions %d  matches per pair %.1f  tags NONE %d ALL %d LIST %d DENSE %d"
                  % (kind, nq, n_pairs, len(kinds), a[5].mean(), tags[0], tags[1], tags[2], tags[3]))
            for name, label in (("bits", "bsg_match_rows_wide + word scan"), ("rows", "bsg_match_rows_wide_rows       ")):
                call, host, dev, nbytes = zip(*res[name])
                print("   %s  call wall ms %s   host step ms %s   device ms %s   returned %9.2f MB"
                      % (label, fmt(call), fmt(host), fmt(dev), nbytes[0] / 1e6))
            tot = {k: np.median([r[0] + r[1] for r in v]) for k, v in res.items()}
            callw = {k: np.median([r[0] for r in v]) for k, v in res.items()}
            devm = {k: np.median([r[2] for r in v]) for k, v in res.items()}
            print("   rows / bits: call wall %.3f, call + host step %.3f, device %.3f" % (callw["rows"] / callw["bits"], tot["rows"] / tot["bits"], devm["rows"] / devm["bits"]))
            del words, payload, word_pair, word_tile
    ctx.pinned_free(blob)
