"""What the MinMax scanner of a device ingest costs (k_minmax_rows, csrc/minmax.hip.h), on synth log rows over 16 sets, default tokenizer:

  (a)  bsg_last_minmax_ms of bsg_ingest_rows_minmax with 1, 2 and 8 fields: "timestamp", then "user_id", then six names no row has
  (b)  ms_walk (bsg_ingest_stats) of the same calls
  (c)  ms_walk of bsg_ingest_rows_tok without fields, in this library and - with --parent-lib - in the library built from the parent
       commit: the walkers did not change, so the two must agree within the spread of the rounds
  (d)  in the parent library, ms_walk untrusted minus ms_walk trusted: what the walker's validation pass over the same bytes costs.
       The scanner reads the same bytes once and does less per byte, so (a) with 2 fields should not exceed (d)

Every leg is one call on the same rows; the legs alternate inside one process, one untimed warm-up round first, R timed rounds; every
figure is the median of the rounds with its spread (min .. max).  Both bars are written down as MET or MISSED with the figures.  The
feature is opt-in and no routing rule is derived from this file.

    python tools/ingest_minmax_lab.py [n_rows] [rounds] [--parent-lib PATH/libbloomgpu.so] [--out profiles/ingest_minmax_lab.txt]
"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bloomsearch_amd import _lib, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
opts = {sys.argv[i]: sys.argv[i + 1] for i in range(1, len(sys.argv) - 1) if sys.argv[i].startswith("--")}
args = [a for a in args if a not in opts.values()]
N_SETS = 16
n_rows = int(args[0]) if args else 1_000_000
rounds = int(args[1]) if len(args) > 1 else 5
per_set = n_rows // N_SETS
n_rows = per_set * N_SETS
FIELDS = ["timestamp", "user_id"] + ["absent_field_%d" % i for i in range(6)]


class Lib:
    """the few calls this tool makes, bound on a library of its own (this commit's, or the parent commit's)"""

    def __init__(self, path):
        self.L = L = C.CDLL(path)
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
        L.bsg_open.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
        L.bsg_close.argtypes = [vp]
        L.bsg_last_error.argtypes = [vp]
        L.bsg_last_error.restype = C.c_char_p
        L.bsg_ingest_rows_tok.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, C.POINTER(u64)]
        L.bsg_ingest_fallback_rows.argtypes = [vp, u64, vp, u32, C.POINTER(u32)]
        L.bsg_ingest_stats_read.argtypes = [vp, u64, C.POINTER(_lib.IngestStats)]
        L.bsg_ingest_free.argtypes = [vp, u64]
        self.has_minmax = hasattr(L, "bsg_ingest_rows_minmax")
        if self.has_minmax:
            L.bsg_ingest_rows_minmax.argtypes = L.bsg_ingest_rows_tok.argtypes + [vp, vp, u32]
            L.bsg_last_minmax_ms.argtypes = [vp, C.POINTER(C.c_float)]
        self.h = vp()
        ids = (i32 * 1)(0)
        self.check(L.bsg_open(ids, 1, C.byref(self.h)))

    def check(self, rc):
        if rc:
            raise RuntimeError("libbloomgpu error %d: %s" % (rc, self.L.bsg_last_error(self.h).decode()))

    def ingest(self, blob, off, first, flags, n_fields=0):
        """one call -> (ms_walk, ms of the scanner or None, rows handed back)"""
        ing = C.c_uint64()
        a = [self.h, blob.ctypes.data, off.ctypes.data, len(off) - 1, first.ctypes.data, len(first) - 1, None, 0, None, flags, None, C.byref(ing)]
        mm = None
        if n_fields:
            names = [f.encode() for f in FIELDS[:n_fields]]
            fo = np.zeros(n_fields + 1, dtype=np.uint32)
            fo[1:] = np.cumsum([len(f) for f in names])
            fb = np.frombuffer(b"".join(names), dtype=np.uint8).copy()
            self.check(self.L.bsg_ingest_rows_minmax(*a, fb.ctypes.data, fo.ctypes.data, n_fields))
            v = C.c_float()
            self.check(self.L.bsg_last_minmax_ms(self.h, C.byref(v)))
            mm = float(v.value)
        else:
            self.check(self.L.bsg_ingest_rows_tok(*a))
        st, n = _lib.IngestStats(), C.c_uint32()
        self.check(self.L.bsg_ingest_stats_read(self.h, ing.value, C.byref(st)))
        self.check(self.L.bsg_ingest_fallback_rows(self.h, ing.value, None, 0, C.byref(n)))
        self.check(self.L.bsg_ingest_free(self.h, ing.value))
        return float(st.ms_walk), mm, int(n.value)


def med(xs):
    return "%8.3f ms  (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    rows = [r for s in range(N_SETS) for r in synth.rows_json(s * per_set, per_set)]
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
    first = (np.arange(N_SETS + 1, dtype=np.uint32) * per_set).astype(np.uint32)
    here = Lib(_lib.LIB_PATH)
    parent = Lib(opts["--parent-lib"]) if "--parent-lib" in opts else None
    T = _lib.INGEST_TRUSTED_JSON
    legs = {"a1": [], "a2": [], "a8": [], "b1": [], "b2": [], "b8": [], "c_here": [], "c_parent": [], "d_untrusted": [], "d_trusted": [], "d": []}
    for r in range(rounds + 1):
        out = {}
        for nf in (1, 2, 8):                                   # untrusted, as (c): the walk validates, the scanner scans
            walk, mm, nfb = here.ingest(blob, off, first, 0, nf)
            assert nfb == 0, nfb
            out["a%d" % nf], out["b%d" % nf] = mm, walk
        out["c_here"] = here.ingest(blob, off, first, 0)[0]
        if parent:
            out["c_parent"] = parent.ingest(blob, off, first, 0)[0]
            out["d_untrusted"] = out["c_parent"]
            out["d_trusted"] = parent.ingest(blob, off, first, T)[0]
            out["d"] = out["d_untrusted"] - out["d_trusted"]
        if r:                                                  # round 0 warms up
            for k, v in out.items():
                legs[k].append(v)
    lines = ["ingest_minmax_lab: %d synth rows (%d bytes) over %d sets, default tokenizer, %d rounds, medians (min .. max)" % (n_rows, len(blob), N_SETS, rounds), ""]
    for nf in (1, 2, 8):
        lines.append("(a) k_minmax_rows, %d field%s   %s" % (nf, " " if nf == 1 else "s", med(legs["a%d" % nf])))
    for nf in (1, 2, 8):
        lines.append("(b) ms_walk of that call, %d f.  %s" % (nf, med(legs["b%d" % nf])))
    lines.append("(c) ms_walk, no fields, here    %s" % med(legs["c_here"]))
    if parent:
        lines.append("(c) ms_walk, no fields, parent  %s" % med(legs["c_parent"]))
        lines.append("(d) parent: untrusted           %s" % med(legs["d_untrusted"]))
        lines.append("    parent: trusted             %s" % med(legs["d_trusted"]))
        lines.append("    validation = the difference %s" % med(legs["d"]))
        ch, cp = statistics.median(legs["c_here"]), statistics.median(legs["c_parent"])
        spread_c = max(max(legs["c_here"]) - min(legs["c_here"]), max(legs["c_parent"]) - min(legs["c_parent"]))
        lines += ["", "bar 1: (c) here equals (c) at the parent within the spread of the rounds: |%.3f - %.3f| = %.3f ms against a spread of %.3f ms: %s"
                  % (ch, cp, abs(ch - cp), spread_c, "MET" if abs(ch - cp) <= spread_c else "MISSED")]
        a2, d = statistics.median(legs["a2"]), statistics.median(legs["d"])
        spread_d = max(legs["d"]) - min(legs["d"])
        lines.append("bar 2: (a) with 2 fields <= (d) plus the spread (d) shows: %.3f ms against %.3f + %.3f ms: %s"
                     % (a2, d, spread_d, "MET" if a2 <= d + spread_d else "MISSED"))
    else:
        lines += ["", "no --parent-lib: (c) at the parent commit and (d) were not measured, neither bar is judged"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if "--out" in opts:
        with open(opts["--out"], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
