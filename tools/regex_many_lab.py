"""bsg_match_rows_many_regex against Q bsg_match_rows_regex calls: synth log rows in page-locked memory, Q in {1, 4, 16, 64} queries
of the reference's QueryRegex shape (a FieldToken bloom side AND a FieldRegex, tools/regex_lab.py) in three shapes:
  (i)   distinct fields: the regex conditions spread over eight fields, two patterns each (16 distinct conditions at Q >= 16,
        further queries pair them with other bloom sides), so the whole batch is ONE call;
  (ii)  the same field (message) with Q distinct patterns: the engine's rule (host/regex_groups.hpp co_active_bound <= slots) cuts
        the batch into groups of `slots` queries, one call each; the number of groups is printed beside the time;
  (iii) mixed: every second query is a plain three-term And of the bench's shape, the others of shape (i).
Per shape and Q: wall time and device time (bsg_last_match_ms, summed over the calls) of the batched call(s) and of the Q single
calls, medians over R runs with the run-to-run spread (min .. max), measured in one process on one device.

    python tools/regex_many_lab.py [n_rows] [repeats] [--slots N] [--lib PATH]

--slots N: the slot count the library under --lib was built with, for the 4-against-8 comparison: the grouping rule follows it.
The two runs of that comparison, on one box in one session, each GPU step under its own time limit and chained:

    BSG_EXTRA_CXXFLAGS=-DBSG_RX_MANY_SLOTS=8 python -m bloomsearch_amd.build --force
    mkdir -p tools/lab && cp bloomsearch_amd/csrc/libbloomgpu.so tools/lab/libbloomgpu_slots8.so
    python -m bloomsearch_amd.build --force
    timeout -k 10 400 python tools/regex_many_lab.py 1000000 5 > profiles/regex_many_lab.txt &&
    timeout -k 10 400 python tools/regex_many_lab.py 1000000 5 --slots 8 --lib tools/lab/libbloomgpu_slots8.so >> profiles/regex_many_lab.txt
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import _lib  # noqa: E402

args = [a for a in sys.argv[1:]]
slots = 4
for flag in ("--lib", "--slots"):
    if flag in args:
        i = args.index(flag)
        if flag == "--lib":
            _lib.LIB_PATH = os.path.abspath(args[i + 1])
        else:
            slots = int(args[i + 1])
        del args[i: i + 2]
from bloomsearch_amd import query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402

n_rows = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 5
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
print("library %s, %d slots\nrows %d, %.1f MB of row bytes in page-locked memory, %d runs per figure: median (min .. max)"
      % (_lib.LIB_PATH, slots, n_rows, n_bytes / 1e6, reps))

FIELD_PATTERNS = [("message", "timeout|cache"), ("service", "^pay"), ("level", "^err"), ("nested.region", "region-[37]$"), ("tags", "^(cache|miss)$"),
                  ("nested.az", "az-[01]$"), ("user_id", "^[0-9]{5}$"), ("timestamp", "7$"),
                  ("message", "upstream .*latency"), ("service", "(?i)AUTH"), ("level", "^(warn|info)$"), ("nested.region", "-0$"), ("tags", "shard"),
                  ("nested.az", "^az-2$"), ("user_id", "^1"), ("timestamp", "^17000[0-9]+$")]
MESSAGE_PATTERNS = ["%s .*%s" % (a, b) for a in synth.WORDS[:8] for b in synth.WORDS[5:13]]
d = synth.draws(0, 64)


def bloom_side(q):
    return Q.FieldToken("level", synth.LEVELS[d["level"][q]])


def plain(q):
    return Q.And(Q.FieldToken("level", synth.LEVELS[d["level"][q]]), Q.FieldToken("service", synth.SERVICES[d["service"][q]]),
                 Q.FieldToken("nested.region", "region-%d" % int(d["region"][q])))


def shape(name, nq):
    if name == "i":
        return [(bloom_side(q), Q.FieldRegex(*FIELD_PATTERNS[q % 16])) for q in range(nq)]
    if name == "ii":
        return [(bloom_side(q), Q.FieldRegex("message", MESSAGE_PATTERNS[q])) for q in range(nq)]
    return [(plain(q), None) if q % 2 else (bloom_side(q), Q.FieldRegex(*FIELD_PATTERNS[(q // 2) % 16])) for q in range(nq)]


def covers(a, path):
    return a != "" and (path == a or path.startswith(a + "."))


def groups_of(pairs):
    """the engine's rule (engine.hpp match_rows_device_many): a group closes at 64 queries / 64 conditions / 16 regex conditions, or
    when one leaf could lie under more regex conditions than a lane holds"""
    out, cur = [], []
    for p in pairs:
        try:
            b = Q.CompiledRowQueryBatch(cur + [p])
            fields = [f.decode() for k, f in zip(b.kinds, b.fields) if k == _lib.KIND_FIELD_REGEX]
            ok = max((sum(covers(a, f) for a in fields) for f in fields), default=0) <= slots
        except ValueError:
            ok = False
        if not ok and cur:
            out.append(cur)
            cur = []
        cur.append(p)
    return out + ([cur] if cur else [])


def fmt(v):
    return "%9.2f (%8.2f .. %8.2f)" % (float(np.median(v)), min(v), max(v))


with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    del rows
    ctx.match_rows_regex((blob, off), Q.CompiledRowQuery(*shape("i", 1)[0]))        # warm: module load, scratch, lower table
    for name in ("i", "ii", "iii"):
        for nq in (1, 4, 16, 64):
            pairs = shape(name, nq)
            matchers = [Q.CompiledRowQuery(b, r) for b, r in pairs]
            s_dev, s_wall, hits = [], [], []
            for _ in range(reps):
                dev, t0 = 0.0, time.perf_counter()
                for m in matchers:
                    h, fb = ctx.match_rows_regex((blob, off), m)
                    dev += ctx.last_match_ms()
                s_wall.append((time.perf_counter() - t0) * 1e3)
                s_dev.append(dev)
            batches = [Q.CompiledRowQueryBatch(g) for g in groups_of(pairs)]
            last = None
            m_dev, m_wall = [], []
            for _ in range(reps + 1):                                               # the first run warms the batched kernels and is dropped
                dev, n_fb, t0 = 0.0, 0, time.perf_counter()
                for b in batches:
                    last, fb = ctx.match_rows_many_regex((blob, off), b)
                    dev += ctx.last_match_ms()
                    n_fb += len(fb)
                m_wall.append((time.perf_counter() - t0) * 1e3)
                m_dev.append(dev)
            m_dev, m_wall = m_dev[1:], m_wall[1:]
            assert n_fb == 0 and np.array_equal(last[-1], h)                         # the last query's plane is its single call's bits
            print("(%s) Q=%2d  %2d x bsg_match_rows_regex        device ms %s   wall ms %s" % (name, nq, nq, fmt(s_dev), fmt(s_wall)))
            print("(%s) Q=%2d  %2d x bsg_match_rows_many_regex   device ms %s   wall ms %s   %d group(s), %d regex conditions"
                  % (name, nq, len(batches), fmt(m_dev), fmt(m_wall), len(batches), sum(b.kinds.count(_lib.KIND_FIELD_REGEX) for b in batches)))
            print("(%s) Q=%2d  batched / singles: device %.3f, wall %.3f; %.1f M rows/s per batched walk"
                  % (name, nq, np.median(m_dev) / np.median(s_dev), np.median(m_wall) / np.median(s_wall), n_rows * len(batches) / np.median(m_dev) / 1e3))
    ctx.pinned_free(blob)
