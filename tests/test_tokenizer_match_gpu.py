"""bsg_match_rows_tok (k_match_rows / k_match_rows_regex under a separator-family tokenizer spec): the device's bits, and the
rows it hands back decided by the host matcher under the same spec (bsh_match_row_with, bsh_match_row_regex), equal the Python
restatement's verdicts (tests/tokenizer_restatement.py) on every row, for Field / Token / FieldToken programs, with and without
FieldRegex conditions in the same program; the default-plus-0x01 spec equals bsg_match_rows bit for bit; invalid specs are
refused by both device entry points."""
import random

import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst, ingest as I, query as Q, synth
from bloomsearch_amd._lib import BloomGpuError
from bloomsearch_amd.gpu import Context
from tests import tokenizer_restatement as R
from tests.helpers import device_ids
from tests.test_host_tables import _random_value, go_marshal
from tests.test_tokenizer_ingest_gpu import EDGE_ROWS, FALLBACK_ROWS

pytestmark = pytest.mark.gpu

TOKENS = ["alice", "user", "user=alice", "get", "GET", "api", "v1", "users", "error", "timeout", "error:timeout", "1", "5e", "3",
          "-1.5e-3", "true", "tru", "false", "k", "kelvin", "i", "stanbul", "x", "y", "z", "quoted", "paren", "br", "v", "w", "q",
          "value", "key", "alpha", "beta", "gamma", "delta", "a", "b", "héllo", "日本語", "x::y"]
FIELDS = ["msg", "e", "n", "u", "w", "K", "arr", "arr.k", "deep.a.b.c", "user", "a.b", "user.name", "nothere", "s", "d"]
PATTERNS = ["alice", "^user", "[0-9]+", "time(out)?", "=", "^a", "e$", "[a-z]+=[a-z]+"]


def rows_for(seed):
    rng = np.random.default_rng(seed)
    rows = list(synth.rows_json(seed * 100, 150))
    for _ in range(250):
        rows.append(go_marshal({"msg": _random_value(rng, 0), "user": _random_value(rng, 1), "a.b": _random_value(rng, 2)}))
    rows += EDGE_ROWS * 3 + FALLBACK_ROWS
    random.Random(seed).shuffle(rows)
    return rows


def cond(r):
    t = r.choice(["FIELD", "TOKEN", "FIELD_TOKEN", "TOKEN"])
    c = {"Type": t}
    if t != "TOKEN":
        c["Field"] = r.choice(FIELDS)
    if t != "FIELD":
        c["Token"] = r.choice(TOKENS)
    return {"ExpressionType": "CONDITION", "Condition": c}


def expr(r, depth=0):
    if depth >= 2 or r.random() < 0.4:
        return cond(r)
    return {"ExpressionType": r.choice(["AND", "OR"]), "Children": [expr(r, depth + 1) for _ in range(r.randint(1, 3))]}


def regex_expr(r):
    leaf = lambda: {"ExpressionType": "CONDITION", "Condition": {"Field": r.choice(FIELDS[:6]), "Pattern": r.choice(PATTERNS)}}
    if r.random() < 0.5:
        return leaf()
    return {"ExpressionType": r.choice(["AND", "OR"]), "Children": [leaf(), leaf()]}


def run(ctx, rows, spec, bloom, regex=None):
    """-> (every row's verdict, the rows handed back): the device's bits, the handed-back rows decided by the host matcher
    under the same spec — bloom side bsh_match_row_with, regex side bsh_match_row_regex — as the engine mirror does"""
    if regex is None:
        got, fb = ctx.match_rows(rows, Q.CompiledMatcher(bloom), tokenizer=spec)
    else:
        got, fb = ctx.match_rows_regex(rows, Q.CompiledRowQuery(bloom, regex), tokenizer=spec)
    assert not got[fb].any()
    got = got.copy()
    for i in fb:
        row = rows[int(i)]
        got[i] = Hst.match_row(bloom, row, spec) and (regex is None or Hst.match_row_regex(regex, row))
    return got, fb


@pytest.mark.parametrize("name", sorted(R.SPECS))
def test_match_rows_tok_matches_the_restatement(ctx, name):
    spec = R.SPECS[name]
    r = random.Random(name)
    rows = rows_for(2)
    for _ in range(25):
        bloom = expr(r)
        want = np.array([R.row_verdict(x, spec, bloom) for x in rows])
        got, fb = run(ctx, rows, spec, bloom)
        assert set(fb.tolist()) >= {rows.index(x) for x in FALLBACK_ROWS}
        assert np.array_equal(got, want), (name, bloom, np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("name", sorted(R.SPECS))
def test_match_rows_tok_with_regex_conditions(ctx, name):
    spec = R.SPECS[name]
    r = random.Random("regex-" + name)
    rows = rows_for(3)
    for _ in range(12):
        bloom, regex = (expr(r) if r.random() < 0.8 else None), regex_expr(r)
        want = np.array([R.row_verdict(x, spec, bloom, regex) for x in rows])
        got, fb = run(ctx, rows, spec, bloom, regex)
        assert len(fb) >= len(FALLBACK_ROWS)
        assert np.array_equal(got, want), (name, bloom, regex, np.flatnonzero(got != want)[:5])


def test_token_alice_on_user_equals_alice(ctx):
    rows = [b'{"msg":"user=alice"}', b'{"msg":"GET /api/v1/users"}', b'{"msg":"error:timeout"}']
    alice = {"ExpressionType": "CONDITION", "Condition": {"Type": "TOKEN", "Token": "alice"}}
    users = {"ExpressionType": "CONDITION", "Condition": {"Type": "FIELD_TOKEN", "Field": "msg", "Token": "users"}}
    timeout = {"ExpressionType": "CONDITION", "Condition": {"Type": "TOKEN", "Token": "timeout"}}
    for q, want in ((alice, [1, 0, 0]), (users, [0, 1, 0]), (timeout, [0, 0, 1])):
        got, fb = ctx.match_rows(rows, Q.CompiledMatcher(q), tokenizer=R.SPECS["punct_lower"])
        assert got.tolist() == [bool(x) for x in want] and len(fb) == 0
        got, fb = ctx.match_rows(rows, Q.CompiledMatcher(q))
        assert not got.any() and len(fb) == 0


def test_default_plus_0x01_equals_match_rows(ctx):
    rows = [x for x in rows_for(4) if b"\\u0001" not in x]
    r = random.Random(77)
    for _ in range(20):
        bloom = expr(r)
        a = ctx.match_rows(rows, Q.CompiledMatcher(bloom), tokenizer=R.SPECS["default_plus_01"])
        b = ctx.match_rows(rows, Q.CompiledMatcher(bloom))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), bloom
        regex = regex_expr(r)
        a = ctx.match_rows_regex(rows, Q.CompiledRowQuery(bloom, regex), tokenizer=R.SPECS["default_plus_01"])
        b = ctx.match_rows_regex(rows, Q.CompiledRowQuery(bloom, regex))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (bloom, regex)


def test_match_rows_tok_on_two_devices():
    spec = R.SPECS["punct_raw"]
    rows = rows_for(5) * 4
    bloom = {"ExpressionType": "OR", "Children": [cond(random.Random(s)) for s in range(4)]}
    want = np.array([R.row_verdict(x, spec, bloom) for x in rows])
    with Context(device_ids(2)) as m:
        m.set_lab(8, 1)                                     # shard whatever the size
        m.set_ingest_chunk(1 << 16)
        got, fb = run(m, rows, spec, bloom)
    assert np.array_equal(got, want)


def test_device_entry_points_refuse_invalid_specs(ctx):
    """tok_spec: NUL as a separator, a non-zero reserved word, unknown flags -> BSG_E_INVALID before anything runs"""
    rows = [b'{"msg":"a,b"}']
    bloom = {"ExpressionType": "CONDITION", "Condition": {"Type": "TOKEN", "Token": "a"}}
    for sep0, flags, reserved in ((1 | (1 << 44), 0, 0), (1 << 44, 0, 7), (1 << 44, 4, 0), (1 << 44, 0x80000000, 0)):
        t = _lib.Tokenizer()
        t.sep_ascii[0], t.flags, t.reserved = sep0, flags, reserved
        with pytest.raises(BloomGpuError) as e:
            ctx.ingest_rows(rows, np.array([0, 1], dtype=np.uint32), tokenizer=t)
        assert e.value.code == _lib.BSG_E_INVALID
        with pytest.raises(BloomGpuError) as e:
            ctx.match_rows(rows, Q.CompiledMatcher(bloom), tokenizer=t)
        assert e.value.code == _lib.BSG_E_INVALID
    t = _lib.Tokenizer()
    t.sep_ascii[0] = 1 << 44                                            # ',' alone: valid, and the same call now runs
    got, fb = ctx.match_rows(rows, Q.CompiledMatcher(bloom), tokenizer=t)
    assert got.tolist() == [True] and len(fb) == 0
    res = I.device_ingest(ctx, [rows], 0.001, tokenizer=t)
    assert [int(x) for x in res.counts[0]] == [1, 2, 2]
