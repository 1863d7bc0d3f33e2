"""A restatement of the MinMax index contract (include/bloomgpu.h "per-set MinMax indexes") in plain Python over fractions.Fraction,
for the tests of host/minmax.hpp, of the device scanner (csrc/minmax.hip.h) and of the engine: a field is a TOP-LEVEL key compared
with the decoded key, the last member with the key counts, its value must itself be a number, and the exact value v contributes
(clamp(floor(v)), clamp(ceil(v))).  No float is involved anywhere."""
import fractions
import math

from tests.range_restatement import BIG, I64_MAX, I64_MIN, LITERALS, Obj, exact, parse  # noqa: F401  (re-exported for the tests)

OPS = ["EQ", "NE", "GT", "GTE", "LT", "LTE", "IN", "NOT_IN", "BETWEEN", "NOT_BETWEEN"]


def clamp(v: int) -> int:
    return max(I64_MIN, min(I64_MAX, v))


def contribution_of(value: fractions.Fraction):
    return clamp(math.floor(value)), clamp(math.ceil(value))


def row_contributions(row: bytes, fields):
    """-> {field: (min, max)} for the fields the row contributes to.  ValueError when the row is not a JSON object."""
    node = parse(row)
    if not isinstance(node, Obj):
        raise ValueError("not an object")
    last = {}
    for k, v in node.pairs:                     # the last member with a key wins, whatever it holds
        last[k] = v
    out = {}
    for f in fields:
        v = last.get(f)
        if isinstance(v, fractions.Fraction):   # bool, str, None, list, Obj contribute nothing
            out[f] = contribution_of(v)
    return out


def fold(index, contribution):
    """UpdateMinMaxIndex; index None = absent"""
    if index is None:
        return contribution
    return min(index[0], contribution[0]), max(index[1], contribution[1])


def set_indexes(row_sets, fields):
    """row_sets: list of lists of rows -> per set a list (one per field) of (min, max) or None (absent).  Rows that are not valid
    JSON objects contribute nothing."""
    out = []
    for rows in row_sets:
        idx = [None] * len(fields)
        for row in rows:
            try:
                c = row_contributions(row, fields)
            except ValueError:
                continue
            for i, f in enumerate(fields):
                if f in c:
                    idx[i] = fold(idx[i], c[f])
        out.append(idx)
    return out


def evaluate(index, op: str, value: int = 0, values=(), lo: int = 0, hi: int = 0) -> bool:
    """EvaluateMinMaxCondition on a present index (min, max): might the block hold a matching value.  A bound at an int64 extreme is
    saturated: the true value may lie beyond it."""
    imin, imax = index
    above, below = imax == I64_MAX, imin == I64_MIN
    if op == "EQ":
        return imin <= value <= imax
    if op == "NE":
        return not (imin == value == imax) or above or below
    if op == "GT":
        return imax > value or above
    if op == "GTE":
        return imax >= value
    if op == "LT":
        return imin < value or below
    if op == "LTE":
        return imin <= value
    if op == "IN":
        return any(imin <= v <= imax for v in values)
    if op == "NOT_IN":
        return True
    if op == "BETWEEN":
        return imin <= hi and lo <= imax
    if op == "NOT_BETWEEN":
        return imin < lo or imax > hi or above or below
    return False


def string_evaluate(v: str, cond: dict) -> bool:
    op = cond.get("Operator")
    value, values, lo, hi = cond.get("Value") or "", cond.get("Values") or [], cond.get("Min") or "", cond.get("Max") or ""
    b = lambda s: s.encode()                    # Go compares strings byte-wise
    return {"EQ": v == value, "NE": v != value, "GT": b(v) > b(value), "GTE": b(v) >= b(value), "LT": b(v) < b(value), "LTE": b(v) <= b(value),
            "IN": v in values, "NOT_IN": v not in values, "BETWEEN": b(lo) <= b(v) <= b(hi), "NOT_BETWEEN": b(v) < b(lo) or b(v) > b(hi)}.get(op, False)


def prefilter_holds(tree, partition_id: str, indexes: dict) -> bool:
    """evaluatePrefilterExpression: indexes = {field: (min, max)} the block carries"""
    if tree is None:
        return True
    t = tree.get("ExpressionType")
    if t == "CONDITION":
        c = tree.get("Condition")
        if c is None:
            return True
        if c.get("ConditionType") == "PARTITION":
            pc = c.get("PartitionCondition")
            return True if pc is None else (partition_id != "" and string_evaluate(partition_id, pc))
        if c.get("ConditionType") == "MINMAX":
            mc = c.get("MinMaxCondition")
            if mc is None:
                return True
            idx = indexes.get(c.get("MinMaxFieldName") or "")
            return idx is not None and evaluate(idx, mc.get("Operator"), mc.get("Value") or 0, mc.get("Values") or [], mc.get("Min") or 0, mc.get("Max") or 0)
        return False
    kids = [prefilter_holds(c, partition_id, indexes) for c in tree.get("Children") or []]
    return all(kids) if t == "AND" else any(kids) if t == "OR" else False
