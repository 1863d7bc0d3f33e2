"""The keyed ingest's partition rule (include/bloomgpu.h "keyed streaming ingest"), restated over Python's json, independent of the
library: partition_text gives the text of EVERY valid row (object_pairs_hook keeps duplicate keys in order, so the FIRST member with
the key counts; parse_int / parse_float receive a number's raw literal, so it stays as written), device_decides restates which rows
the device decides and which it hands back, from the raw spans of the top-level members (json.decoder.scanstring / raw_decode)."""
import json
from json.decoder import scanstring

MAX_NAME, MAX_KEY = 64, 128           # BSG_PARTITION_MAX_NAME, BSG_PARTITION_MAX_KEY
WS = " \t\n\r"


class _Raw(str):
    """a number, as its literal"""


class _Obj(list):
    """an object, as its (key, value) pairs in order"""


def _constant(name):
    raise ValueError("not JSON: " + name)


def partition_text(row: bytes, name: str) -> bytes:
    """ValueError for a row that is not one JSON object"""
    top = json.loads(row.decode("utf-8"), object_pairs_hook=_Obj, parse_int=_Raw, parse_float=_Raw, parse_constant=_constant)
    if not isinstance(top, _Obj):
        raise ValueError("not an object")
    for k, v in top:
        if k != name:
            continue
        if isinstance(v, _Raw):
            return str(v).encode()
        if isinstance(v, str):
            return v.encode("utf-8")
        if v is True:
            return b"true"
        if v is False:
            return b"false"
        return b""                    # null, an object, an array
    return b""


def top_members(row: bytes):
    """[(raw key between its quotes, decoded key, raw value)] of the row's top-level members, in order"""
    s = row.decode("utf-8")
    dec = json.JSONDecoder()
    i = 0

    def ws(i):
        while i < len(s) and s[i] in WS:
            i += 1
        return i
    i = ws(i)
    if i >= len(s) or s[i] != "{":
        raise ValueError("not an object")
    i = ws(i + 1)
    out = []
    if s[i] == "}":
        return out
    while True:
        i = ws(i)
        if s[i] != '"':
            raise ValueError("key expected")
        key, end = scanstring(s, i + 1)
        raw_key = s[i + 1: end - 1]
        i = ws(end)
        if s[i] != ":":
            raise ValueError("colon expected")
        i = ws(i + 1)
        _, end = dec.raw_decode(s, i)
        out.append((raw_key, key, s[i:end]))
        i = ws(end)
        if s[i] == "}":
            return out
        if s[i] != ",":
            raise ValueError("comma expected")
        i += 1


def device_decides(row: bytes, name: str) -> bool:
    """False: the row is handed back — a top-level key with a backslash is met before the member is found (or the member is never
    found), the member's value is a string with a backslash, or the text is longer than MAX_KEY bytes"""
    for raw_key, key, raw_value in top_members(row):
        if "\\" in raw_key:
            return False
        if key != name:
            continue
        if raw_value[0] == '"':
            return "\\" not in raw_value and len(raw_value[1:-1].encode("utf-8")) <= MAX_KEY
        if raw_value[0] in "-0123456789":
            return len(raw_value) <= MAX_KEY
        return True
    return True


def assign_sets(batches, name, known=None, host_finish=False):
    """The numbering of a keyed ingest fed `batches` (lists of rows): per batch every row's set (None for a handed-back row) and the
    text of every set — new texts numbered by their first decided row.  known: texts registered before (their sets come first).
    host_finish: after each batch the caller registers the texts of its handed-back rows, in row order (bsg_ingest_add_sets_keyed);
    the rows then carry those sets."""
    keys = list(known or [])
    index = {k: i for i, k in enumerate(keys)}

    def set_of(t):
        if t not in index:
            index[t] = len(keys)
            keys.append(t)
        return index[t]
    out = []
    for rows in batches:
        decided = [device_decides(r, name) for r in rows]
        sets = [set_of(partition_text(r, name)) if d else None for r, d in zip(rows, decided)]
        if host_finish:
            sets = [set_of(partition_text(r, name)) if s is None else s for r, s in zip(rows, sets)]
        out.append(sets)
    return out, keys
