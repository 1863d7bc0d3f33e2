"""The streaming ingest's surface without a GPU: the header declares bsg_ingest_open / bsg_ingest_add_sets /
bsg_ingest_append_rows with the documented argument names, the built library exports them, ctypes binds them with the header's
arity, a null context is refused, the engine mirror refuses DeviceIngestStream without DeviceIngest before it looks at the
context, and the Go binding agrees with the header (tools/check_go.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

from bloomsearch_amd import _lib, host as Hst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "bsg_ingest_open": ["ctx", "n_sets", "parent_of_set", "n_parents", "slots_hint", "flags", "tok", "out_ingest_id"],
    "bsg_ingest_add_sets": ["ctx", "ingest_id", "n_more", "parent_of_new_set", "slots_hint_new", "out_first_new_set"],
    "bsg_ingest_append_rows": ["ctx", "ingest_id", "rows", "row_off", "n_rows", "set_of_row", "out_fallback_rows", "fallback_cap", "out_n_fallback"],
}


def declared(name):
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    m = re.search(r"BSG_API int32_t %s\(([^;]*)\);" % name, gpu_h)
    assert m, "bloomgpu.h does not declare " + name
    return [re.split(r"[ *]", p.strip())[-1] for p in m.group(1).replace("\n", " ").split(",")]


def test_header_library_and_ctypes_agree():
    L = _lib.load()
    for name, args in WANT.items():
        assert declared(name) == args, name
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == len(args), name
    out, first, n = C.c_uint64(), C.c_uint32(), C.c_uint32()
    assert L.bsg_ingest_open(None, 0, None, 0, None, 0, None, C.byref(out)) == _lib.BSG_E_INVALID
    assert L.bsg_ingest_add_sets(None, 1, 0, None, None, C.byref(first)) == _lib.BSG_E_INVALID
    assert L.bsg_ingest_append_rows(None, 1, None, None, 0, None, None, 0, C.byref(n)) == _lib.BSG_E_INVALID
    assert L.bsg_last_error(None)


def test_the_header_states_the_limits_of_a_stream():
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    doc = gpu_h[gpu_h.index("streaming device ingest"): gpu_h.index("BSG_API int32_t bsg_ingest_fallback_rows")]
    assert "ONE device" in doc and "1 024" in doc and "fallback_cap" in doc and "BSG_E_NOTFOUND" in doc


def test_engine_config_needs_device_ingest():
    H = Hst.lib()
    h = C.c_void_p()
    for cfg, want in ((b'{"DeviceIngestStream":true}', -101), (b'{"DeviceIngestStream":true,"DeviceIngest":false}', -101)):
        assert H.bse_open(cfg, len(cfg), None, C.byref(h)) == want, cfg            # the config is checked before the context
    ok = b'{"DeviceIngestStream":true,"DeviceIngest":true}'
    assert H.bse_open(ok, len(ok), None, C.byref(h)) not in (0, -101)              # a valid config, refused only for its NULL context


def test_go_binding_has_the_three_calls():
    src = open(os.path.join(ROOT, "go", "bloomgpu", "bloomgpu.go")).read()
    for fn, call in (("func (g *Context) IngestOpen(", "C.bsg_ingest_open("), ("func (in *Ingest) IngestAddSets(", "C.bsg_ingest_add_sets("),
                     ("func (in *Ingest) IngestAppendRows(", "C.bsg_ingest_append_rows(")):
        assert fn in src and call in src, fn
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
