"""The keyed ingest at the C boundary, without a device: the header declares the five calls, the library exports them with those
signatures, every call refuses a NULL context, the constants of _lib.py and the kernel header are the header's, the lab key is
documented, and the partition kernels are kernels of their own beside the walkers and the MinMax scanner."""
import ctypes as C
import os
import re

from bloomsearch_amd import _lib, host
from bloomsearch_amd._lib import BSG_E_INVALID
from tests.test_regex_substr_cabi import constant, params
from tests import partition_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bloomsearch_amd", "csrc")
GPU_H = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
LAB_H = open(os.path.join(ROOT, "include", "bloomgpu_lab.h")).read()
HOST_H = open(os.path.join(ROOT, "include", "bloomsearch_host.h")).read()
CALLS = ("bsg_ingest_open_keyed", "bsg_ingest_append_rows_keyed", "bsg_ingest_add_sets_keyed", "bsg_ingest_keys", "bsg_last_partition_ms")


def test_the_header_declares_the_calls():
    assert params("bsg_ingest_open_keyed", GPU_H) == [
        "bsg_ctx *ctx", "uint32_t n_parents", "uint32_t parent_of_new_sets", "uint32_t flags", "const bsg_tokenizer *tok", "uint64_t *out_ingest_id",
        "const uint8_t *name_bytes", "uint32_t name_len", "const uint8_t *field_bytes", "const uint32_t *field_off", "uint32_t n_fields"]
    plain = params("bsg_ingest_append_rows", GPU_H)
    assert params("bsg_ingest_append_rows_keyed", GPU_H) == plain[:5] + ["uint32_t *out_set_of_row", "uint32_t *out_n_new_sets"] + plain[6:]
    assert "const uint32_t *set_of_row" == plain[5]
    assert params("bsg_ingest_add_sets_keyed", GPU_H) == ["bsg_ctx *ctx", "uint64_t ingest_id", "const uint8_t *key_bytes", "const uint32_t *key_off",
                                                          "uint32_t n_keys", "uint32_t *out_set_of_key"]
    assert params("bsg_ingest_keys", GPU_H)[:3] == ["bsg_ctx *ctx", "uint64_t ingest_id", "uint32_t first"]
    assert params("bsg_last_partition_ms", GPU_H) == ["bsg_ctx *ctx", "float *partition_ms"]
    # the streaming calls keep their signatures
    assert len(plain) == 9 and len(params("bsg_ingest_add_sets", GPU_H)) == 6 and len(params("bsg_ingest_open", GPU_H)) == 8
    block = GPU_H[GPU_H.index("/* ---- keyed streaming ingest"): GPU_H.index("#define BSG_PARTITION_MAX_NAME")]
    for phrase in ("FIRST top-level member", "raw\n * literal exactly as written", "holds a backslash", "BSG_PARTITION_MAX_KEY", "lowest row index",
                   "bit-identical", "plain bsg_ingest_add_sets on a keyed ingest is BSG_E_INVALID"):
        assert phrase in block, phrase


def test_the_library_exports_them_and_every_call_refuses_a_null_context():
    L = _lib.load()
    for name in CALLS:
        assert hasattr(L, name) and name in _lib.EXPORTS
        assert len(getattr(L, name).argtypes) == len(params(name, GPU_H)), name
    out, n, m, nb, ms = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_float()
    name = (C.c_uint8 * 1)(112)
    assert L.bsg_ingest_open_keyed(None, 1, 0, 0, None, C.byref(out), name, 1, None, None, 0) == BSG_E_INVALID
    assert L.bsg_ingest_append_rows_keyed(None, 1, None, None, 0, None, C.byref(m), None, 0, C.byref(n)) == BSG_E_INVALID
    assert L.bsg_ingest_add_sets_keyed(None, 1, None, None, 0, None) == BSG_E_INVALID
    assert L.bsg_ingest_keys(None, 1, 0, None, 0, None, C.byref(n), C.byref(nb)) == BSG_E_INVALID
    assert L.bsg_last_partition_ms(None, C.byref(ms)) == BSG_E_INVALID


def define(name, text=GPU_H):
    m = re.search(r"#define %s\s+(\(1u << \d+\)|0x[0-9A-Fa-f]+u|\d+u)" % name, text)
    assert m, name
    v = m.group(1)
    if v.startswith("("):
        return 1 << int(re.search(r"<< (\d+)", v).group(1))
    return int(v[:-1], 0)


def test_the_constants_agree_with_the_header_and_the_kernels():
    kernel = open(os.path.join(CSRC, "partition.hip.h")).read()
    assert _lib.PARTITION_MAX_NAME == define("BSG_PARTITION_MAX_NAME") == constant(kernel, "kPkeyMaxName") == PR.MAX_NAME == 64
    assert _lib.PARTITION_MAX_KEY == define("BSG_PARTITION_MAX_KEY") == constant(kernel, "kPkeyMaxKey") == PR.MAX_KEY
    assert _lib.PARTITION_MAX_KEY >= 64
    assert _lib.PARTITION_PENDING_SLOTS == define("BSG_PARTITION_PENDING_SLOTS") == constant(kernel, "kPkeyPendingSlots")
    assert _lib.PARTITION_PENDING_SLOTS & (_lib.PARTITION_PENDING_SLOTS - 1) == 0          # the kernels mask with it
    assert _lib.PARTITION_MAX_SETS == define("BSG_PARTITION_MAX_SETS")
    assert _lib.SET_UNDECIDED == define("BSG_SET_UNDECIDED") == 0xFFFFFFFF
    assert "kPkeyUndecided = 0xFFFFFFFFu" in kernel
    host_hdr = open(os.path.join(CSRC, "host", "partition.hpp")).read()
    assert constant(host_hdr, "kPartitionMaxName") == 64
    assert C.sizeof(_lib.IngestStats) == 48                        # bsg_ingest_stats keeps its layout
    assert "key 29" in LAB_H and "low 2 bits" in LAB_H and _lib.LAB_PARTITION_HASH_MASK == 29
    assert "bloomgpu_lab.h" not in open(os.path.join(ROOT, "go", "bloomgpu", "bloomgpu.go")).read()


def test_the_host_call_is_declared_and_exported():
    L = host.lib()
    assert hasattr(L, "bsh_partition_key") and "bsh_partition_key" in host.HOST_EXPORTS
    assert len(L.bsh_partition_key.argtypes) == len(params("bsh_partition_key", HOST_H)) == 7
    n = C.c_uint64()
    assert L.bsh_partition_key(b"{}", 2, b"p", 1, None, 0, None) == -1                     # no out_len
    assert L.bsh_partition_key(b"{}", 2, None, 1, None, 0, C.byref(n)) == -1
    assert L.bsh_partition_key(b'{"p":"abc"}', 11, b"p", 1, None, 0, C.byref(n)) == 0 and n.value == 3      # the length alone


def test_the_partition_kernels_are_kernels_of_their_own():
    kernel = open(os.path.join(CSRC, "partition.hip.h")).read()
    for name in ("k_partition_rows", "k_partition_assign"):
        assert len(re.findall(r"void %s\(" % name, kernel)) == 1, name
    for other in ("minmax.hip.h", "ingest.hip.h"):                 # the walkers and the MinMax scanner are not edited
        assert "k_partition" not in open(os.path.join(CSRC, other)).read() and "kPkey" not in open(os.path.join(CSRC, other)).read(), other
    api = open(os.path.join(CSRC, "ingest_api.inc")).read()
    assert api.count("bsg::k_partition_rows,") == 1 and api.count("bsg::k_partition_assign,") == 1
    # a lookup is decided by the bytes, never by the tag alone
    lookup = kernel[kernel.index("uint32_t part_lookup("): kernel.index("// a slot for this tag")]
    assert "a.pool[e.off + k] == part_byte(" in lookup and "if (k == len) return e.set;" in lookup
    # plain add_sets refuses a keyed ingest
    add = api[api.index("int32_t bsg_ingest_add_sets(bsg_ctx"): api.index("int32_t bsg_ingest_append_rows(bsg_ctx")]
    assert "if (I.keyed) return fail(BSG_E_INVALID" in add
