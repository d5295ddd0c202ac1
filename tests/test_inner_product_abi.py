"""CPU tests of agx_ntt_inner_product's boundary: declared by include/agx_ntt.h with its two limits, exported by the library and bound by the Python
layer with the header's argument count; without a plan it says so (status 1) before it touches a device or any memory."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {"agx_ntt_inner_product": 9}


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


def test_symbol_is_declared_exported_and_bound(agx):
    text = _header()
    raw = ctypes.CDLL(agx.LIB_PATH)
    for name in WANT:
        assert re.search(r"AGX_API\s+int\s+" + name + r"\s*\(", text), name
        assert hasattr(raw, name), name
        assert name in agx.ABI and agx.ABI[name][0] is ctypes.c_int, name


def test_argument_count_matches_the_header(agx):
    text = _header()
    for name, count in WANT.items():
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text).group(1)
        assert len(args.split(",")) == count == len(agx.ABI[name][1]), name


def test_limits_are_defined_and_mirrored(agx):
    text = _header()
    assert re.search(r"#define\s+AGX_INNER_MAX_TERMS\s+16\b", text) and re.search(r"#define\s+AGX_INNER_MAX_OUTPUTS\s+2\b", text)
    assert (agx.INNER_MAX_TERMS, agx.INNER_MAX_OUTPUTS) == (16, 2)


def test_python_layer_has_the_method(agx):
    assert callable(agx.Plan.inner_product)


def test_the_basis_prototypes_are_unchanged(agx):
    text = re.sub(r"\s+", " ", _header())
    for proto in ("int agx_ntt_basis_create(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count);",
                  "int agx_ntt_basis_destroy(agx_ntt_basis* basis);",
                  "int agx_ntt_basis_info(const agx_ntt_basis* basis, uint32_t* src_first, uint32_t* src_count, uint32_t* dst_first, uint32_t* dst_count, int* launches_ntt_form);",
                  "int agx_ntt_basis_extend(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream);",
                  "int agx_ntt_basis_mod_down(const agx_ntt_basis* basis, const uint64_t* d_xq, const uint64_t* d_xp, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream);",
                  "int agx_ntt_basis_mod_down_info(const agx_ntt_basis* basis, int* launches);",
                  "int agx_ntt_pointwise(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, void* stream);"):
        assert proto in text, proto


def test_null_plan_is_status_1_and_touches_nothing(agx):
    L = agx.lib()
    buf = (ctypes.c_uint64 * 48)()
    p = ctypes.addressof(buf)
    assert L.agx_ntt_inner_product(None, p, p + 128, p + 256, 1, 1, 1, 1, None) == 1
    assert L.agx_ntt_inner_product(None, p, p, p, 1, 1, 2, 2, None) == 1
    assert L.agx_ntt_inner_product(None, p, p + 128, p + 256, 1, 1, 0, 3, None) == 1      # the NULL rule comes first
    assert L.agx_ntt_inner_product(None, None, None, None, 0, 0, 0, 0, None) == 1
    assert all(w == 0 for w in buf)
