"""CPU tests of ModDown's boundary: agx_ntt_basis_mod_down and agx_ntt_basis_mod_down_info are declared by include/agx_ntt.h, exported by the
library and bound by the Python layer with the header's argument counts; without a basis both say so (status 1) before they touch a device or
any memory."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {"agx_ntt_basis_mod_down": 7, "agx_ntt_basis_mod_down_info": 2}


def _header():
    """include/agx_ntt.h without its comments"""
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_are_declared_exported_and_bound(agx):
    text = _header()
    raw = ctypes.CDLL(agx.LIB_PATH)
    for name in WANT:
        assert re.search(r"AGX_API\s+int\s+" + name + r"\s*\(", text), name
        assert hasattr(raw, name), name
        assert name in agx.ABI and agx.ABI[name][0] is ctypes.c_int, name


def test_argument_counts_match_the_header(agx):
    text = _header()
    for name, count in WANT.items():
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text).group(1)
        assert len(args.split(",")) == count == len(agx.ABI[name][1]), name


def test_python_layer_has_the_methods(agx):
    for method in ("mod_down", "mod_down_launches"):
        assert callable(getattr(agx.Basis, method)), method


def test_the_four_earlier_basis_prototypes_are_unchanged(agx):
    text = re.sub(r"\s+", " ", _header())
    for proto in ("int agx_ntt_basis_create(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count);",
                  "int agx_ntt_basis_destroy(agx_ntt_basis* basis);",
                  "int agx_ntt_basis_info(const agx_ntt_basis* basis, uint32_t* src_first, uint32_t* src_count, uint32_t* dst_first, uint32_t* dst_count, int* launches_ntt_form);",
                  "int agx_ntt_basis_extend(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream);"):
        assert proto in text, proto


def test_null_basis_is_status_1_and_touches_nothing(agx):
    L = agx.lib()
    k = ctypes.c_int(7)
    assert L.agx_ntt_basis_mod_down_info(None, ctypes.byref(k)) == 1 and k.value == 7
    assert L.agx_ntt_basis_mod_down_info(None, None) == 1
    buf = (ctypes.c_uint64 * 32)()
    p = ctypes.addressof(buf)
    assert L.agx_ntt_basis_mod_down(None, p, p + 64, p + 128, p + 192, 1, None) == 1
    assert L.agx_ntt_basis_mod_down(None, p, p, p, p, 1, None) == 1
    assert L.agx_ntt_basis_mod_down(None, None, None, None, None, 0, None) == 1
    assert all(w == 0 for w in buf)
