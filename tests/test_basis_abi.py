"""CPU tests of the fast base conversion's boundary: agx_ntt_basis_create / _destroy / _info / _extend are declared by include/agx_ntt.h,
exported by the library and bound by the Python layer; AGX_BASIS_MAX_SRC is 16 on both sides; without a basis or a plan every entry
point says so (status 1) before it touches a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("agx_ntt_basis_create", "agx_ntt_basis_destroy", "agx_ntt_basis_info", "agx_ntt_basis_extend")


def _header():
    """include/agx_ntt.h without its comments"""
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_are_declared_exported_and_bound(agx):
    text = _header()
    raw = ctypes.CDLL(agx.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"AGX_API\s+int\s+" + name + r"\s*\(", text), name
        assert hasattr(raw, name), name
        assert name in agx.ABI and agx.ABI[name][0] is ctypes.c_int, name
    assert re.search(r"typedef\s+struct\s+agx_ntt_basis\s+agx_ntt_basis\s*;", text)


def test_argument_counts_match_the_header(agx):
    want = {"agx_ntt_basis_create": 6, "agx_ntt_basis_destroy": 1, "agx_ntt_basis_info": 6, "agx_ntt_basis_extend": 6}
    text = _header()
    for name, count in want.items():
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text).group(1)
        assert len(args.split(",")) == count == len(agx.ABI[name][1]), name


def test_python_layer_has_the_basis(agx):
    assert isinstance(agx.Basis, type)
    for method in ("extend", "info", "close"):
        assert callable(getattr(agx.Basis, method)), method
    assert callable(agx.Plan.basis)


def test_source_cap_is_16_in_header_and_binding(agx):
    assert re.findall(r"#define\s+AGX_BASIS_MAX_SRC\s+(\d+)", _header()) == ["16"]
    assert agx.BASIS_MAX_SRC == 16


def test_no_new_form_or_rescale_constants(agx):
    """out_form reuses AGX_FORM_COEFF / AGX_FORM_NTT"""
    assert sorted(re.findall(r"#define\s+(AGX_FORM_\w+|AGX_RESCALE_\w+)", _header())) == ["AGX_FORM_COEFF", "AGX_FORM_NTT", "AGX_RESCALE_FLOOR", "AGX_RESCALE_ROUND"]


def test_null_basis_or_plan_is_status_1(agx):
    L = agx.lib()
    h = ctypes.c_void_p(None)
    assert L.agx_ntt_basis_create(None, None, 0, 1, 0, 1) == 1
    assert L.agx_ntt_basis_create(ctypes.byref(h), None, 0, 1, 0, 1) == 1 and not h.value      # no plan
    assert L.agx_ntt_basis_create(ctypes.byref(h), None, 0, 0, 0, 0) == 1 and not h.value      # ... whatever the ranges
    v = [ctypes.c_uint32(7) for _ in range(4)]
    k = ctypes.c_int(7)
    assert L.agx_ntt_basis_info(None, *[ctypes.byref(x) for x in v], ctypes.byref(k)) == 1
    assert L.agx_ntt_basis_info(None, None, None, None, None, None) == 1
    assert [x.value for x in v] == [7] * 4 and k.value == 7
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(buf)
    for form in (0, 1, 7):
        assert L.agx_ntt_basis_extend(None, p, p, 1, form, None) == 1
        assert L.agx_ntt_basis_extend(None, None, None, 0, form, None) == 1
    assert all(w == 0 for w in buf)


def test_destroying_nothing_is_fine(agx):
    assert agx.lib().agx_ntt_basis_destroy(None) == 0
    assert agx.lib().agx_ntt_basis_destroy(None) == 0
