"""CPU tests of the key switch's boundary: the five agx_ntt_keyswitch_* calls are declared by include/agx_ntt.h, exported by the library and bound by
the Python layer with the header's argument counts; without a handle or a plan each says so (status 1) before it touches a device or any memory,
and destroying no handle is fine."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {"agx_ntt_keyswitch_create": 6, "agx_ntt_keyswitch_destroy": 1, "agx_ntt_keyswitch_info": 7, "agx_ntt_keyswitch_scratch_words": 3,
        "agx_ntt_keyswitch_apply": 7}


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
    assert re.search(r"typedef\s+struct\s+agx_ntt_keyswitch\s+agx_ntt_keyswitch\s*;", text)
    assert re.search(r"#define\s+AGX_KEYSWITCH_MAX_DIGITS\s+16\b", text) and agx.KEYSWITCH_MAX_DIGITS == 16


def test_argument_counts_match_the_header(agx):
    text = _header()
    for name, count in WANT.items():
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text).group(1)
        assert len(args.split(",")) == count == len(agx.ABI[name][1]), name


def test_python_layer_has_the_methods(agx):
    assert callable(agx.Plan.keyswitch)
    for method in ("info", "scratch_words", "apply", "close"):
        assert callable(getattr(agx.KeySwitch, method)), method


def test_the_basis_prototypes_are_unchanged(agx):
    text = re.sub(r"\s+", " ", _header())
    for proto in ("int agx_ntt_basis_create(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count);",
                  "int agx_ntt_basis_destroy(agx_ntt_basis* basis);",
                  "int agx_ntt_basis_info(const agx_ntt_basis* basis, uint32_t* src_first, uint32_t* src_count, uint32_t* dst_first, uint32_t* dst_count, int* launches_ntt_form);",
                  "int agx_ntt_basis_extend(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream);",
                  "int agx_ntt_basis_mod_down(const agx_ntt_basis* basis, const uint64_t* d_xq, const uint64_t* d_xp, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream);",
                  "int agx_ntt_basis_mod_down_info(const agx_ntt_basis* basis, int* launches);"):
        assert proto in text, proto


def test_null_handle_or_plan_is_status_1_and_touches_nothing(agx):
    L = agx.lib()
    h = ctypes.c_void_p(0x1234)
    assert L.agx_ntt_keyswitch_create(None, None, 4, 4, 2, 2) == 1
    assert L.agx_ntt_keyswitch_create(ctypes.byref(h), None, 4, 4, 2, 2) == 1 and h.value is None      # the out-pointer is cleared, nothing else
    assert L.agx_ntt_keyswitch_destroy(None) == 0
    v = [ctypes.c_uint32(7) for _ in range(5)]
    k = ctypes.c_int(7)
    assert L.agx_ntt_keyswitch_info(None, *[ctypes.byref(x) for x in v], ctypes.byref(k)) == 1
    assert all(x.value == 7 for x in v) and k.value == 7
    assert L.agx_ntt_keyswitch_info(None, None, None, None, None, None, None) == 1
    words = (ctypes.c_uint64 * 1)(7)
    assert L.agx_ntt_keyswitch_scratch_words(None, 5, words) == 1 and words[0] == 7
    assert L.agx_ntt_keyswitch_scratch_words(None, 5, None) == 1
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    assert L.agx_ntt_keyswitch_apply(None, p, p + 128, p + 256, p + 384, 1, None) == 1
    assert L.agx_ntt_keyswitch_apply(None, p, p, p, p, 1, None) == 1
    assert L.agx_ntt_keyswitch_apply(None, None, None, None, None, 0, None) == 1
    assert all(w == 0 for w in buf)
