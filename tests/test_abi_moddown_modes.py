"""The ModDown modes at the C boundary, no device: agx_ntt_basis_create_plain, agx_ntt_basis_mod_down_mode and agx_ntt_keyswitch_create_plain are declared
AGX_API int with the prototypes stated below, exported and bound; Basis, KeySwitch and Plan take t and mode with their defaults and lose nothing; and a call
without a handle returns AGX_ERR_NULL_POINTER whatever its other arguments say -- before the mode, t, the ranges and the overlap rule are looked at -- and
writes nothing.  (No plan can be made without a device: the rules behind the NULL rule are tests/test_gpu_moddown_modes.py's.)"""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "agx_ntt_basis_create_plain":
        "int agx_ntt_basis_create_plain(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, "
        "uint32_t dst_count, uint64_t t);",
    "agx_ntt_basis_mod_down_mode":
        "int agx_ntt_basis_mod_down_mode(const agx_ntt_basis* basis, const uint64_t* d_xq, const uint64_t* d_xp, uint64_t* d_out, uint64_t* d_scratch, "
        "uint64_t batch, int mode, void* stream);",
    "agx_ntt_keyswitch_create_plain":
        "int agx_ntt_keyswitch_create_plain(agx_ntt_keyswitch** ks, const agx_ntt_plan* plan, uint32_t q_count, uint32_t p_first, uint32_t p_count, "
        "uint32_t alpha, uint64_t t);",
}
CTYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}


def _header():
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", PROTOTYPES)
def test_symbol_is_declared_exported_and_bound(agx, name):
    flat = re.sub(r"\s+", " ", _header())
    assert "AGX_API " + PROTOTYPES[name] in flat, name
    assert hasattr(ctypes.CDLL(agx.LIB_PATH), name), name
    restype, argtypes = agx.ABI[name]
    assert restype is ctypes.c_int
    # a handle out-pointer is a pointer to a void pointer, every other pointer a void pointer, every scalar bound by its own width
    declared = [a.strip() for a in PROTOTYPES[name].split("(", 1)[1].rsplit(")", 1)[0].split(",")]
    want = [ctypes.POINTER(ctypes.c_void_p) if "**" in a else ctypes.c_void_p if "*" in a else CTYPES[a.split()[0]] for a in declared]
    assert argtypes == want, (name, declared)
    assert getattr(agx.lib(), name).argtypes == want


def test_they_stand_beside_the_calls_they_extend_and_add_no_handle_or_constant():
    text = _header()
    at = lambda name: text.index(name + "(")      # noqa: E731
    assert at("agx_ntt_basis_create") < at("agx_ntt_basis_create_plain") < at("agx_ntt_basis_mod_down")
    assert at("agx_ntt_basis_mod_down_info") < at("agx_ntt_basis_mod_down_mode") < at("agx_ntt_inner_product")
    assert at("agx_ntt_keyswitch_create") < at("agx_ntt_keyswitch_create_plain") < at("agx_ntt_keyswitch_mod_down") < at("agx_ntt_fill_synthetic")
    assert sorted(re.findall(r"typedef\s+struct\s+(\w+)", text)) == ["agx_ntt_basis", "agx_ntt_group", "agx_ntt_keyswitch", "agx_ntt_plan"]
    assert sorted(re.findall(r"#define\s+(AGX_FORM_\w+|AGX_RESCALE_\w+)", text)) == ["AGX_FORM_COEFF", "AGX_FORM_NTT", "AGX_RESCALE_FLOOR", "AGX_RESCALE_ROUND"]


def test_the_python_layer_has_the_keywords_with_their_defaults(agx):
    p = inspect.signature(agx.Basis.__init__).parameters
    assert list(p) == ["self", "plan", "src_first", "src_count", "dst_first", "dst_count", "t"] and p["t"].default == 1
    p = inspect.signature(agx.Plan.basis).parameters
    assert list(p) == ["self", "src_first", "src_count", "dst_first", "dst_count", "t"] and p["t"].default == 1
    p = inspect.signature(agx.Basis.mod_down).parameters
    assert list(p) == ["self", "d_xq", "d_xp", "d_out", "d_scratch", "batch", "stream", "mode"]      # the stream stays the sixth positional argument
    assert (p["stream"].default, p["mode"].default) == (0, agx.RESCALE_FLOOR) and agx.RESCALE_FLOOR == 0 and agx.RESCALE_ROUND == 1
    p = inspect.signature(agx.KeySwitch.__init__).parameters
    assert list(p) == ["self", "plan", "q_count", "p_first", "p_count", "alpha", "t"] and p["t"].default == 1
    p = inspect.signature(agx.Plan.keyswitch).parameters
    assert list(p) == ["self", "q_count", "p_first", "p_count", "alpha", "t"] and p["t"].default == 1
    p = inspect.signature(agx.KeySwitch.mod_down).parameters      # no rounding inside the key switch's ModDown
    assert list(p) == ["self", "d_acc", "d_out", "batch", "stream"]


def test_a_call_without_a_handle_says_so_and_touches_nothing(agx):
    L = agx.lib()
    buf = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.addressof(buf) + k      # noqa: E731
    B, M, K = "agx_ntt_basis_create_plain", "agx_ntt_basis_mod_down_mode", "agx_ntt_keyswitch_create_plain"
    for mode in (0, 1, 7, -1):      # the NULL rule comes before the mode rule
        for args in ((None, at(0), at(64), at(128), at(192), 1, mode, None), (None, at(0), at(0), at(0), at(0), 1, mode, None),
                     (None, at(4), at(1), at(2), at(3), (1 << 64) - 1, mode, None), (None, None, None, None, None, 0, mode, None)):
            assert getattr(L, M)(*args) == 1, (M, args)
    for t in (1, 0, 65537, (1 << 64) - 1):      # ... and before t and the ranges
        assert getattr(L, B)(None, None, 0, 1, 0, 1, t) == 1
        assert getattr(L, K)(None, None, 4, 4, 2, 2, t) == 1
        for ranges in ((0, 1, 0, 1), (0, 0, 0, 0), (7, 99, 3, 0xffffffff)):
            h = ctypes.c_void_p(0x1234)
            assert getattr(L, B)(ctypes.byref(h), None, *ranges, t) == 1 and h.value is None      # the out-pointer is cleared, nothing else
            h = ctypes.c_void_p(0x1234)
            assert getattr(L, K)(ctypes.byref(h), None, *ranges, t) == 1 and h.value is None
    assert all(w == 0 for w in buf), "a buffer was written"
    # a wrapper without a handle reports the same status, in either mode
    basis = agx.Basis.__new__(agx.Basis)
    basis._h = ctypes.c_void_p(None)
    for mode in (agx.RESCALE_FLOOR, agx.RESCALE_ROUND, 7):
        with pytest.raises(agx.AgxError) as e:
            basis.mod_down(at(0), at(64), at(128), at(192), 1, 0, mode)
        assert e.value.status == 1
    for make in (lambda: agx.Basis(None, 0, 1, 0, 1, t=65537), lambda: agx.KeySwitch(None, 4, 4, 2, 2, t=65537)):
        with pytest.raises(agx.AgxError) as e:
            make()
        assert e.value.status == 1
    assert all(w == 0 for w in buf), "a buffer was written"
