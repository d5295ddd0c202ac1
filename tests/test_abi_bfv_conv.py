"""The BEHZ base conversions at the C boundary, no device: agx_ntt_basis_create_aux, agx_ntt_basis_aux_info, agx_ntt_basis_extend_exact and
agx_ntt_basis_extend_mont are declared AGX_API int with the prototypes stated below, exported and bound; they stand behind agx_ntt_basis_mod_down_mode and in
front of agx_ntt_inner_product and add no handle type and no constant; Basis and Plan have the new methods and keep the signatures they had; and a call
without a handle or with a NULL pointer returns AGX_ERR_NULL_POINTER whatever its other arguments say, and writes nothing.  (No plan can be made without a
device: the rules behind the NULL rule are tests/test_gpu_bfv_conv.py's.)"""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "agx_ntt_basis_create_aux":
        "int agx_ntt_basis_create_aux(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, "
        "uint32_t dst_count, uint32_t aux_prime);",
    "agx_ntt_basis_aux_info": "int agx_ntt_basis_aux_info(const agx_ntt_basis* basis, int* has_aux, uint32_t* aux_prime, int* launches_ntt_form);",
    "agx_ntt_basis_extend_exact":
        "int agx_ntt_basis_extend_exact(const agx_ntt_basis* basis, const uint64_t* d_x, const uint64_t* d_xaux, uint64_t* d_out, uint64_t batch, "
        "int out_form, void* stream);",
    "agx_ntt_basis_extend_mont":
        "int agx_ntt_basis_extend_mont(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream);",
}
CTYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}


def _header():
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _bound(arg):
    """a handle out-pointer is a pointer to a void pointer, an int or uint32_t out-pointer (the info calls) a pointer to its own width, every other
    pointer a void pointer, every scalar bound by its own width"""
    if "**" in arg:
        return ctypes.POINTER(ctypes.c_void_p)
    if "*" in arg:
        base = arg.replace("const ", "").split("*")[0].strip()
        return ctypes.POINTER(CTYPES[base]) if base in ("int", "uint32_t") else ctypes.c_void_p
    return CTYPES[arg.split()[0]]


@pytest.mark.parametrize("name", PROTOTYPES)
def test_symbol_is_declared_exported_and_bound(agx, name):
    flat = re.sub(r"\s+", " ", _header())
    assert "AGX_API " + PROTOTYPES[name] in flat, name
    assert hasattr(ctypes.CDLL(agx.LIB_PATH), name), name
    restype, argtypes = agx.ABI[name]
    assert restype is ctypes.c_int
    declared = [a.strip() for a in PROTOTYPES[name].split("(", 1)[1].rsplit(")", 1)[0].split(",")]
    want = [_bound(a) for a in declared]
    assert argtypes == want, (name, declared)
    assert getattr(agx.lib(), name).argtypes == want


def test_they_stand_behind_mod_down_mode_and_add_no_handle_or_constant():
    text = _header()
    at = lambda name: text.index(name + "(")      # noqa: E731
    order = ["agx_ntt_basis_mod_down_mode", "agx_ntt_basis_create_aux", "agx_ntt_basis_aux_info", "agx_ntt_basis_extend_exact", "agx_ntt_basis_extend_mont",
             "agx_ntt_inner_product"]
    assert [at(name) for name in order] == sorted(at(name) for name in order)
    assert sorted(re.findall(r"typedef\s+struct\s+(\w+)", text)) == ["agx_ntt_basis", "agx_ntt_group", "agx_ntt_keyswitch", "agx_ntt_plan"]
    assert sorted(re.findall(r"#define\s+(AGX_FORM_\w+|AGX_RESCALE_\w+)", text)) == ["AGX_FORM_COEFF", "AGX_FORM_NTT", "AGX_RESCALE_FLOOR", "AGX_RESCALE_ROUND"]


def test_the_python_layer_has_the_methods_and_keeps_its_signatures(agx):
    p = inspect.signature(agx.Basis.__init__).parameters
    assert list(p) == ["self", "plan", "src_first", "src_count", "dst_first", "dst_count", "t"] and p["t"].default == 1
    p = inspect.signature(agx.Plan.basis).parameters
    assert list(p) == ["self", "src_first", "src_count", "dst_first", "dst_count", "t"] and p["t"].default == 1
    assert list(inspect.signature(agx.Basis.with_aux).parameters) == ["plan", "src_first", "src_count", "dst_first", "dst_count", "aux_prime"]
    assert isinstance(inspect.getattr_static(agx.Basis, "with_aux"), classmethod)
    assert list(inspect.signature(agx.Plan.basis_aux).parameters) == ["self", "src_first", "src_count", "dst_first", "dst_count", "aux_prime"]
    assert list(inspect.signature(agx.Basis.aux_info).parameters) == ["self"]
    p = inspect.signature(agx.Basis.extend_exact).parameters
    assert list(p) == ["self", "d_x", "d_xaux", "d_out", "batch", "form", "stream"] and (p["form"].default, p["stream"].default) == (agx.FORM_NTT, 0)
    p = inspect.signature(agx.Basis.extend_mont).parameters
    assert list(p) == ["self", "d_x", "d_out", "batch", "form", "stream"] and (p["form"].default, p["stream"].default) == (agx.FORM_NTT, 0)
    p = inspect.signature(agx.Basis.extend).parameters
    assert list(p) == ["self", "d_x", "d_out", "batch", "form", "stream"]


def test_a_call_without_a_handle_or_a_pointer_says_so_and_touches_nothing(agx):
    L = agx.lib()
    buf = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.addressof(buf) + k      # noqa: E731
    fake = ctypes.addressof(buf)      # stands for a handle where the NULL rule must answer before the handle is read
    for form in (0, 1, 7, -1):      # the NULL rule comes before the form, the alignment, the batch and the overlap rule
        for args in ((None, at(0), at(64), at(128), 1, form, None), (None, at(0), at(0), at(0), 1, form, None), (None, at(4), at(1), at(2), (1 << 64) - 1, form, None),
                     (None, None, None, None, 0, form, None), (fake, None, at(64), at(128), 1, form, None), (fake, at(0), None, at(128), 1, form, None),
                     (fake, at(0), at(64), None, 1, form, None)):
            assert L.agx_ntt_basis_extend_exact(*args) == 1, args
        for args in ((None, at(0), at(128), 1, form, None), (None, at(0), at(0), 1, form, None), (None, at(3), at(5), (1 << 64) - 1, form, None),
                     (None, None, None, 0, form, None), (fake, None, at(128), 1, form, None), (fake, at(0), None, 1, form, None)):
            assert L.agx_ntt_basis_extend_mont(*args) == 1, args
    has, prime, launches = ctypes.c_int(-5), ctypes.c_uint32(77), ctypes.c_int(-5)
    assert L.agx_ntt_basis_aux_info(None, ctypes.byref(has), ctypes.byref(prime), ctypes.byref(launches)) == 1
    assert L.agx_ntt_basis_aux_info(None, None, None, None) == 1
    assert (has.value, prime.value, launches.value) == (-5, 77, -5)
    for aux in (0, 3, 0xffffffff):      # ... and before the ranges and the auxiliary prime
        assert L.agx_ntt_basis_create_aux(None, None, 0, 1, 1, 1, aux) == 1
        for ranges in ((0, 1, 1, 1), (0, 0, 0, 0), (7, 99, 3, 0xffffffff)):
            h = ctypes.c_void_p(0x1234)
            assert L.agx_ntt_basis_create_aux(ctypes.byref(h), None, *ranges, aux) == 1 and h.value is None      # the out-pointer is cleared, nothing else
    assert all(w == 0 for w in buf), "a buffer was written"
    # a wrapper without a handle reports the same status
    basis = agx.Basis.__new__(agx.Basis)
    basis._h = ctypes.c_void_p(None)
    for call in (lambda: basis.extend_exact(at(0), at(64), at(128), 1), lambda: basis.extend_mont(at(0), at(128), 1, agx.FORM_COEFF), basis.aux_info,
                 lambda: agx.Basis.with_aux(None, 0, 1, 1, 1, 2)):
        with pytest.raises(agx.AgxError) as e:
            call()
        assert e.value.status == 1
    assert all(w == 0 for w in buf), "a buffer was written"
