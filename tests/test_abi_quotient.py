"""agx_ntt_basis_quotient and the range transforms at the C boundary, no device: agx_ntt_basis_create_quotient, agx_ntt_basis_quotient_info,
agx_ntt_basis_quotient, agx_ntt_forward_range and agx_ntt_inverse_range are declared AGX_API int with the prototypes stated below, exported and bound; the
three basis calls stand right behind agx_ntt_basis_extend_mont and in front of agx_ntt_inner_product, the range transforms behind agx_ntt_inverse_strided,
and none adds a handle type or a constant; Basis and Plan have the new methods and keep the signatures they had; and a call without a handle or with a
NULL pointer returns AGX_ERR_NULL_POINTER whatever its other arguments say, writes nothing, and clears a handle out-pointer.  (No plan can be made without a
device: the rules behind the NULL rule are tests/test_gpu_quotient.py's.)"""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "agx_ntt_basis_create_quotient":
        "int agx_ntt_basis_create_quotient(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t b_first, uint32_t b_count, uint32_t q_first, "
        "uint32_t q_count, uint32_t aux_prime, uint64_t t);",
    "agx_ntt_basis_quotient_info": "int agx_ntt_basis_quotient_info(const agx_ntt_basis* basis, int* has_quotient, uint64_t* t, int* launches);",
    "agx_ntt_basis_quotient":
        "int agx_ntt_basis_quotient(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream);",
    "agx_ntt_forward_range":
        "int agx_ntt_forward_range(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t prime_first, "
        "uint32_t prime_count, void* stream);",
    "agx_ntt_inverse_range":
        "int agx_ntt_inverse_range(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t prime_first, "
        "uint32_t prime_count, void* stream);",
}
CTYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}
OUT_WORDS = {"agx_ntt_basis_quotient_info": ("t",)}      # uint64_t out-parameters: bound by their own width; every other uint64_t pointer is device data


def _header():
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _bound(name, arg):
    """a handle out-pointer is a pointer to a void pointer, an int, uint32_t or (the info call's t) uint64_t out-pointer a pointer to its own width, every
    other pointer a void pointer, every scalar bound by its own width"""
    if "**" in arg:
        return ctypes.POINTER(ctypes.c_void_p)
    if "*" in arg:
        base, ident = arg.replace("const ", "").split("*")[0].strip(), arg.split("*")[-1].strip()
        return ctypes.POINTER(CTYPES[base]) if base in ("int", "uint32_t") or ident in OUT_WORDS.get(name, ()) else ctypes.c_void_p
    return CTYPES[arg.split()[0]]


@pytest.mark.parametrize("name", PROTOTYPES)
def test_symbol_is_declared_exported_and_bound(agx, name):
    flat = re.sub(r"\s+", " ", _header())
    assert "AGX_API " + PROTOTYPES[name] in flat, name
    assert hasattr(ctypes.CDLL(agx.LIB_PATH), name), name
    restype, argtypes = agx.ABI[name]
    assert restype is ctypes.c_int
    declared = [a.strip() for a in PROTOTYPES[name].split("(", 1)[1].rsplit(")", 1)[0].split(",")]
    want = [_bound(name, a) for a in declared]
    assert argtypes == want, (name, declared)
    assert getattr(agx.lib(), name).argtypes == want


def test_where_they_stand_and_that_they_add_no_handle_or_constant():
    text = _header()
    at = lambda name: text.index(name + "(")      # noqa: E731
    for order in (["agx_ntt_basis_extend_mont", "agx_ntt_basis_create_quotient", "agx_ntt_basis_quotient_info", "agx_ntt_basis_quotient", "agx_ntt_inner_product"],
                  ["agx_ntt_inverse_strided", "agx_ntt_forward_range", "agx_ntt_inverse_range", "agx_ntt_pointwise"]):
        assert [at(name) for name in order] == sorted(at(name) for name in order)
    between = text[at("agx_ntt_basis_extend_mont"):at("agx_ntt_basis_quotient")]
    assert re.findall(r"\b(agx_ntt_\w+)\s*\(", between) == ["agx_ntt_basis_extend_mont", "agx_ntt_basis_create_quotient", "agx_ntt_basis_quotient_info"]      # right behind
    assert sorted(re.findall(r"typedef\s+struct\s+(\w+)", text)) == ["agx_ntt_basis", "agx_ntt_group", "agx_ntt_keyswitch", "agx_ntt_plan"]
    assert sorted(re.findall(r"#define\s+(AGX_FORM_\w+|AGX_RESCALE_\w+)", text)) == ["AGX_FORM_COEFF", "AGX_FORM_NTT", "AGX_RESCALE_FLOOR", "AGX_RESCALE_ROUND"]


def test_the_python_layer_has_the_methods_and_keeps_its_signatures(agx):
    p = inspect.signature(agx.Basis.__init__).parameters
    assert list(p) == ["self", "plan", "src_first", "src_count", "dst_first", "dst_count", "t"] and p["t"].default == 1
    assert list(inspect.signature(agx.Basis.with_aux).parameters) == ["plan", "src_first", "src_count", "dst_first", "dst_count", "aux_prime"]
    assert list(inspect.signature(agx.Basis.with_quotient).parameters) == ["plan", "b_first", "b_count", "q_first", "q_count", "aux_prime", "t"]
    assert isinstance(inspect.getattr_static(agx.Basis, "with_quotient"), classmethod)
    assert list(inspect.signature(agx.Plan.basis_quotient).parameters) == ["self", "b_first", "b_count", "q_first", "q_count", "aux_prime", "t"]
    assert list(inspect.signature(agx.Basis.quotient_info).parameters) == ["self"]
    p = inspect.signature(agx.Basis.quotient).parameters
    assert list(p) == ["self", "d_x", "d_out", "d_scratch", "batch", "stream"] and p["stream"].default == 0
    for name in ("forward_range", "inverse_range"):
        p = inspect.signature(getattr(agx.Plan, name)).parameters
        assert list(p) == ["self", "d_in", "d_out", "batch", "prime_first", "prime_count", "stream"] and p["stream"].default == 0
    assert list(inspect.signature(agx.Plan.forward).parameters) == ["self", "d_in", "d_out", "batch", "stream"]
    assert list(inspect.signature(agx.Plan.inverse).parameters) == ["self", "d_in", "d_out", "batch", "stream"]
    p = inspect.signature(agx.Basis.mod_down).parameters
    assert list(p) == ["self", "d_xq", "d_xp", "d_out", "d_scratch", "batch", "stream", "mode"]


def test_a_call_without_a_handle_or_a_pointer_says_so_and_touches_nothing(agx):
    L = agx.lib()
    buf = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.addressof(buf) + k      # noqa: E731
    fake = ctypes.addressof(buf)      # stands for a handle where the NULL rule must answer before the handle is read
    for args in ((None, at(0), at(64), at(128), 1, None), (None, at(0), at(0), at(0), 1, None), (None, at(4), at(1), at(2), (1 << 64) - 1, None),
                 (None, None, None, None, 0, None), (fake, None, at(64), at(128), 1, None), (fake, at(0), None, at(128), 1, None), (fake, at(0), at(64), None, 1, None)):
        assert L.agx_ntt_basis_quotient(*args) == 1, args
    has, t, launches = ctypes.c_int(-5), ctypes.c_uint64(77), ctypes.c_int(-5)
    assert L.agx_ntt_basis_quotient_info(None, ctypes.byref(has), ctypes.byref(t), ctypes.byref(launches)) == 1
    assert L.agx_ntt_basis_quotient_info(None, None, None, None) == 1
    assert (has.value, t.value, launches.value) == (-5, 77, -5)
    for t_arg in (0, 1, 65537, (1 << 64) - 1):      # ... before the ranges, the auxiliary prime and t
        for aux in (0, 3, 0xffffffff):
            assert L.agx_ntt_basis_create_quotient(None, None, 0, 1, 1, 1, aux, t_arg) == 1
            for ranges in ((0, 1, 1, 1), (0, 0, 0, 0), (7, 99, 3, 0xffffffff)):
                h = ctypes.c_void_p(0x1234)
                assert L.agx_ntt_basis_create_quotient(ctypes.byref(h), None, *ranges, aux, t_arg) == 1 and h.value is None      # the out-pointer is cleared
    for fn in (L.agx_ntt_forward_range, L.agx_ntt_inverse_range):
        for first, count in ((0, 1), (0, 0), (5, 0xffffffff)):      # the NULL rule comes before the range rule
            for args in ((None, at(0), at(0), 1), (None, None, None, 0), (fake, None, at(0), 1), (fake, at(0), None, 1), (None, at(4), at(1), (1 << 64) - 1)):
                assert fn(*args, first, count, None) == 1, (args, first, count)
    assert all(w == 0 for w in buf), "a buffer was written"
    # a wrapper without a handle reports the same status
    basis = agx.Basis.__new__(agx.Basis)
    basis._h = ctypes.c_void_p(None)
    plan = agx.Plan.__new__(agx.Plan)
    plan._h = ctypes.c_void_p(None)
    for call in (lambda: basis.quotient(at(0), at(64), at(128), 1), basis.quotient_info, lambda: agx.Basis.with_quotient(None, 0, 1, 1, 1, 2, 65537),
                 lambda: plan.forward_range(at(0), at(0), 1, 0, 1), lambda: plan.inverse_range(at(0), at(0), 1, 0, 1)):
        with pytest.raises(agx.AgxError) as e:
            call()
        assert e.value.status == 1
    assert all(w == 0 for w in buf), "a buffer was written"
    plan._h = None      # nothing to destroy
