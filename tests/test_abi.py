"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/agx_ntt.h declares, validates arguments, and its host math agrees with the oracle.
No compute call can succeed here (no GPU): the product path must fail loudly, not fall back.
Every operation added to the boundary is a row of one of two tables: OPERATIONS (plan and group
forms) and RNS_OPERATIONS (bases, inner products, the key switch and its two halves)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    """include/agx_ntt.h without its comments"""
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _prototypes():
    """{name: (return type, number of arguments)} of every function the header declares"""
    out = {}
    for ret, name, args in re.findall(r"AGX_API\s+([\w\s\*]+?)\s*\b(agx_ntt_\w+)\s*\(([^)]*)\)\s*;", _header()):
        out[name] = (ret.replace(" ", ""), 0 if args.strip() == "void" else len(args.split(",")))
    return out


def _declared_symbols():
    return sorted(set(re.findall(r"\b(agx_ntt_\w+)\s*\(", _header())))


def test_header_and_binding_agree(agx):
    declared = _declared_symbols()
    assert len(declared) >= 20
    assert sorted(agx.ABI) == declared


def test_binding_matches_the_header(agx):
    """argument count and return type of every prototype, as the binding has them: int everywhere but agx_ntt_strerror's char*"""
    protos = _prototypes()
    assert sorted(protos) == _declared_symbols()
    for name, (ret, nargs) in protos.items():
        assert nargs == len(agx.ABI[name][1]), name
        if name == "agx_ntt_strerror":
            assert ret == "constchar*" and agx.ABI[name][0] is ctypes.c_char_p
        else:
            assert ret == "int" and agx.ABI[name][0] is ctypes.c_int, name


# the operations added to the boundary one at a time: their symbols, the Plan / DeviceGroup wrapper, the header's constants with the
# values the binding repeats, and calls with a NULL plan or group with the status each must return before it touches a device
OPERATIONS = {
    "polymul_ntt": {
        "names": ("agx_ntt_polymul_ntt", "agx_ntt_group_polymul_ntt"),
        "constants": {},
        "null_calls": [("agx_ntt_polymul_ntt", (None, None, None, None, 1, 1, None), 1),
                       ("agx_ntt_group_polymul_ntt", (None, None, None, None, None, None), 1)],
    },
    "rescale": {
        "names": ("agx_ntt_rescale", "agx_ntt_group_rescale"),
        "constants": {"RESCALE_FLOOR": 0, "RESCALE_ROUND": 1},
        "null_calls": [("agx_ntt_rescale", (None, None, None, None, 1, 0, None), 1), ("agx_ntt_rescale", (None, None, None, None, 1, 7, None), 1),
                       ("agx_ntt_group_rescale", (None, None, None, None, None, 0), 1), ("agx_ntt_group_rescale", (None, None, None, None, None, 1), 1)],
    },
    "automorphism": {
        "names": ("agx_ntt_automorphism", "agx_ntt_group_automorphism", "agx_ntt_galois_element"),
        "constants": {"FORM_COEFF": 0, "FORM_NTT": 1},
        "null_calls": [(name, args, 1) for form in (0, 1, 7) for name, args in (("agx_ntt_automorphism", (None, None, None, 1, 5, form, None)),
                                                                               ("agx_ntt_group_automorphism", (None, None, None, None, 5, form)))],
    },
}


@pytest.mark.parametrize("op", OPERATIONS)
def test_operation_is_bound_exported_and_declared(agx, op):
    text = _header()
    raw = ctypes.CDLL(agx.LIB_PATH)
    for name in OPERATIONS[op]["names"]:
        assert name in agx.ABI, name
        assert hasattr(raw, name), name
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert hasattr(agx.Plan, op) and hasattr(agx.DeviceGroup, op)
    if op == "automorphism":
        assert callable(agx.galois_element)


@pytest.mark.parametrize("op", [op for op in OPERATIONS if OPERATIONS[op]["constants"]])
def test_operation_constants_match_the_header(agx, op):
    """every AGX_<OP>_* constant of the header, and the same values under the binding's names"""
    want = OPERATIONS[op]["constants"]
    prefix = os.path.commonprefix(["AGX_" + k for k in want])      # AGX_RESCALE_, AGX_FORM_
    assert prefix.endswith("_") and len(prefix) > len("AGX_")
    consts = dict(re.findall(r"#define\s+(" + prefix + r"\w+)\s+(\d+)", _header()))
    assert consts == {"AGX_" + k: str(v) for k, v in want.items()}
    assert all(getattr(agx, k) == v for k, v in want.items())


@pytest.mark.parametrize("op", OPERATIONS)
def test_operation_fails_loudly_without_a_plan_or_a_group(agx, op):
    L = agx.lib()
    for name, args, status in OPERATIONS[op]["null_calls"]:
        assert getattr(L, name)(*args) == status, (name, args)


# ---- the RNS calls: handles of their own (agx_ntt_basis, agx_ntt_keyswitch) or a plan, no group form --------------------------------------------
# Arguments of a NULL-handle call that are more than a value: BUF(k) is the address k bytes into one zeroed buffer, which must still be zero after
# every call of the operation; U32, U64 and INT are out-parameters holding 7, which must keep it; HANDLE(v) is a handle out-parameter holding v,
# which must read NULL afterwards (cleared, or never set).
def BUF(offset=0):
    return ("buf", offset)


def HANDLE(initial):
    return ("handle", initial)


U32, U64, INT = ("out", ctypes.c_uint32), ("out", ctypes.c_uint64), ("out", ctypes.c_int)

# per operation: "names" {symbol: argument count}, every one AGX_API int; "typedefs" the opaque handle types the header declares; "methods" {class of the
# binding: its callables}; "limits" {AGX_<name> of the header = <name> of the binding: value}; "null_calls" [(symbol, arguments, status)] without a
# handle or a plan -- status 1 before a device or any memory is touched, whatever the other arguments say, and 0 for destroying nothing
RNS_OPERATIONS = {
    "basis_extend": {
        "names": {"agx_ntt_basis_create": 6, "agx_ntt_basis_destroy": 1, "agx_ntt_basis_info": 6, "agx_ntt_basis_extend": 6},
        "typedefs": ("agx_ntt_basis",),
        "methods": {"Basis": ("extend", "info", "close"), "Plan": ("basis",)},
        "limits": {"BASIS_MAX_SRC": 16},
        "null_calls": [("agx_ntt_basis_create", (None, None, 0, 1, 0, 1), 1),
                       ("agx_ntt_basis_create", (HANDLE(None), None, 0, 1, 0, 1), 1),      # no plan
                       ("agx_ntt_basis_create", (HANDLE(None), None, 0, 0, 0, 0), 1),      # ... whatever the ranges
                       ("agx_ntt_basis_info", (None, U32, U32, U32, U32, INT), 1), ("agx_ntt_basis_info", (None, None, None, None, None, None), 1),
                       ("agx_ntt_basis_destroy", (None,), 0), ("agx_ntt_basis_destroy", (None,), 0)]
                      + [call for form in (0, 1, 7) for call in (("agx_ntt_basis_extend", (None, BUF(), BUF(), 1, form, None), 1),
                                                                 ("agx_ntt_basis_extend", (None, None, None, 0, form, None), 1))],
    },
    "basis_mod_down": {
        "names": {"agx_ntt_basis_mod_down": 7, "agx_ntt_basis_mod_down_info": 2},
        "typedefs": (),
        "methods": {"Basis": ("mod_down", "mod_down_launches")},
        "limits": {},
        "null_calls": [("agx_ntt_basis_mod_down_info", (None, INT), 1), ("agx_ntt_basis_mod_down_info", (None, None), 1),
                       ("agx_ntt_basis_mod_down", (None, BUF(), BUF(64), BUF(128), BUF(192), 1, None), 1),
                       ("agx_ntt_basis_mod_down", (None, BUF(), BUF(), BUF(), BUF(), 1, None), 1),
                       ("agx_ntt_basis_mod_down", (None, None, None, None, None, 0, None), 1)],
    },
    "inner_product": {
        "names": {"agx_ntt_inner_product": 9},
        "typedefs": (),
        "methods": {"Plan": ("inner_product",)},
        "limits": {"INNER_MAX_TERMS": 16, "INNER_MAX_OUTPUTS": 2},
        "null_calls": [("agx_ntt_inner_product", (None, BUF(), BUF(128), BUF(256), 1, 1, 1, 1, None), 1),
                       ("agx_ntt_inner_product", (None, BUF(), BUF(), BUF(), 1, 1, 2, 2, None), 1),
                       ("agx_ntt_inner_product", (None, BUF(), BUF(128), BUF(256), 1, 1, 0, 3, None), 1),      # the NULL rule comes first
                       ("agx_ntt_inner_product", (None, None, None, None, 0, 0, 0, 0, None), 1)],
    },
    "keyswitch": {
        "names": {"agx_ntt_keyswitch_create": 6, "agx_ntt_keyswitch_destroy": 1, "agx_ntt_keyswitch_info": 7, "agx_ntt_keyswitch_scratch_words": 3,
                  "agx_ntt_keyswitch_apply": 7},
        "typedefs": ("agx_ntt_keyswitch",),
        "methods": {"Plan": ("keyswitch",), "KeySwitch": ("info", "scratch_words", "apply", "close")},
        "limits": {"KEYSWITCH_MAX_DIGITS": 16},
        "null_calls": [("agx_ntt_keyswitch_create", (None, None, 4, 4, 2, 2), 1),
                       ("agx_ntt_keyswitch_create", (HANDLE(0x1234), None, 4, 4, 2, 2), 1),      # the out-pointer is cleared, nothing else
                       ("agx_ntt_keyswitch_destroy", (None,), 0),
                       ("agx_ntt_keyswitch_info", (None, U32, U32, U32, U32, U32, INT), 1),
                       ("agx_ntt_keyswitch_info", (None, None, None, None, None, None, None), 1),
                       ("agx_ntt_keyswitch_scratch_words", (None, 5, U64), 1), ("agx_ntt_keyswitch_scratch_words", (None, 5, None), 1),
                       ("agx_ntt_keyswitch_apply", (None, BUF(), BUF(128), BUF(256), BUF(384), 1, None), 1),
                       ("agx_ntt_keyswitch_apply", (None, BUF(), BUF(), BUF(), BUF(), 1, None), 1),
                       ("agx_ntt_keyswitch_apply", (None, None, None, None, None, 0, None), 1)],
    },
    "hoisted_rotations": {
        "names": {"agx_ntt_inner_product_galois": 10, "agx_ntt_keyswitch_hoisted_words": 5, "agx_ntt_keyswitch_decompose": 6,
                  "agx_ntt_keyswitch_apply_decomposed": 8, "agx_ntt_keyswitch_hoisted_info": 3},
        "typedefs": (),
        "methods": {"Plan": ("inner_product_galois",), "KeySwitch": ("hoisted_words", "decompose", "apply_decomposed", "hoisted_info")},
        "limits": {},
        "null_calls": [("agx_ntt_inner_product_galois", (None, BUF(), BUF(128), BUF(256), 1, 1, 1, 1, 5, None), 1),
                       ("agx_ntt_inner_product_galois", (None, BUF(), BUF(), BUF(), 1, 1, 2, 2, 5, None), 1),
                       # the NULL rule comes first: before the counts and the even element
                       ("agx_ntt_inner_product_galois", (None, BUF(), BUF(128), BUF(256), 1, 1, 0, 3, 4, None), 1),
                       ("agx_ntt_inner_product_galois", (None, None, None, None, 0, 0, 0, 0, 0, None), 1),
                       ("agx_ntt_keyswitch_hoisted_words", (None, 5, U64, U64, U64), 1), ("agx_ntt_keyswitch_hoisted_words", (None, 5, None, None, None), 1),
                       ("agx_ntt_keyswitch_hoisted_info", (None, INT, INT), 1), ("agx_ntt_keyswitch_hoisted_info", (None, None, None), 1),
                       ("agx_ntt_keyswitch_decompose", (None, BUF(), BUF(128), BUF(256), 1, None), 1),
                       ("agx_ntt_keyswitch_decompose", (None, BUF(), BUF(), BUF(), 1, None), 1),
                       ("agx_ntt_keyswitch_decompose", (None, None, None, None, 0, None), 1),
                       ("agx_ntt_keyswitch_apply_decomposed", (None, BUF(), BUF(128), BUF(256), BUF(384), 1, 5, None), 1),
                       ("agx_ntt_keyswitch_apply_decomposed", (None, BUF(), BUF(), BUF(), BUF(), 1, 4, None), 1),      # before the overlap rule and the even element
                       ("agx_ntt_keyswitch_apply_decomposed", (None, None, None, None, None, 0, 0, None), 1)],
    },
}


@pytest.mark.parametrize("op", RNS_OPERATIONS)
def test_rns_symbols_are_declared_exported_and_bound(agx, op):
    text = _header()
    raw = ctypes.CDLL(agx.LIB_PATH)
    for name in RNS_OPERATIONS[op]["names"]:
        assert re.search(r"AGX_API\s+int\s+" + name + r"\s*\(", text), name
        assert hasattr(raw, name), name
        assert name in agx.ABI and agx.ABI[name][0] is ctypes.c_int, name
    for handle in RNS_OPERATIONS[op]["typedefs"]:
        assert re.search(r"typedef\s+struct\s+" + handle + r"\s+" + handle + r"\s*;", text), handle


@pytest.mark.parametrize("op", RNS_OPERATIONS)
def test_rns_argument_counts_match_the_header(agx, op):
    text = _header()
    for name, count in RNS_OPERATIONS[op]["names"].items():
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text).group(1)
        assert len(args.split(",")) == count == len(agx.ABI[name][1]), name


@pytest.mark.parametrize("op", RNS_OPERATIONS)
def test_python_layer_has_the_rns_methods(agx, op):
    for cls, methods in RNS_OPERATIONS[op]["methods"].items():
        assert isinstance(getattr(agx, cls), type), cls
        for method in methods:
            assert callable(getattr(getattr(agx, cls), method)), (cls, method)


@pytest.mark.parametrize("op", [op for op in RNS_OPERATIONS if RNS_OPERATIONS[op]["limits"]])
def test_rns_limits_are_defined_once_and_mirrored(agx, op):
    """AGX_BASIS_MAX_SRC, AGX_INNER_MAX_TERMS / _OUTPUTS, AGX_KEYSWITCH_MAX_DIGITS: one #define each, the same value under the binding's name"""
    for name, value in RNS_OPERATIONS[op]["limits"].items():
        assert re.findall(r"#define\s+AGX_" + name + r"\s+(\d+)\b", _header()) == [str(value)], name
        assert getattr(agx, name) == value, name


def test_no_new_form_or_rescale_constants(agx):
    """agx_ntt_basis_extend's out_form reuses AGX_FORM_COEFF / AGX_FORM_NTT"""
    assert sorted(re.findall(r"#define\s+(AGX_FORM_\w+|AGX_RESCALE_\w+)", _header())) == ["AGX_FORM_COEFF", "AGX_FORM_NTT", "AGX_RESCALE_FLOOR", "AGX_RESCALE_ROUND"]


@pytest.mark.parametrize("op", RNS_OPERATIONS)
def test_rns_call_without_a_handle_says_so_and_touches_nothing(agx, op):
    L = agx.lib()
    buf = (ctypes.c_uint64 * 64)()
    for name, args, status in RNS_OPERATIONS[op]["null_calls"]:
        outs, handles, passed = [], [], []
        for a in args:
            if not isinstance(a, tuple):
                passed.append(a)
            elif a[0] == "buf":
                assert a[1] + 8 <= ctypes.sizeof(buf)
                passed.append(ctypes.addressof(buf) + a[1])
            else:
                box = ctypes.c_void_p(a[1]) if a[0] == "handle" else a[1](7)
                (handles if a[0] == "handle" else outs).append(box)
                passed.append(ctypes.byref(box))
        assert getattr(L, name)(*passed) == status, (name, args)
        assert all(v.value == 7 for v in outs), (name, args, "an out-parameter was written")
        assert all(h.value is None for h in handles), (name, args, "a handle was handed out")
    assert all(w == 0 for w in buf), "a buffer was written"


# prototypes later features promised to leave alone, character for character (whitespace runs of the header count as one blank)
FROZEN_PROTOTYPES = [
    "int agx_ntt_basis_create(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count);",
    "int agx_ntt_basis_destroy(agx_ntt_basis* basis);",
    "int agx_ntt_basis_info(const agx_ntt_basis* basis, uint32_t* src_first, uint32_t* src_count, uint32_t* dst_first, uint32_t* dst_count, int* launches_ntt_form);",
    "int agx_ntt_basis_extend(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream);",
    "int agx_ntt_basis_mod_down(const agx_ntt_basis* basis, const uint64_t* d_xq, const uint64_t* d_xp, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream);",
    "int agx_ntt_basis_mod_down_info(const agx_ntt_basis* basis, int* launches);",
    "int agx_ntt_pointwise(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, void* stream);",
    "int agx_ntt_inner_product(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c, uint64_t batch, uint64_t bhat_batch, uint32_t terms, uint32_t outputs, void* stream);",
    "int agx_ntt_keyswitch_scratch_words(const agx_ntt_keyswitch* ks, uint64_t batch, uint64_t* words);",
    "int agx_ntt_keyswitch_apply(const agx_ntt_keyswitch* ks, const uint64_t* d_chat, const uint64_t* d_keyhat, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream);",
    "int agx_ntt_automorphism(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t galois_elt, int form, void* stream);",
]


@pytest.mark.parametrize("proto", FROZEN_PROTOTYPES, ids=[p.split("(")[0].split()[-1] for p in FROZEN_PROTOTYPES])
def test_frozen_prototype_is_unchanged(proto):
    assert proto in re.sub(r"\s+", " ", _header()), proto


def test_a_plan_cannot_be_made_without_a_device(agx):
    """where no GPU is visible there is no plan to call with: creation reports it instead of handing out something a rescale could run on"""
    if agx.device_count() != 0:
        return
    h = ctypes.c_void_p(None)
    q = (ctypes.c_uint64 * 2)(*agx.find_primes(60, 64, 2))
    assert agx.lib().agx_ntt_plan_create_auto(ctypes.byref(h), 64, 2, q, None) == 6      # AGX_ERR_NO_DEVICE
    assert not h.value


@pytest.mark.parametrize("n", [2, 4, 8, 4096, 32768])
def test_galois_elements_are_powers_of_five(agx, n):
    for step in (0, 1, -1, 7, n // 2, -(n // 2) - 3):
        g = agx.galois_element(n, step)
        assert g == pow(5, step, 2 * n), (n, step)
        assert agx.galois_element(n, -step) == pow(5, -step, 2 * n), (n, -step)
        assert g % 2 == 1 and g < 2 * n
        assert g * agx.galois_element(n, -step) % (2 * n) == 1


def test_galois_element_validates_its_arguments(agx):
    L = agx.lib()
    g = ctypes.c_uint32(0)
    for n in (0, 1, 3, 1000, 65536):
        assert L.agx_ntt_galois_element(n, 1, ctypes.byref(g)) == 2, n
    assert L.agx_ntt_galois_element(4096, 1, None) == 1
    assert L.agx_ntt_galois_element(4096, -(1 << 63), ctypes.byref(g)) == 0 and g.value == pow(5, -(1 << 63), 8192)


def test_library_exports_every_declared_symbol(agx):
    raw = ctypes.CDLL(agx.LIB_PATH)
    for name in _declared_symbols():
        assert hasattr(raw, name), name


def test_library_exports_nothing_but_the_c_abi(agx):
    """built with -fvisibility=hidden and csrc/exports.map: the dynamic symbol table holds the agx_ntt_* entry points only (no
    C++ internals, no kernel host stubs), and exactly the ones the header declares"""
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only", agx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert names == _declared_symbols(), [n for n in names if not n.startswith("agx_ntt_")][:10]


def test_no_torch_or_oracle_in_product_library(agx):
    """the shipped library links neither torch nor the oracle"""
    import subprocess

    needed = subprocess.run(["readelf", "-d", agx.LIB_PATH], capture_output=True, text=True).stdout
    assert "torch" not in needed and "oracle" not in needed
    assert "amdhip64" in needed


def test_release_caches_without_a_device(agx):
    """agx_ntt_release_caches has nothing to free on a box without a GPU and must say so quietly (no HIP call may be required for it)"""
    assert agx.lib().agx_ntt_release_caches() == 0
    assert agx.lib().agx_ntt_release_caches() == 0


def test_strerror(agx):
    L = agx.lib()
    assert L.agx_ntt_strerror(0) == b"success"
    for code in range(1, 10):
        assert L.agx_ntt_strerror(code) not in (b"", b"unknown status")
    assert L.agx_ntt_strerror(1234) == b"unknown status"


@pytest.mark.parametrize("n,bits", [(32, 30), (1024, 30), (4096, 60), (8192, 61), (16384, 60), (32768, 60)])
def test_host_math_matches_oracle(agx, orc, n, bits):
    qs = agx.find_primes(bits, n, 3)
    assert qs == [orc.find_prime(bits, n, k) for k in range(3)]
    q = qs[0]
    psi = agx.min_root(q, n)
    assert psi == orc.min_root(q, n)
    tw, pre = agx.make_tables(q, psi, n)
    otw, opre = orc.make_tables(q, psi, n)
    assert np.array_equal(tw, otw) and np.array_equal(pre, opre)
    itw, ipre = agx.make_tables(q, psi, n, inverse=True)
    oitw, oipre = orc.make_inv_tables(q, psi, n)
    assert np.array_equal(itw, oitw) and np.array_equal(ipre, oipre)


def test_argument_validation(agx):
    L = agx.lib()
    out = np.zeros(4, dtype=np.uint64)
    p64 = ctypes.POINTER(ctypes.c_uint64)
    ptr = out.ctypes.data_as(p64)
    assert L.agx_ntt_find_primes(60, 4096, 1, None) == 1          # NULL
    assert L.agx_ntt_find_primes(60, 1000, 1, ptr) == 2           # not a power of two
    assert L.agx_ntt_find_primes(60, 65536, 1, ptr) == 2          # beyond AGX_NTT_MAX_N
    assert L.agx_ntt_find_primes(63, 4096, 1, ptr) == 5           # q must stay below 2^62
    r = ctypes.c_uint64(0)
    assert L.agx_ntt_min_root(65537, 16384, ctypes.byref(r)) == 0  # the reference's example modulus (main.cpp:55)
    assert L.agx_ntt_min_root(65536, 16, ctypes.byref(r)) == 3     # even
    assert L.agx_ntt_min_root(97, 64, ctypes.byref(r)) == 3        # 96 not divisible by 128
    assert L.agx_ntt_min_root((1 << 62) + 1, 2, ctypes.byref(r)) == 3  # too large
    assert L.agx_ntt_make_tables(97, 5, 16, ptr, ptr) == 4         # 5 is not a primitive 32nd root mod 97
    h = ctypes.c_void_p(None)
    mods = np.array([97], dtype=np.uint64)
    mp = mods.ctypes.data_as(p64)
    assert L.agx_ntt_plan_create_auto(ctypes.byref(h), 24, 1, mp, None) == 2
    assert L.agx_ntt_plan_create_auto(ctypes.byref(h), 16, 0, mp, None) == 5
    assert L.agx_ntt_plan_create_auto(None, 16, 1, mp, None) == 1
    mods[0] = 33  # 1 mod 32 but composite
    assert L.agx_ntt_plan_create_auto(ctypes.byref(h), 16, 1, mp, None) == 3
    assert L.agx_ntt_forward(None, None, None, 1, None) == 1
    assert L.agx_ntt_plan_destroy(None) == 0


def test_product_fails_loudly_without_gpu(agx):
    """there is no CPU fallback behind the boundary: without a device every compute entry
    point reports AGX_ERR_NO_DEVICE"""
    if agx.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(agx.AgxError) as ei:
        agx.Plan(16, [97])
    assert ei.value.status == 6
    q = agx.find_primes(30, 32)[0]
    tw, pre = agx.make_tables(q, agx.min_root(q, 32), 32)
    x = np.zeros(32, dtype=np.uint64)
    with pytest.raises(agx.AgxError) as ei:
        agx.forward_host(x, x, q, tw, pre, 32, 1)
    assert ei.value.status == 6


def test_product_sources_never_reference_the_oracle():
    pkg = os.path.join(ROOT, "agilex-ntt_amd")
    for dirpath, _, files in os.walk(pkg):
        if any(part in ("build", "lib", "bin", "__pycache__") for part in dirpath.split(os.sep)):
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in text.lower(), os.path.join(dirpath, f)


def test_bench_cpu_baseline_leg_runs(orc):
    """bench.py's cpu_baseline leg (the oracle timed on host cores) on a tiny budget"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    os.environ["AGX_BENCH_CPU_THREADS"] = "2"
    try:
        r = bench.cpu_baseline(target_seconds=0.3)
    finally:
        del os.environ["AGX_BENCH_CPU_THREADS"]
    assert r["kind"] == "port" and r["unit"] == "NTT/s" and r["cores"] == 2
    assert r["value"] > 1000 and r["single_core_value"] > 500
    assert bench.host_cores() >= 1


def test_diag_header_declares_only_the_debug_hook():
    """tools/agx_ntt_diag.h (lib/libagxntt_diag.so) adds exactly one symbol to the boundary, and the public header none of it"""
    text = open(os.path.join(ROOT, "tools", "agx_ntt_diag.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(agx_ntt_\w+)\s*\(", text))) == ["agx_ntt_debug_set_trace_buffer"]
    assert "agx_ntt_debug_set_trace_buffer" not in _declared_symbols()


def test_kernel_source_hash_tracks_the_sources(agx, tmp_path):
    """profiles/hbm_traffic.json is tied to the kernel sources by agx.kernel_source_sha16(): stable, 16 hex digits"""
    h = agx.kernel_source_sha16()
    assert re.fullmatch(r"[0-9a-f]{16}", h) and h == agx.kernel_source_sha16()


def test_kernel_source_hash_covers_every_included_device_source(agx):
    """what kernel_source_sha16() hashes is every csrc/*.hip and the closure of their #include "..." lines within csrc/, found here by a walk of its own"""
    csrc = os.path.join(ROOT, "agilex-ntt_amd", "csrc")
    names = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert names
    for name in names:      # grows as it is walked
        for inc in re.findall(r'(?m)^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(os.path.join(csrc, name)).read()):
            if "/" not in inc and os.path.exists(os.path.join(csrc, inc)) and inc not in names:
                names.append(inc)
    assert sorted(os.path.relpath(f, csrc) for f in agx.kernel_source_files()) == sorted(names)
    for header in ("moddown_arith.hpp", "bfv_conv_arith.hpp", "bfv_quotient_arith.hpp", "moddown_coeff_body.hpp", "moddown_rb2_body.hpp",
                   "inner_kernels.hpp", "automorphism_kernels.hpp", "basis_coeff_kernels.hpp", "ring_kernels.hpp", "weighted_kernels.hpp"):
        assert header in names, header
    assert not [n for n in names if n.endswith(".cpp")]


def test_bench_power_sampler_reads_amdgpu_sysfs_layout(tmp_path):
    """bench.py's PowerSampler on a fake amdgpu sysfs tree: microwatts -> watts, the starred pp_dpm_sclk level, window medians"""
    import importlib.util
    import time

    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    hw = tmp_path / "hwmon" / "hwmon3"
    hw.mkdir(parents=True)
    (hw / "power1_average").write_text("1370000000\n")
    (hw / "power1_cap").write_text("1400000000\n")
    (tmp_path / "pp_dpm_sclk").write_text("0: 500Mhz\n1: 1744Mhz *\n2: 2400Mhz\n")
    s = bench.PowerSampler.__new__(bench.PowerSampler)
    s.samples, s.power_file, s.cap_file, s.sclk_file = [], str(hw / "power1_average"), str(hw / "power1_cap"), str(tmp_path / "pp_dpm_sclk")
    t0 = time.perf_counter()
    for _ in range(3):
        s.samples.append((time.perf_counter(),) + s._read())
    w = s.window(t0, time.perf_counter())
    assert w["socket_power_w_median"] == 1370.0 and w["power_cap_w"] == 1400.0 and w["sclk_mhz_median"] == 1744 and w["samples"] == 3
    assert s.window(t0 - 10, t0 - 5) is None
