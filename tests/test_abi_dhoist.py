"""The double-hoisting calls at the C boundary, no device: agx_ntt_keyswitch_accumulate_decomposed, agx_ntt_keyswitch_mod_down and agx_ntt_mul_add_galois
are declared AGX_API int with the prototypes stated below, exported and bound; KeySwitch and Plan have the methods with their defaults; and a call
without a handle returns AGX_ERR_NULL_POINTER whatever its other arguments say -- before weight_batch, accumulate, the overlap rule, the prime range and the
Galois element are looked at -- and writes nothing.  (No plan can be made without a device: the rules behind the NULL rule are tests/test_gpu_dhoist.py's.)"""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "agx_ntt_keyswitch_accumulate_decomposed":
        "int agx_ntt_keyswitch_accumulate_decomposed(const agx_ntt_keyswitch* ks, const uint64_t* d_ext, const uint64_t* d_keyhat, const uint64_t* d_weight, "
        "uint64_t weight_batch, uint64_t* d_acc, uint64_t batch, uint32_t galois_elt, int accumulate, void* stream);",
    "agx_ntt_keyswitch_mod_down": "int agx_ntt_keyswitch_mod_down(const agx_ntt_keyswitch* ks, uint64_t* d_acc, uint64_t* d_out, uint64_t batch, void* stream);",
    "agx_ntt_mul_add_galois":
        "int agx_ntt_mul_add_galois(const agx_ntt_plan* plan, const uint64_t* d_w, uint64_t w_batch, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, "
        "uint32_t prime_first, uint32_t prime_count, uint32_t galois_elt, int accumulate, void* stream);",
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
    # every pointer is bound as a void pointer, every scalar by its own width
    declared = [a.strip() for a in PROTOTYPES[name].split("(", 1)[1].rsplit(")", 1)[0].split(",")]
    want = [ctypes.c_void_p if "*" in a else CTYPES[a.split()[0]] for a in declared]
    assert argtypes == want, (name, declared)
    assert getattr(agx.lib(), name).argtypes == want


def test_they_stand_behind_the_calls_they_split_and_extend():
    text = _header()
    at = lambda name: text.index(name + "(")      # noqa: E731
    assert at("agx_ntt_tensor") < at("agx_ntt_mul_add_galois") < at("agx_ntt_keyswitch_create")
    assert at("agx_ntt_keyswitch_hoisted_info") < at("agx_ntt_keyswitch_accumulate_decomposed") < at("agx_ntt_keyswitch_mod_down") < at("agx_ntt_fill_synthetic")
    assert sorted(re.findall(r"typedef\s+struct\s+(\w+)", text)) == ["agx_ntt_basis", "agx_ntt_group", "agx_ntt_keyswitch", "agx_ntt_plan"]      # no new handle


def test_the_python_layer_has_the_methods_with_their_defaults(agx):
    p = inspect.signature(agx.KeySwitch.accumulate_decomposed).parameters
    assert list(p) == ["self", "d_ext", "d_keyhat", "d_acc", "batch", "galois_elt", "d_weight", "weight_batch", "accumulate", "stream"]
    assert (p["d_weight"].default, p["weight_batch"].default, p["accumulate"].default, p["stream"].default) == (None, None, False, 0)
    p = inspect.signature(agx.KeySwitch.mod_down).parameters
    assert list(p) == ["self", "d_acc", "d_out", "batch", "stream"] and p["stream"].default == 0
    p = inspect.signature(agx.Plan.mul_add_galois).parameters
    assert list(p) == ["self", "d_w", "d_b", "d_c", "batch", "galois_elt", "w_batch", "accumulate", "prime_first", "prime_count", "stream"]
    assert [p[k].default for k in ("galois_elt", "w_batch", "accumulate", "prime_first", "prime_count", "stream")] == [1, None, False, 0, None, 0]


def test_a_call_without_a_handle_says_so_and_touches_nothing(agx):
    L = agx.lib()
    buf = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.addressof(buf) + k      # noqa: E731
    A, M, G = "agx_ntt_keyswitch_accumulate_decomposed", "agx_ntt_keyswitch_mod_down", "agx_ntt_mul_add_galois"
    calls = [
        (A, (None, at(0), at(128), at(256), 1, at(384), 1, 5, 0, None)),
        (A, (None, at(0), at(128), None, 0, at(384), 1, 5, 1, None)),                # no weight
        (A, (None, at(0), at(128), at(256), 7, at(384), 3, 5, 0, None)),             # weight_batch neither batch nor 1: the NULL rule comes first
        (A, (None, at(0), at(128), at(256), 1, at(384), 1, 5, 2, None)),             # accumulate = 2
        (A, (None, at(0), at(0), at(0), 1, at(0), 1, 4, -1, None)),                  # everything on one address, an even element
        (A, (None, at(4), at(1), at(2), 1, at(3), 1 << 63, 0, 0, None)),             # misaligned, a batch past every limit
        (A, (None, None, None, None, 0, None, 0, 0, 0, None)),
        (M, (None, at(0), at(256), 1, None)),
        (M, (None, at(0), at(0), 1, None)),                                          # acc on out
        (M, (None, at(4), at(1), (1 << 64) - 1, None)),
        (M, (None, None, None, 0, None)),
        (G, (None, at(0), 1, at(128), at(256), 1, 0, 1, 5, 0, None)),
        (G, (None, at(0), 3, at(128), at(256), 2, 0, 1, 5, 0, None)),                # w_batch neither batch nor 1
        (G, (None, at(0), 1, at(128), at(256), 1, 0, 0, 4, 7, None)),                # prime_count = 0, an even element, accumulate = 7
        (G, (None, at(0), 1, at(0), at(0), 1, 7, 0xffffffff, 0, 1, None)),           # c on w and b, a range that would wrap
        (G, (None, None, 0, None, None, 0, 0, 0, 0, 0, None)),
    ]
    for name, args in calls:
        assert getattr(L, name)(*args) == 1, (name, args)
    assert all(w == 0 for w in buf), "a buffer was written"
    # a wrapper without a handle reports the same status
    ks = agx.KeySwitch.__new__(agx.KeySwitch)
    ks._h = ctypes.c_void_p(None)
    for call in (lambda: ks.accumulate_decomposed(at(0), at(128), at(256), 1, 5), lambda: ks.mod_down(at(0), at(256), 1)):
        with pytest.raises(agx.AgxError) as e:
            call()
        assert e.value.status == 1
    assert all(w == 0 for w in buf), "a buffer was written"
