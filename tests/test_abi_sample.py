"""agx_ntt_sample_* at the C boundary, no device: the three calls are declared AGX_API int with the prototypes stated below, exported and bound with matching
argument counts; they stand behind agx_ntt_fill_synthetic; the header adds no AGX_FORM_* and no other constant; Plan has the three methods with the
signatures stated here; and a call without a plan, a key or an output returns AGX_ERR_NULL_POINTER whatever its other arguments say and writes nothing.
(No plan can be made without a device: the rules behind the NULL rule are tests/test_gpu_sample.py's.)"""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "agx_ntt_sample_uniform":
        "int agx_ntt_sample_uniform(const agx_ntt_plan* plan, const uint8_t key[32], uint64_t nonce, uint64_t* d_out, uint64_t batch, uint64_t frame_first, "
        "uint32_t prime_first, uint32_t prime_count, void* stream);",
    "agx_ntt_sample_ternary":
        "int agx_ntt_sample_ternary(const agx_ntt_plan* plan, const uint8_t key[32], uint64_t nonce, uint64_t* d_out, uint64_t batch, uint64_t frame_first, "
        "uint32_t prime_first, uint32_t prime_count, int out_form, void* stream);",
    "agx_ntt_sample_cbd":
        "int agx_ntt_sample_cbd(const agx_ntt_plan* plan, const uint8_t key[32], uint64_t nonce, uint32_t eta, uint64_t* d_out, uint64_t batch, "
        "uint64_t frame_first, uint32_t prime_first, uint32_t prime_count, int out_form, void* stream);",
}
CTYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}


def _header():
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _bound(arg):
    """every pointer (the key's array parameter is one) a void pointer, every scalar bound by its own width"""
    return ctypes.c_void_p if "*" in arg or "[" in arg else CTYPES[arg.split()[0]]


@pytest.mark.parametrize("name", PROTOTYPES)
def test_symbol_is_declared_exported_and_bound(agx, name):
    flat = re.sub(r"\s+", " ", _header())
    assert "AGX_API " + PROTOTYPES[name] in flat, name
    assert hasattr(ctypes.CDLL(agx.LIB_PATH), name), name
    restype, argtypes = agx.ABI[name]
    assert restype is ctypes.c_int
    declared = [a.strip() for a in PROTOTYPES[name].split("(", 1)[1].rsplit(")", 1)[0].split(",")]
    want = [_bound(a) for a in declared]
    assert len(argtypes) == len(declared) and argtypes == want, (name, declared)
    assert getattr(agx.lib(), name).argtypes == want


def test_where_they_stand_and_what_the_header_adds():
    text = _header()
    at = lambda name: text.index(name + "(")      # noqa: E731
    order = ["agx_ntt_fill_synthetic", "agx_ntt_sample_uniform", "agx_ntt_sample_ternary", "agx_ntt_sample_cbd", "agx_ntt_find_primes"]
    assert [at(name) for name in order] == sorted(at(name) for name in order)
    between = text[at("agx_ntt_fill_synthetic"):at("agx_ntt_find_primes")]
    assert re.findall(r"\b(agx_ntt_\w+)\s*\(", between) == order[:-1]      # nothing else in between
    assert sorted(re.findall(r"#define\s+(AGX_FORM_\w+|AGX_RESCALE_\w+)", text)) == ["AGX_FORM_COEFF", "AGX_FORM_NTT", "AGX_RESCALE_FLOOR", "AGX_RESCALE_ROUND"]
    assert not re.findall(r"#define\s+(AGX_SAMPLE\w*)", text) and not re.findall(r"typedef struct\s+(agx_ntt_sample\w*)", text)      # stateless: no handle


def test_the_python_layer_has_the_methods(agx):
    tail = ["d_out", "batch", "frame_first", "prime_first", "prime_count"]
    p = inspect.signature(agx.Plan.sample_uniform).parameters
    assert list(p) == ["self", "key", "nonce", *tail, "stream"]
    assert (p["frame_first"].default, p["prime_first"].default, p["prime_count"].default, p["stream"].default) == (0, 0, None, 0)
    for name, head in (("sample_ternary", ["self", "key", "nonce"]), ("sample_cbd", ["self", "key", "nonce", "eta"])):
        p = inspect.signature(getattr(agx.Plan, name)).parameters
        assert list(p) == [*head, *tail, "form", "stream"] and p["form"].default == agx.FORM_NTT and p["stream"].default == 0
    assert not hasattr(agx.DeviceGroup, "sample_uniform")      # no group form, as for a basis


def test_a_call_without_a_plan_a_key_or_an_output_says_so_and_touches_nothing(agx):
    L = agx.lib()
    buf = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.addressof(buf) + k      # noqa: E731
    fake = ctypes.addressof(buf)      # stands for a plan where the NULL rule must answer before the plan is read
    key = bytes(range(32))
    triples = ((None, key, at(0)), (None, None, None), (fake, None, at(0)), (fake, key, None), (None, key, at(4)), (fake, None, None))
    shapes = ((1, 0, 0, 1), (0, 0, 0, 0), ((1 << 64) - 1, (1 << 64) - 1, 7, 0xffffffff), (5, 1 << 32, 3, 0))      # batch, frame_first, prime_first, prime_count
    for plan, k, out in triples:
        for shape in shapes:
            for nonce in (0, (1 << 64) - 1):
                assert L.agx_ntt_sample_uniform(plan, k, nonce, out, *shape, None) == 1, (plan, k, out, shape)
                for form in (0, 1, 7):      # the NULL rule comes before the form and eta rules
                    assert L.agx_ntt_sample_ternary(plan, k, nonce, out, *shape, form, None) == 1
                    for eta in (0, 1, 21, 32, 33):
                        assert L.agx_ntt_sample_cbd(plan, k, nonce, eta, out, *shape, form, None) == 1
    assert all(w == 0 for w in buf), "a buffer was written"
    # a wrapper without a plan reports the same status; a key of another length never reaches the library
    plan = agx.Plan.__new__(agx.Plan)
    plan._h, plan.moduli = ctypes.c_void_p(None), [17]
    for call in (lambda: plan.sample_uniform(key, 0, at(0), 1), lambda: plan.sample_ternary(key, 0, at(0), 1, form=agx.FORM_COEFF),
                 lambda: plan.sample_cbd(key, 0, 21, at(0), 1), lambda: plan.sample_uniform(None, 0, at(0), 1)):
        with pytest.raises(agx.AgxError) as e:
            call()
        assert e.value.status == 1
    with pytest.raises(ValueError):
        plan.sample_uniform(key[:31], 0, at(0), 1)
    assert all(w == 0 for w in buf), "a buffer was written"
