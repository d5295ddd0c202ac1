"""agx_ntt_ckks_* at the C boundary, no device: the six calls are declared AGX_API int with the prototypes stated below, exported and bound (scale as a
c_double); they stand behind agx_ntt_galois_element and in front of the groups; the handle is named by its struct tag and the header adds no constant; Ckks,
Plan.ckks and ckks_twiddle exist with the signatures stated here; agx_ntt_ckks_destroy(NULL) returns 0; a call without a handle or with a NULL pointer returns
AGX_ERR_NULL_POINTER whatever its other arguments say, writes nothing, and clears a handle out-pointer; agx_ntt_ckks_twiddle validates its arguments.  (No plan
can be made without a device: the rules behind the NULL rule are tests/test_gpu_ckks.py's.)"""
import ctypes
import inspect
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "agx_ntt_ckks_create": "int agx_ntt_ckks_create(struct agx_ntt_ckks** h, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count);",
    "agx_ntt_ckks_destroy": "int agx_ntt_ckks_destroy(struct agx_ntt_ckks* h);",
    "agx_ntt_ckks_info":
        "int agx_ntt_ckks_info(const struct agx_ntt_ckks* h, uint32_t* q_first, uint32_t* q_count, uint32_t* max_slots, int* launches_encode_ntt, "
        "int* launches_decode_ntt);",
    "agx_ntt_ckks_encode":
        "int agx_ntt_ckks_encode(const struct agx_ntt_ckks* h, const double* d_z, uint32_t slots, double scale, uint64_t* d_out, uint64_t batch, uint32_t count, "
        "int out_form, void* stream);",
    "agx_ntt_ckks_decode":
        "int agx_ntt_ckks_decode(const struct agx_ntt_ckks* h, const uint64_t* d_x, int in_form, uint32_t count, double scale, double* d_z, uint32_t slots, "
        "uint64_t* d_scratch, uint64_t batch, void* stream);",
    "agx_ntt_ckks_twiddle": "int agx_ntt_ckks_twiddle(uint32_t len, uint32_t j, double out[2]);",
}
CTYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int, "double": ctypes.c_double}


def _header():
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _bound(name, arg):
    """a handle out-pointer is a pointer to a void pointer, an int or uint32_t out-pointer and the twiddle's host array a pointer to its own width, every other
    pointer (device data) a void pointer, every scalar bound by its own width"""
    if "**" in arg:
        return ctypes.POINTER(ctypes.c_void_p)
    if arg.endswith("[2]"):
        return ctypes.POINTER(CTYPES[arg.split()[0]])
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
    want = [_bound(name, a) for a in declared]
    assert argtypes == want, (name, declared)
    assert getattr(agx.lib(), name).argtypes == want


def test_where_they_stand_and_what_the_header_adds():
    text = _header()
    at = lambda name: text.index(name + "(")      # noqa: E731
    order = ["agx_ntt_galois_element", "agx_ntt_ckks_create", "agx_ntt_ckks_destroy", "agx_ntt_ckks_info", "agx_ntt_ckks_encode", "agx_ntt_ckks_decode",
             "agx_ntt_ckks_twiddle", "agx_ntt_shard_range"]
    assert [at(name) for name in order] == sorted(at(name) for name in order)
    between = text[at("agx_ntt_galois_element"):at("agx_ntt_shard_range")]
    assert re.findall(r"\b(agx_ntt_\w+)\s*\(", between) == order[:-1]      # nothing else in between
    assert re.search(r"^struct agx_ntt_ckks;", text, flags=re.M)           # the handle: an opaque struct, named by its tag
    assert sorted(re.findall(r"#define\s+(AGX_FORM_\w+|AGX_RESCALE_\w+)", text)) == ["AGX_FORM_COEFF", "AGX_FORM_NTT", "AGX_RESCALE_FLOOR", "AGX_RESCALE_ROUND"]
    assert not re.findall(r"#define\s+(AGX_CKKS\w*)", text)
    assert "CKKS decoding" not in open(os.path.join(ROOT, "include", "agx_ntt.h")).read()      # no longer out of scope


def test_the_python_layer_has_the_class_and_the_methods(agx):
    assert isinstance(agx.Ckks, type)
    assert list(inspect.signature(agx.Ckks.__init__).parameters) == ["self", "plan", "q_first", "q_count"]
    assert list(inspect.signature(agx.Plan.ckks).parameters) == ["self", "q_first", "q_count"]
    assert list(inspect.signature(agx.Ckks.info).parameters) == ["self"]
    p = inspect.signature(agx.Ckks.encode).parameters
    assert list(p) == ["self", "d_z", "slots", "scale", "d_out", "batch", "count", "form", "stream"] and p["form"].default == agx.FORM_NTT and p["stream"].default == 0
    p = inspect.signature(agx.Ckks.decode).parameters
    assert list(p) == ["self", "d_x", "form", "count", "scale", "d_z", "slots", "d_scratch", "batch", "stream"] and p["stream"].default == 0
    assert callable(agx.Ckks.close) and list(inspect.signature(agx.ckks_twiddle).parameters) == ["length", "j"]


def test_a_call_without_a_handle_or_a_pointer_says_so_and_touches_nothing(agx):
    L = agx.lib()
    assert L.agx_ntt_ckks_destroy(None) == 0 and L.agx_ntt_ckks_destroy(None) == 0
    buf = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.addressof(buf) + k      # noqa: E731
    fake = ctypes.addressof(buf)      # stands for a handle where the NULL rule must answer before the handle is read
    for form in (0, 1, 7):      # the NULL rule comes before every other rule
        for slots, scale, count in ((1, 1.0, 1), (3, -1.0, 0), (0, math.nan, 99)):
            for h, z, out in ((None, at(0), at(64)), (None, at(0), at(0)), (None, at(4), at(1)), (None, None, None), (fake, None, at(64)), (fake, at(0), None)):
                assert L.agx_ntt_ckks_encode(h, z, slots, scale, out, 1, count, form, None) == 1, (h, z, out, form)
            for h, x, z, scr in ((None, at(0), at(64), at(128)), (None, at(0), at(0), at(0)), (None, None, None, None), (fake, None, at(64), at(128)),
                                 (fake, at(0), None, at(128))):
                assert L.agx_ntt_ckks_decode(h, x, form, count, scale, z, slots, scr, 1, None) == 1, (h, x, z, scr, form)
    assert L.agx_ntt_ckks_decode(fake, at(0), 1, 1, 1.0, at(64), 1, None, 1, None) == 1      # NTT form needs its scratch
    v = [ctypes.c_uint32(7) for _ in range(3)]
    enc, dec = ctypes.c_int(-5), ctypes.c_int(-5)
    assert L.agx_ntt_ckks_info(None, *[ctypes.byref(x) for x in v], ctypes.byref(enc), ctypes.byref(dec)) == 1
    assert L.agx_ntt_ckks_info(None, None, None, None, None, None) == 1
    assert [x.value for x in v] == [7, 7, 7] and (enc.value, dec.value) == (-5, -5)
    assert L.agx_ntt_ckks_create(None, None, 0, 1) == 1
    for first, count in ((0, 1), (0, 0), (7, 99), (3, 0xffffffff)):      # ... before the range
        h = ctypes.c_void_p(0x1234)
        assert L.agx_ntt_ckks_create(ctypes.byref(h), None, first, count) == 1 and h.value is None      # the out-pointer is cleared
    assert all(w == 0 for w in buf), "a buffer was written"
    ck = agx.Ckks.__new__(agx.Ckks)      # a wrapper without a handle reports the same status
    ck._h = ctypes.c_void_p(None)
    for call in (lambda: ck.encode(at(0), 1, 1.0, at(64), 1, 1), lambda: ck.decode(at(0), agx.FORM_COEFF, 1, 1.0, at(64), 1, None, 1), ck.info,
                 lambda: agx.Ckks(None, 0, 1)):
        with pytest.raises(agx.AgxError) as e:
            call()
        assert e.value.status == 1
    assert all(w == 0 for w in buf), "a buffer was written"


def test_twiddle_validates_and_is_a_point_of_the_circle(agx):
    L = agx.lib()
    out = (ctypes.c_double * 2)(7.0, 7.0)
    assert L.agx_ntt_ckks_twiddle(2, 0, None) == 1
    for length, j in ((0, 0), (1, 0), (3, 0), (6, 1), (2, 1), (8, 4), (16384, 8192), (32768, 0), (1 << 31, 0), (4, 0xffffffff)):
        assert L.agx_ntt_ckks_twiddle(length, j, out) == 5, (length, j)
        assert (out[0], out[1]) == (7.0, 7.0)
    assert L.agx_ntt_ckks_twiddle(16384, 8191, out) == 0 and abs(math.hypot(out[0], out[1]) - 1) < 4e-16
    c, s = agx.ckks_twiddle(2, 0)      # theta = 2 pi / 8
    assert c == s == math.sqrt(0.5)
    c, s = agx.ckks_twiddle(4, 1)      # theta = 2 pi 5 / 16
    assert abs(c - math.cos(5 * math.pi / 8)) < 2 ** -52 and abs(s - math.sin(5 * math.pi / 8)) < 2 ** -52
    with pytest.raises(agx.AgxError) as e:
        agx.ckks_twiddle(4, 2)
    assert e.value.status == 5
