"""agx_ntt_batch_* and agx_ntt_plain_reduce at the C boundary, no device: the seven calls are declared AGX_API int with the prototypes stated below, exported
and bound; they stand behind agx_ntt_group_synchronize, the last declarations of the header; the batching handle is named by its struct tag and the header
adds no constant; Batch and Plain.reduce exist with the signatures stated here; agx_ntt_batch_destroy(NULL) returns 0; a call without a handle or with a NULL
pointer returns AGX_ERR_NULL_POINTER whatever its other arguments say, writes nothing, and create clears its out-pointer; create judges n and t before any
device is needed.  The three "BGV decryption is out of scope" remarks are gone.  (The rules behind these are tests/test_gpu_batch.py's.)"""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "agx_ntt_batch_create": "int agx_ntt_batch_create(struct agx_ntt_batch** h, uint32_t n, uint64_t t);",
    "agx_ntt_batch_destroy": "int agx_ntt_batch_destroy(struct agx_ntt_batch* h);",
    "agx_ntt_batch_info":
        "int agx_ntt_batch_info(const struct agx_ntt_batch* h, uint32_t* n, uint64_t* t, uint64_t* psi, int* launches_encode, int* launches_decode);",
    "agx_ntt_batch_plan": "int agx_ntt_batch_plan(const struct agx_ntt_batch* h, agx_ntt_plan** plan);",
    "agx_ntt_batch_encode": "int agx_ntt_batch_encode(const struct agx_ntt_batch* h, const uint64_t* d_z, uint64_t* d_m, uint64_t batch, void* stream);",
    "agx_ntt_batch_decode":
        "int agx_ntt_batch_decode(const struct agx_ntt_batch* h, const uint64_t* d_m, uint64_t* d_z, uint64_t* d_scratch, uint64_t batch, void* stream);",
    "agx_ntt_plain_reduce":
        "int agx_ntt_plain_reduce(const struct agx_ntt_plain* h, const uint64_t* d_x, uint64_t* d_m, uint64_t* d_scratch, uint64_t factor, uint64_t batch, "
        "void* stream);",
}
CTYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}
HOST_OUT = {"n", "t", "psi", "launches_encode", "launches_decode"}      # info's out-pointers: host memory, bound by their own width


def _header():
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _bound(arg):
    """a handle out-pointer is a pointer to a void pointer, a host out-pointer a pointer to its own width, every other pointer (a handle, device data, the
    stream) a void pointer, every scalar bound by its own width"""
    if "**" in arg:
        return ctypes.POINTER(ctypes.c_void_p)
    if "*" in arg:
        base, name = arg.replace("const ", "").split("*")[0].strip(), arg.split("*")[-1].strip()
        return ctypes.POINTER(CTYPES[base]) if name in HOST_OUT else ctypes.c_void_p
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


def test_where_they_stand_and_what_the_header_adds():
    text = _header()
    at = lambda name: text.index(name + "(")      # noqa: E731
    order = ["agx_ntt_group_synchronize"] + list(PROTOTYPES)
    assert [at(name) for name in order] == sorted(at(name) for name in order)
    behind = text[at("agx_ntt_group_synchronize"):]
    assert re.findall(r"\b(agx_ntt_\w+)\s*\(", behind) == order      # nothing else behind the groups: the closed blocks stay closed
    assert re.search(r"^struct agx_ntt_batch;", text, flags=re.M)      # the handle: an opaque struct, named by its tag
    assert "agx_ntt_batch" not in " ".join(re.findall(r"typedef struct \w+ \w+;", text))
    assert not re.findall(r"#define\s+(AGX_BATCH\w*|AGX_BGV\w*)", text)
    assert sorted(re.findall(r"#define\s+(AGX_FORM_\w+|AGX_RESCALE_\w+)", text)) == ["AGX_FORM_COEFF", "AGX_FORM_NTT", "AGX_RESCALE_FLOOR", "AGX_RESCALE_ROUND"]
    for doc in (os.path.join("include", "agx_ntt.h"), "INTEGRATION.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert not re.search(r"Out of scope:[^.]*BGV decryption", body), doc      # no longer out of scope


def test_the_python_layer_has_the_class_and_the_methods(agx):
    assert isinstance(agx.Batch, type)
    assert list(inspect.signature(agx.Batch.__init__).parameters) == ["self", "n", "t"]
    assert list(inspect.signature(agx.Batch.info).parameters) == ["self"] and list(inspect.signature(agx.Batch.plan).parameters) == ["self"]
    p = inspect.signature(agx.Batch.encode).parameters
    assert list(p) == ["self", "d_z", "d_m", "batch", "stream"] and p["stream"].default == 0
    p = inspect.signature(agx.Batch.decode).parameters
    assert list(p) == ["self", "d_m", "d_z", "d_scratch", "batch", "stream"] and p["stream"].default == 0
    p = inspect.signature(agx.Plain.reduce).parameters
    assert list(p) == ["self", "d_x", "d_m", "d_scratch", "batch", "factor", "stream"] and p["factor"].default == 1 and p["stream"].default == 0
    assert callable(agx.Batch.close)


def test_a_call_without_a_handle_or_a_pointer_says_so_and_touches_nothing(agx):
    L = agx.lib()
    assert L.agx_ntt_batch_destroy(None) == 0 and L.agx_ntt_batch_destroy(None) == 0
    buf = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.addressof(buf) + k      # noqa: E731
    fake = ctypes.addressof(buf)      # stands for a handle where the NULL rule must answer before the handle is read
    for batch in (1, 0, 1 << 63):      # the NULL rule comes before every other rule
        for h, z, m in ((None, at(0), at(64)), (None, at(0), at(0)), (None, at(4), at(1)), (None, None, None), (fake, None, at(64)), (fake, at(0), None)):
            assert L.agx_ntt_batch_encode(h, z, m, batch, None) == 1, (h, z, m, batch)
        for h, m, z, scr in ((None, at(0), at(64), at(128)), (None, at(0), at(0), at(0)), (None, None, None, None), (fake, None, at(64), at(128)),
                             (fake, at(0), None, at(128)), (fake, at(0), at(64), None)):
            assert L.agx_ntt_batch_decode(h, m, z, scr, batch, None) == 1, (h, m, z, scr, batch)
            for factor in (1, 0, (1 << 64) - 1):
                assert L.agx_ntt_plain_reduce(h, m, z, scr, factor, batch, None) == 1, (h, m, z, scr, factor, batch)
    n, enc, dec = ctypes.c_uint32(7), ctypes.c_int(-5), ctypes.c_int(-5)
    t, psi = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.agx_ntt_batch_info(None, ctypes.byref(n), ctypes.byref(t), ctypes.byref(psi), ctypes.byref(enc), ctypes.byref(dec)) == 1
    assert L.agx_ntt_batch_info(None, None, None, None, None, None) == 1
    assert (n.value, t.value, psi.value, enc.value, dec.value) == (7, 7, 7, -5, -5)
    plan = ctypes.c_void_p(0x1234)
    assert L.agx_ntt_batch_plan(None, ctypes.byref(plan)) == 1 and plan.value == 0x1234
    assert L.agx_ntt_batch_plan(fake, None) == 1 and L.agx_ntt_batch_plan(None, None) == 1
    assert L.agx_ntt_batch_create(None, 64, 257) == 1 and L.agx_ntt_batch_create(None, 0, 0) == 1      # ... before the size and the modulus
    assert all(w == 0 for w in buf), "a buffer was written"
    b = agx.Batch.__new__(agx.Batch)      # a wrapper without a handle reports the same status
    b._h = ctypes.c_void_p(None)
    p = agx.Plain.__new__(agx.Plain)
    p._h = ctypes.c_void_p(None)
    for call in (lambda: b.encode(at(0), at(64), 1), lambda: b.decode(at(0), at(64), at(128), 1), b.info, b.plan, lambda: p.reduce(at(0), at(64), at(128), 1)):
        with pytest.raises(agx.AgxError) as e:
            call()
        assert e.value.status == 1
    assert all(w == 0 for w in buf), "a buffer was written"


def test_create_judges_the_size_and_the_modulus_before_it_needs_a_device(agx):
    L = agx.lib()
    bad_argument, bad_modulus = 5, L.agx_ntt_min_root(15, 2, ctypes.byref(ctypes.c_uint64(0)))      # a composite modulus: AGX_ERR_BAD_MODULUS, as min_root says it
    assert bad_modulus not in (0, 1, bad_argument)
    for n in (0, 1, 3, 48, 65536, 1 << 31):      # not a size the plans admit
        h = ctypes.c_void_p(0x1234)
        assert L.agx_ntt_batch_create(ctypes.byref(h), n, 65537) == bad_argument and h.value is None, n
    for n, t in ((64, 129), (64, 385), (64, 256), (64, 0), (64, 1), (64, 2), (64, 193), (4096, 257), (2, 9), (8, 17 * 97),
                 (64, (1 << 62) + 129), (64, (1 << 64) - 127), (2, 1 << 62)):
        # composite (129 = 3 43, 385 = 5 7 11, 9, 17 97 = 1 mod 16), not 1 modulo 2n (256, 193, 257 at n = 4096), too small, at or above 2^62
        h = ctypes.c_void_p(0x1234)
        assert L.agx_ntt_batch_create(ctypes.byref(h), n, t) == bad_modulus and h.value is None, (n, t)
    with pytest.raises(agx.AgxError) as e:
        agx.Batch(64, 129)
    assert e.value.status == bad_modulus
