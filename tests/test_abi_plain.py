"""agx_ntt_plain_* at the C boundary, no device: the six calls are declared AGX_API int with the prototypes stated below, exported and bound; they stand behind
agx_ntt_keyswitch_mod_down and in front of agx_ntt_fill_synthetic; the handle is named by its struct tag and the header adds no constant; Plain and
Plan.plain exist with the signatures stated here; agx_ntt_plain_destroy(NULL) returns 0; and a call without a handle or with a NULL pointer returns
AGX_ERR_NULL_POINTER whatever its other arguments say, writes nothing, and clears a handle out-pointer.  (No plan can be made without a device: the rules
behind the NULL rule are tests/test_gpu_plain.py's.)"""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "agx_ntt_plain_create":
        "int agx_ntt_plain_create(struct agx_ntt_plain** h, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count, uint32_t gamma_prime, uint64_t t);",
    "agx_ntt_plain_destroy": "int agx_ntt_plain_destroy(struct agx_ntt_plain* h);",
    "agx_ntt_plain_info":
        "int agx_ntt_plain_info(const struct agx_ntt_plain* h, uint32_t* q_first, uint32_t* q_count, uint32_t* gamma_prime, uint64_t* t, "
        "int* launches_scale_down, int* launches_ntt_form);",
    "agx_ntt_plain_scale_up":
        "int agx_ntt_plain_scale_up(const struct agx_ntt_plain* h, const uint64_t* d_m, uint64_t* d_out, uint64_t batch, int out_form, void* stream);",
    "agx_ntt_plain_lift":
        "int agx_ntt_plain_lift(const struct agx_ntt_plain* h, const uint64_t* d_m, uint64_t* d_out, uint64_t batch, int out_form, void* stream);",
    "agx_ntt_plain_scale_down":
        "int agx_ntt_plain_scale_down(const struct agx_ntt_plain* h, const uint64_t* d_x, uint64_t* d_m, uint64_t* d_scratch, uint64_t batch, void* stream);",
}
CTYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}
OUT_WORDS = {"agx_ntt_plain_info": ("t",)}      # uint64_t out-parameters: bound by their own width; every other uint64_t pointer is device data


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


def test_where_they_stand_and_what_the_header_adds():
    text = _header()
    at = lambda name: text.index(name + "(")      # noqa: E731
    order = ["agx_ntt_keyswitch_mod_down", "agx_ntt_plain_create", "agx_ntt_plain_destroy", "agx_ntt_plain_info", "agx_ntt_plain_scale_up", "agx_ntt_plain_lift",
             "agx_ntt_plain_scale_down", "agx_ntt_fill_synthetic"]
    assert [at(name) for name in order] == sorted(at(name) for name in order)
    between = text[at("agx_ntt_keyswitch_mod_down"):at("agx_ntt_fill_synthetic")]
    assert re.findall(r"\b(agx_ntt_\w+)\s*\(", between) == order[:-1]      # nothing else in between
    assert re.search(r"^struct agx_ntt_plain;", text, flags=re.M)          # the handle: an opaque struct, named by its tag
    assert sorted(re.findall(r"#define\s+(AGX_FORM_\w+|AGX_RESCALE_\w+)", text)) == ["AGX_FORM_COEFF", "AGX_FORM_NTT", "AGX_RESCALE_FLOOR", "AGX_RESCALE_ROUND"]
    assert not re.findall(r"#define\s+(AGX_PLAIN\w*)", text)


def test_the_python_layer_has_the_class_and_the_methods(agx):
    assert isinstance(agx.Plain, type)
    assert list(inspect.signature(agx.Plain.__init__).parameters) == ["self", "plan", "q_first", "q_count", "gamma_prime", "t"]
    assert list(inspect.signature(agx.Plan.plain).parameters) == ["self", "q_first", "q_count", "gamma_prime", "t"]
    assert list(inspect.signature(agx.Plain.info).parameters) == ["self"]
    for name in ("scale_up", "lift"):
        p = inspect.signature(getattr(agx.Plain, name)).parameters
        assert list(p) == ["self", "d_m", "d_out", "batch", "form", "stream"] and p["form"].default == agx.FORM_NTT and p["stream"].default == 0
    p = inspect.signature(agx.Plain.scale_down).parameters
    assert list(p) == ["self", "d_x", "d_m", "d_scratch", "batch", "stream"] and p["stream"].default == 0
    assert callable(agx.Plain.close)


def test_a_call_without_a_handle_or_a_pointer_says_so_and_touches_nothing(agx):
    L = agx.lib()
    assert L.agx_ntt_plain_destroy(None) == 0 and L.agx_ntt_plain_destroy(None) == 0
    buf = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.addressof(buf) + k      # noqa: E731
    fake = ctypes.addressof(buf)      # stands for a handle where the NULL rule must answer before the handle is read
    for fn in (L.agx_ntt_plain_scale_up, L.agx_ntt_plain_lift):
        for form in (0, 1, 7):      # the NULL rule comes before the form rule
            for args in ((None, at(0), at(64), 1), (None, at(0), at(0), 1), (None, at(4), at(1), (1 << 64) - 1), (None, None, None, 0), (fake, None, at(64), 1),
                         (fake, at(0), None, 1)):
                assert fn(*args, form, None) == 1, (args, form)
    for args in ((None, at(0), at(64), at(128), 1, None), (None, at(0), at(0), at(0), 1, None), (None, at(4), at(1), at(2), (1 << 64) - 1, None),
                 (None, None, None, None, 0, None), (fake, None, at(64), at(128), 1, None), (fake, at(0), None, at(128), 1, None), (fake, at(0), at(64), None, 1, None)):
        assert L.agx_ntt_plain_scale_down(*args) == 1, args
    v = [ctypes.c_uint32(7) for _ in range(3)]
    t, down, ntt = ctypes.c_uint64(77), ctypes.c_int(-5), ctypes.c_int(-5)
    assert L.agx_ntt_plain_info(None, *[ctypes.byref(x) for x in v], ctypes.byref(t), ctypes.byref(down), ctypes.byref(ntt)) == 1
    assert L.agx_ntt_plain_info(None, None, None, None, None, None, None) == 1
    assert [x.value for x in v] == [7, 7, 7] and (t.value, down.value, ntt.value) == (77, -5, -5)
    for t_arg in (0, 1, 65537, (1 << 62), (1 << 64) - 1):      # ... before the range, the auxiliary prime and t
        for gamma in (0, 3, 0xffffffff):
            assert L.agx_ntt_plain_create(None, None, 0, 1, gamma, t_arg) == 1
            for first, count in ((0, 1), (0, 0), (7, 99), (3, 0xffffffff)):
                h = ctypes.c_void_p(0x1234)
                assert L.agx_ntt_plain_create(ctypes.byref(h), None, first, count, gamma, t_arg) == 1 and h.value is None      # the out-pointer is cleared
    assert all(w == 0 for w in buf), "a buffer was written"
    # a wrapper without a handle reports the same status
    plain = agx.Plain.__new__(agx.Plain)
    plain._h = ctypes.c_void_p(None)
    for call in (lambda: plain.scale_up(at(0), at(64), 1), lambda: plain.lift(at(0), at(64), 1, agx.FORM_COEFF), lambda: plain.scale_down(at(0), at(64), at(128), 1),
                 plain.info, lambda: agx.Plain(None, 0, 1, 1, 65537)):
        with pytest.raises(agx.AgxError) as e:
            call()
        assert e.value.status == 1
    assert all(w == 0 for w in buf), "a buffer was written"
