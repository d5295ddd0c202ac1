"""CPU tests of the boundary of the hoisted rotations: agx_ntt_inner_product_galois and the four agx_ntt_keyswitch_* calls of the two halves are
declared by include/agx_ntt.h, exported by the library and bound by the Python layer with the header's argument counts; without a plan or a handle
each says so (status 1) before it touches a device or any memory; agx_ntt_keyswitch_apply and agx_ntt_inner_product keep their prototypes."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {"agx_ntt_inner_product_galois": 10, "agx_ntt_keyswitch_hoisted_words": 5, "agx_ntt_keyswitch_decompose": 6,
        "agx_ntt_keyswitch_apply_decomposed": 8, "agx_ntt_keyswitch_hoisted_info": 3}


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


def test_argument_counts_match_the_header(agx):
    text = _header()
    for name, count in WANT.items():
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text).group(1)
        assert len(args.split(",")) == count == len(agx.ABI[name][1]), name


def test_python_layer_has_the_methods(agx):
    assert callable(agx.Plan.inner_product_galois)
    for method in ("hoisted_words", "decompose", "apply_decomposed", "hoisted_info"):
        assert callable(getattr(agx.KeySwitch, method)), method


def test_the_one_call_prototypes_are_unchanged(agx):
    text = re.sub(r"\s+", " ", _header())
    for proto in ("int agx_ntt_inner_product(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c, uint64_t batch, uint64_t bhat_batch, uint32_t terms, uint32_t outputs, void* stream);",
                  "int agx_ntt_keyswitch_scratch_words(const agx_ntt_keyswitch* ks, uint64_t batch, uint64_t* words);",
                  "int agx_ntt_keyswitch_apply(const agx_ntt_keyswitch* ks, const uint64_t* d_chat, const uint64_t* d_keyhat, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream);",
                  "int agx_ntt_automorphism(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t galois_elt, int form, void* stream);"):
        assert proto in text, proto


def test_null_plan_or_handle_is_status_1_and_touches_nothing(agx):
    L = agx.lib()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    G = L.agx_ntt_inner_product_galois
    assert G(None, p, p + 128, p + 256, 1, 1, 1, 1, 5, None) == 1
    assert G(None, p, p, p, 1, 1, 2, 2, 5, None) == 1
    assert G(None, p, p + 128, p + 256, 1, 1, 0, 3, 4, None) == 1      # the NULL rule comes first: before the counts and the even element
    assert G(None, None, None, None, 0, 0, 0, 0, 0, None) == 1
    words = [ctypes.c_uint64(7) for _ in range(3)]
    assert L.agx_ntt_keyswitch_hoisted_words(None, 5, *[ctypes.byref(w) for w in words]) == 1 and all(w.value == 7 for w in words)
    assert L.agx_ntt_keyswitch_hoisted_words(None, 5, None, None, None) == 1
    counts = [ctypes.c_int(7), ctypes.c_int(7)]
    assert L.agx_ntt_keyswitch_hoisted_info(None, ctypes.byref(counts[0]), ctypes.byref(counts[1])) == 1 and all(c.value == 7 for c in counts)
    assert L.agx_ntt_keyswitch_hoisted_info(None, None, None) == 1
    D, A = L.agx_ntt_keyswitch_decompose, L.agx_ntt_keyswitch_apply_decomposed
    assert D(None, p, p + 128, p + 256, 1, None) == 1
    assert D(None, p, p, p, 1, None) == 1
    assert D(None, None, None, None, 0, None) == 1
    assert A(None, p, p + 128, p + 256, p + 384, 1, 5, None) == 1
    assert A(None, p, p, p, p, 1, 4, None) == 1      # before the overlap rule and the even element
    assert A(None, None, None, None, None, 0, 0, None) == 1
    assert all(w == 0 for w in buf)
