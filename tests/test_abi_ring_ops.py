"""The ring calls at the C boundary, no device: agx_ntt_add, _sub, _negate, _add_galois and _tensor are declared AGX_API int with the argument counts
the issue fixed, exported and bound; Plan has the five methods; and a call without a plan returns AGX_ERR_NULL_POINTER whatever its other arguments
say -- before the prime range and the Galois element are looked at -- and writes nothing."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {"agx_ntt_add": 8, "agx_ntt_sub": 8, "agx_ntt_negate": 7, "agx_ntt_add_galois": 9, "agx_ntt_tensor": 8}
METHODS = ("add", "sub", "negate", "add_galois", "tensor")


def _header():
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_declared_exported_and_bound(agx, name):
    text = _header()
    assert re.search(r"AGX_API\s+int\s+" + name + r"\s*\(", text), name
    args = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text).group(1)
    assert len(args.split(",")) == NAMES[name] == len(agx.ABI[name][1]), name
    assert agx.ABI[name][0] is ctypes.c_int
    assert hasattr(ctypes.CDLL(agx.LIB_PATH), name), name
    # the range comes behind the batch, the stream last, in every one of them
    assert re.search(r"uint64_t batch,\s*uint32_t prime_first,\s*uint32_t prime_count,(\s*uint32_t galois_elt,)?\s*void\* stream$", re.sub(r"\s+", " ", args)), args


def test_they_follow_the_galois_inner_product_in_the_header():
    text = _header()
    order = [text.index(name + "(") for name in ("agx_ntt_inner_product_galois", *NAMES, "agx_ntt_keyswitch_create")]
    assert order == sorted(order)


def test_no_new_constants_or_handles():
    text = _header()
    assert not re.findall(r"#define\s+AGX_(RING|ADD|SUB|NEGATE|TENSOR)\w*", text)
    assert sorted(re.findall(r"typedef\s+struct\s+(\w+)", text)) == ["agx_ntt_basis", "agx_ntt_group", "agx_ntt_keyswitch", "agx_ntt_plan"]


@pytest.mark.parametrize("method", METHODS)
def test_plan_has_the_method(agx, method):
    import inspect

    fn = getattr(agx.Plan, method)
    assert callable(fn)
    params = inspect.signature(fn).parameters
    assert params["prime_first"].default == 0 and params["prime_count"].default is None and params["stream"].default == 0


def test_a_call_without_a_plan_says_so_and_touches_nothing(agx):
    L = agx.lib()
    buf = (ctypes.c_uint64 * 64)()
    at = lambda k: ctypes.addressof(buf) + k
    calls = [
        ("agx_ntt_add", (None, at(0), at(128), at(256), 1, 0, 1, None)),
        ("agx_ntt_add", (None, at(0), at(0), at(0), 1, 0, 0, None)),               # prime_count = 0: the NULL rule comes first
        ("agx_ntt_add", (None, at(4), at(128), at(8), 1, 7, 0xffffffff, None)),    # misaligned, overlapping, a range that would wrap
        ("agx_ntt_add", (None, None, None, None, 0, 0, 0, None)),
        ("agx_ntt_sub", (None, at(0), at(128), at(256), 1, 0, 1, None)),
        ("agx_ntt_sub", (None, at(0), at(128), at(8), 1, 0, 0, None)),
        ("agx_ntt_negate", (None, at(0), at(256), 1, 0, 1, None)),
        ("agx_ntt_negate", (None, at(0), at(8), 1, 3, 0, None)),
        ("agx_ntt_add_galois", (None, at(0), at(128), at(256), 1, 0, 1, 5, None)),
        ("agx_ntt_add_galois", (None, at(0), at(128), at(128), 1, 0, 0, 4, None)),  # prime_count = 0, c on b and an even element
        ("agx_ntt_add_galois", (None, None, None, None, 0, 0, 0, 0, None)),
        ("agx_ntt_tensor", (None, at(0), at(128), at(256), 1, 0, 1, None)),
        ("agx_ntt_tensor", (None, at(0), at(0), at(0), 1, 0, 0, None)),             # in place
    ]
    for name, args in calls:
        assert getattr(L, name)(*args) == 1, (name, args)
    assert all(w == 0 for w in buf), "a buffer was written"
    # a NULL operand without a plan is the same status
    assert L.agx_ntt_tensor(None, None, at(0), at(0), 1, 0, 1, None) == 1
