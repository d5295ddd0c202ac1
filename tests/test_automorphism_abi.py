"""CPU tests of the Galois automorphism at the drop-in boundary: agx_ntt_automorphism, agx_ntt_group_automorphism and
agx_ntt_galois_element are declared in include/agx_ntt.h (with the two form constants), exported by the library, bound in agx.ABI with a
wrapper each, fail loudly before they touch a device, and the Galois elements of rotations are the powers of 5 modulo 2n."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("agx_ntt_automorphism", "agx_ntt_group_automorphism", "agx_ntt_galois_element")


def _header():
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_names_are_bound_exported_and_declared(agx):
    text = _header()
    raw = ctypes.CDLL(agx.LIB_PATH)
    for name in NAMES:
        assert name in agx.ABI, name
        assert hasattr(raw, name), name
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert hasattr(agx.Plan, "automorphism") and hasattr(agx.DeviceGroup, "automorphism") and callable(agx.galois_element)


def test_binding_matches_the_header(agx):
    """argument counts of the three prototypes, and the form constants, as the binding has them"""
    text = _header()
    for name in NAMES:
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(agx.ABI[name][1]), name
        assert agx.ABI[name][0] is ctypes.c_int
    consts = dict(re.findall(r"#define\s+(AGX_FORM_\w+)\s+(\d+)", text))
    assert consts == {"AGX_FORM_COEFF": "0", "AGX_FORM_NTT": "1"}
    assert (agx.FORM_COEFF, agx.FORM_NTT) == (0, 1)


def test_calls_fail_loudly_without_a_plan_or_a_group(agx):
    L = agx.lib()
    for form in (0, 1, 7):
        assert L.agx_ntt_automorphism(None, None, None, 1, 5, form, None) == 1
        assert L.agx_ntt_group_automorphism(None, None, None, None, 5, form) == 1


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
