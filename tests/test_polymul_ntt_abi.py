"""CPU tests of the product by a pre-transformed operand at the drop-in boundary: agx_ntt_polymul_ntt and
agx_ntt_group_polymul_ntt are declared in include/agx_ntt.h, exported by the library, bound in agx.ABI, and refuse NULL
arguments before they touch a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("agx_ntt_polymul_ntt", "agx_ntt_group_polymul_ntt")


def test_names_are_bound_exported_and_declared(agx):
    text = open(os.path.join(ROOT, "include", "agx_ntt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(agx.LIB_PATH)
    for name in NAMES:
        assert name in agx.ABI, name
        assert hasattr(raw, name), name
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert hasattr(agx.Plan, "polymul_ntt") and hasattr(agx.DeviceGroup, "polymul_ntt")


def test_null_arguments(agx):
    L = agx.lib()
    assert L.agx_ntt_polymul_ntt(None, None, None, None, 1, 1, None) == 1
    assert L.agx_ntt_group_polymul_ntt(None, None, None, None, None, None) == 1
