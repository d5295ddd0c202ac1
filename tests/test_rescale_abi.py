"""CPU tests of the exact division by the last RNS modulus at the drop-in boundary: agx_ntt_rescale and agx_ntt_group_rescale are
declared in include/agx_ntt.h (with their two mode constants), exported by the library, bound in agx.ABI with a wrapper each, and
fail loudly before they touch a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("agx_ntt_rescale", "agx_ntt_group_rescale")


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
    assert hasattr(agx.Plan, "rescale") and hasattr(agx.DeviceGroup, "rescale")


def test_binding_matches_the_header(agx):
    """argument counts of the two prototypes, and the mode constants, as the binding has them"""
    text = _header()
    for name in NAMES:
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(agx.ABI[name][1]), name
        assert agx.ABI[name][0] is ctypes.c_int
    consts = dict(re.findall(r"#define\s+(AGX_RESCALE_\w+)\s+(\d+)", text))
    assert consts == {"AGX_RESCALE_FLOOR": "0", "AGX_RESCALE_ROUND": "1"}
    assert (agx.RESCALE_FLOOR, agx.RESCALE_ROUND) == (0, 1)


def test_calls_fail_loudly_without_a_plan_or_a_group(agx):
    L = agx.lib()
    assert L.agx_ntt_rescale(None, None, None, None, 1, 0, None) == 1
    assert L.agx_ntt_rescale(None, None, None, None, 1, 7, None) == 1
    assert L.agx_ntt_group_rescale(None, None, None, None, None, 0) == 1      # a null group
    assert L.agx_ntt_group_rescale(None, None, None, None, None, 1) == 1


def test_a_plan_cannot_be_made_without_a_device(agx):
    """where no GPU is visible there is no plan to call with: creation reports it instead of handing out something a rescale could run on"""
    if agx.device_count() != 0:
        return
    h = ctypes.c_void_p(None)
    q = (ctypes.c_uint64 * 2)(*agx.find_primes(60, 64, 2))
    assert agx.lib().agx_ntt_plan_create_auto(ctypes.byref(h), 64, 2, q, None) == 6      # AGX_ERR_NO_DEVICE
    assert not h.value
