"""agilex-ntt_amd: MI355X-native batched negacyclic NTT engine -- thin Python host layer.

The product is the C-ABI shared library ``lib/libagxntt.so`` (``include/agx_ntt.h``), built
from ``csrc/`` by hipcc for gfx950.  This module only binds that ABI with ctypes so that
bench.py and the tests can drive it from Python with torch providing device memory and
streams.  There is no CPU fallback: if the library is missing, loading fails loudly.

The directory name has a hyphen (it mirrors the reference repository's name), so import it
through the ``agilex_ntt_amd`` shim at the repository root.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AGX_NTT_LIB") or os.path.join(_HERE, "lib", "libagxntt.so")   # override: A/B builds in tools/
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

AGX_OK = 0
VARIANT_AUTO, VARIANT_LDS_RADIX2, VARIANT_REGBLOCK = 0, 1, 2
VARIANT_REGBLOCK_BASE = 256  # + registry index: A/B measurements only
RESCALE_FLOOR, RESCALE_ROUND = 0, 1
FORM_COEFF, FORM_NTT = 0, 1
BASIS_MAX_SRC = 16

_u64 = ctypes.c_uint64
_u32 = ctypes.c_uint32
_i64 = ctypes.c_int64
_int = ctypes.c_int
_vp = ctypes.c_void_p
_dbl = ctypes.c_double
_p64 = ctypes.POINTER(ctypes.c_uint64)

# name -> (restype, argtypes): every symbol include/agx_ntt.h declares
ABI = {
    "agx_ntt_strerror": (ctypes.c_char_p, [_int]),
    "agx_ntt_last_hip_error": (_int, []),
    "agx_ntt_device_count": (_int, [ctypes.POINTER(_int)]),
    "agx_ntt_forward_host": (_int, [_p64, _p64, _p64, _p64, _p64, _p64, _u32, _u32]),
    "agx_ntt_forward_host_stream": (_int, [_vp, _p64, _p64, _p64, _u64]),
    "agx_ntt_inverse_host_stream": (_int, [_vp, _p64, _p64, _u64]),
    "agx_ntt_release_caches": (_int, []),
    "agx_ntt_plan_create": (_int, [ctypes.POINTER(_vp), _u32, _u32, _p64, _p64, _p64, _p64, _p64]),
    "agx_ntt_plan_create_auto": (_int, [ctypes.POINTER(_vp), _u32, _u32, _p64, _p64]),
    "agx_ntt_plan_destroy": (_int, [_vp]),
    "agx_ntt_plan_set_variant": (_int, [_vp, _int]),
    "agx_ntt_plan_info": (_int, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "agx_ntt_plan_forward_kernel": (_int, [_vp, _u64, ctypes.POINTER(_int)]),
    "agx_ntt_plan_get_modulus": (_int, [_vp, _u32, _p64, _p64]),
    "agx_ntt_forward": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_forward_lazy": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_inverse": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_forward_strided": (_int, [_vp, _vp, _vp, _u64, _i64, _i64, _vp]),
    "agx_ntt_inverse_strided": (_int, [_vp, _vp, _vp, _u64, _i64, _i64, _vp]),
    "agx_ntt_forward_range": (_int, [_vp, _vp, _vp, _u64, _u32, _u32, _vp]),
    "agx_ntt_inverse_range": (_int, [_vp, _vp, _vp, _u64, _u32, _u32, _vp]),
    "agx_ntt_pointwise": (_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_polymul": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_polymul_ntt": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _vp]),
    "agx_ntt_rescale": (_int, [_vp, _vp, _vp, _vp, _u64, _int, _vp]),
    "agx_ntt_automorphism": (_int, [_vp, _vp, _vp, _u64, _u32, _int, _vp]),
    "agx_ntt_basis_create": (_int, [ctypes.POINTER(_vp), _vp, _u32, _u32, _u32, _u32]),
    "agx_ntt_basis_destroy": (_int, [_vp]),
    "agx_ntt_basis_info": (_int, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_int)]),
    "agx_ntt_basis_extend": (_int, [_vp, _vp, _vp, _u64, _int, _vp]),
    "agx_ntt_basis_mod_down": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_basis_mod_down_info": (_int, [_vp, ctypes.POINTER(_int)]),
    "agx_ntt_basis_create_plain": (_int, [ctypes.POINTER(_vp), _vp, _u32, _u32, _u32, _u32, _u64]),
    "agx_ntt_basis_mod_down_mode": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _int, _vp]),
    "agx_ntt_keyswitch_create_plain": (_int, [ctypes.POINTER(_vp), _vp, _u32, _u32, _u32, _u32, _u64]),
    "agx_ntt_basis_create_aux": (_int, [ctypes.POINTER(_vp), _vp, _u32, _u32, _u32, _u32, _u32]),
    "agx_ntt_basis_aux_info": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_u32), ctypes.POINTER(_int)]),
    "agx_ntt_basis_extend_exact": (_int, [_vp, _vp, _vp, _vp, _u64, _int, _vp]),
    "agx_ntt_basis_extend_mont": (_int, [_vp, _vp, _vp, _u64, _int, _vp]),
    "agx_ntt_basis_create_quotient": (_int, [ctypes.POINTER(_vp), _vp, _u32, _u32, _u32, _u32, _u32, _u64]),
    "agx_ntt_basis_quotient_info": (_int, [_vp, ctypes.POINTER(_int), _p64, ctypes.POINTER(_int)]),
    "agx_ntt_basis_quotient": (_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_inner_product": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _u32, _u32, _vp]),
    "agx_ntt_inner_product_galois": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _u32, _u32, _u32, _vp]),
    "agx_ntt_add": (_int, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _vp]),
    "agx_ntt_sub": (_int, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _vp]),
    "agx_ntt_negate": (_int, [_vp, _vp, _vp, _u64, _u32, _u32, _vp]),
    "agx_ntt_add_galois": (_int, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    "agx_ntt_tensor": (_int, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _vp]),
    "agx_ntt_mul_add_galois": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, _u32, _u32, _u32, _int, _vp]),
    "agx_ntt_keyswitch_create": (_int, [ctypes.POINTER(_vp), _vp, _u32, _u32, _u32, _u32]),
    "agx_ntt_keyswitch_destroy": (_int, [_vp]),
    "agx_ntt_keyswitch_info": (_int, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_int)]),
    "agx_ntt_keyswitch_scratch_words": (_int, [_vp, _u64, _p64]),
    "agx_ntt_keyswitch_apply": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_keyswitch_hoisted_words": (_int, [_vp, _u64, _p64, _p64, _p64]),
    "agx_ntt_keyswitch_decompose": (_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_keyswitch_apply_decomposed": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp]),
    "agx_ntt_keyswitch_hoisted_info": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "agx_ntt_keyswitch_accumulate_decomposed": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _u64, _u32, _int, _vp]),
    "agx_ntt_keyswitch_mod_down": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_plain_create": (_int, [ctypes.POINTER(_vp), _vp, _u32, _u32, _u32, _u64]),
    "agx_ntt_plain_destroy": (_int, [_vp]),
    "agx_ntt_plain_info": (_int, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32), _p64, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "agx_ntt_plain_scale_up": (_int, [_vp, _vp, _vp, _u64, _int, _vp]),
    "agx_ntt_plain_lift": (_int, [_vp, _vp, _vp, _u64, _int, _vp]),
    "agx_ntt_plain_scale_down": (_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_fill_synthetic": (_int, [_vp, _vp, _u64, _u64, _u64, _vp]),
    "agx_ntt_sample_uniform": (_int, [_vp, _vp, _u64, _vp, _u64, _u64, _u32, _u32, _vp]),
    "agx_ntt_sample_ternary": (_int, [_vp, _vp, _u64, _vp, _u64, _u64, _u32, _u32, _int, _vp]),
    "agx_ntt_sample_cbd": (_int, [_vp, _vp, _u64, _u32, _vp, _u64, _u64, _u32, _u32, _int, _vp]),
    "agx_ntt_find_primes": (_int, [_u32, _u32, _u32, _p64]),
    "agx_ntt_min_root": (_int, [_u64, _u32, _p64]),
    "agx_ntt_make_tables": (_int, [_u64, _u64, _u32, _p64, _p64]),
    "agx_ntt_make_inverse_tables": (_int, [_u64, _u64, _u32, _p64, _p64]),
    "agx_ntt_galois_element": (_int, [_u32, _i64, ctypes.POINTER(_u32)]),
    "agx_ntt_ckks_create": (_int, [ctypes.POINTER(_vp), _vp, _u32, _u32]),
    "agx_ntt_ckks_destroy": (_int, [_vp]),
    "agx_ntt_ckks_info": (_int, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "agx_ntt_ckks_encode": (_int, [_vp, _vp, _u32, _dbl, _vp, _u64, _u32, _int, _vp]),
    "agx_ntt_ckks_decode": (_int, [_vp, _vp, _int, _u32, _dbl, _vp, _u32, _vp, _u64, _vp]),
    "agx_ntt_ckks_twiddle": (_int, [_u32, _u32, ctypes.POINTER(_dbl)]),
    "agx_ntt_batch_create": (_int, [ctypes.POINTER(_vp), _u32, _u64]),
    "agx_ntt_batch_destroy": (_int, [_vp]),
    "agx_ntt_batch_info": (_int, [_vp, ctypes.POINTER(_u32), _p64, _p64, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "agx_ntt_batch_plan": (_int, [_vp, ctypes.POINTER(_vp)]),
    "agx_ntt_batch_encode": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_batch_decode": (_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "agx_ntt_plain_reduce": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _vp]),
    # groups: the same calls over several GPUs (one shard, one host thread, one stream per listed device)
    "agx_ntt_shard_range": (_int, [_u64, _u32, _u32, _p64, _p64]),
    "agx_ntt_group_create": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_int), _u32, _u32, _u32, _p64, _p64, _p64, _p64, _p64]),
    "agx_ntt_group_create_auto": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_int), _u32, _u32, _u32, _p64, _p64]),
    "agx_ntt_group_destroy": (_int, [_vp]),
    "agx_ntt_group_info": (_int, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "agx_ntt_group_shard": (_int, [_vp, _u32, ctypes.POINTER(_int), ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "agx_ntt_group_forward_host": (_int, [_vp, _p64, _p64, _p64, _u64]),
    "agx_ntt_group_inverse_host": (_int, [_vp, _p64, _p64, _u64]),
    "agx_ntt_group_forward": (_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _p64]),
    "agx_ntt_group_inverse": (_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _p64]),
    "agx_ntt_group_polymul": (_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _p64]),
    "agx_ntt_group_polymul_ntt": (_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _p64, _p64]),
    "agx_ntt_group_rescale": (_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _p64, _int]),
    "agx_ntt_group_automorphism": (_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _p64, _u32, _int]),
    "agx_ntt_group_synchronize": (_int, [_vp]),
}


class AgxError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = lib().agx_ntt_strerror(status).decode()
        super().__init__(f"{where}: agx status {status} ({msg}), hip error {lib().agx_ntt_last_hip_error()}")


def build(verbose=False, with_diag=False):
    """Compile the gfx950 library in-tree (hipcc cross-compiles without a GPU).  with_diag: lib/libagxntt_diag.so in the same make
    invocation, so the objects of both libraries compile side by side."""
    cmd = ["make", "-C", _HERE, f"-j{min(8, os.cpu_count() or 1)}", "build"] + (["diag"] if with_diag else [])
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7) and ask for
    it by file name, so a process that loaded /opt/rocm's copy first ends up with two HIP
    runtimes: torch's device pointers and streams would then mean nothing to this library.
    Loading torch's copy by path before libagxntt.so makes both resolve to the same runtime,
    whatever the import order.  Without torch installed the system runtime is used."""
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def lib():
    """Load libagxntt.so.  Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make -C {_HERE} build` (or __graft_entry__.build())")
        _share_hip_runtime_with_torch()
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(L, name)  # AttributeError if the ABI and the header drift apart
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(status, where):
    if status != AGX_OK:
        raise AgxError(status, where)


def _np_ptr(a):
    import numpy as np

    assert isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_p64)


def _table_args(moduli, psi, tables):
    """what follows (n, num_primes) in agx_ntt_{plan,group}_create_auto (tables is None: moduli, psi or NULL) and in
    agx_ntt_{plan,group}_create (moduli, tw, pre, itw or NULL, ipre or NULL; the inverse pair only where four tables are given)"""
    import numpy as np

    if tables is None:
        arrays = [moduli, None if psi is None else [int(p) for p in psi]]
    else:
        arrays = [moduli] + list(tables[:2]) + (list(tables[2:]) if len(tables) == 4 else [None, None])
    return [None if a is None else _np_ptr(np.ascontiguousarray(a, dtype=np.uint64)) for a in arrays]      # a pointer keeps its array alive


def _key32(key):
    """the 32 key bytes of a sampling call as a host buffer; None stays None (the library answers the NULL rule)"""
    if key is None:
        return None
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("a sampling key is 32 bytes")
    return key


def _out_array(out, count):
    """the caller's `out`, or a fresh array of `count` words"""
    import numpy as np

    return np.zeros(count, dtype=np.uint64) if out is None else out


def kernel_source_files():
    """the DEVICE sources the kernels are built from, sorted: every csrc/*.hip and whatever of csrc/ they include, directly or
    through another such file (their `#include "..."` lines, wherever in a file they stand); not the host-side *.cpp"""
    import glob
    import re

    csrc = os.path.join(_HERE, "csrc")
    todo, seen = glob.glob(os.path.join(csrc, "*.hip")), set()
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), flags=re.M):
            inc = os.path.normpath(os.path.join(csrc, inc))
            if os.path.dirname(inc) == csrc and os.path.exists(inc):
                todo.append(inc)
    return sorted(seen)


def kernel_source_sha16():
    """sha256[:16] over kernel_source_files(), names and contents: ties a committed PMC figure (profiles/hbm_traffic.json) to
    the kernels it was measured on"""
    import hashlib

    h = hashlib.sha256()
    for f in kernel_source_files():
        h.update(os.path.relpath(f, _HERE).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


DIAG_LIB_PATH = os.path.join(_HERE, "lib", "libagxntt_diag.so")   # `make diag`: product + diagnostics kernels (tools/agx_ntt_diag.h)


def build_diag():
    """Compile lib/libagxntt_diag.so (trace twin, streaming A/B kernels); load it with AGX_NTT_LIB=DIAG_LIB_PATH."""
    subprocess.check_call(["make", "-s", "-C", _HERE, f"-j{min(8, os.cpu_count() or 1)}", "diag"])
    return DIAG_LIB_PATH


def debug_set_trace_buffer(d_buf, nbytes):
    """Diagnostics (tools/timeline.py), diag library only: where the registry's trace kernel writes its phase
    stamps; (0, 0) = off.  The product library does not export the hook."""
    try:
        fn = lib().agx_ntt_debug_set_trace_buffer
    except AttributeError:
        raise RuntimeError("agx_ntt_debug_set_trace_buffer is only in lib/libagxntt_diag.so: `make -C agilex-ntt_amd diag` "
                           "and run with AGX_NTT_LIB=<that file>") from None
    fn.restype, fn.argtypes = _int, [_vp, _u64]
    _check(fn(d_buf, nbytes), "debug_set_trace_buffer")


def device_count():
    c = _int(0)
    _check(lib().agx_ntt_device_count(ctypes.byref(c)), "device_count")
    return c.value


# ---------------------------------------------------------------------------------------
# host math
# ---------------------------------------------------------------------------------------
def find_primes(bits, n, count=1):
    import numpy as np

    out = np.zeros(count, dtype=np.uint64)
    _check(lib().agx_ntt_find_primes(bits, n, count, _np_ptr(out)), "find_primes")
    return [int(v) for v in out]


def min_root(q, n):
    r = _u64(0)
    _check(lib().agx_ntt_min_root(q, n, ctypes.byref(r)), "min_root")
    return r.value


def make_tables(q, psi, n, inverse=False):
    import numpy as np

    tw = np.zeros(n, dtype=np.uint64)
    pre = np.zeros(n, dtype=np.uint64)
    fn = lib().agx_ntt_make_inverse_tables if inverse else lib().agx_ntt_make_tables
    _check(fn(q, psi, n, _np_ptr(tw), _np_ptr(pre)), "make_tables")
    return tw, pre


def galois_element(n, step):
    """the Galois element of a slot rotation by `step`: 5^step mod 2n (negative step: powers of 5^-1); conjugation is 2n - 1"""
    g = _u32(0)
    _check(lib().agx_ntt_galois_element(n, step, ctypes.byref(g)), "galois_element")
    return g.value


# ---------------------------------------------------------------------------------------
# one-shot host path: the reference's ntt_input_kernel + fwd_ntt_kernel + ntt_output_kernel
# ---------------------------------------------------------------------------------------
def forward_host(in1, in2, modulus, twiddles, precons, n, num_frames):
    import numpy as np

    out = np.zeros(num_frames * n, dtype=np.uint64)
    mod = np.array([modulus], dtype=np.uint64)
    _check(lib().agx_ntt_forward_host(_np_ptr(in1), _np_ptr(in2), _np_ptr(mod), _np_ptr(twiddles), _np_ptr(precons),
                                      _np_ptr(out), n, num_frames), "forward_host")
    return out


# ---------------------------------------------------------------------------------------
# plans and device-pointer calls (pointers are plain integers, e.g. torch.Tensor.data_ptr())
# ---------------------------------------------------------------------------------------
class Plan:
    """Device-resident tables for `moduli` at size n.  Tables are generated by the library
    unless `tables=(tw, pre[, itw, ipre])` (each [num_primes, n] uint64) is given."""

    def __init__(self, n, moduli, psi=None, tables=None):
        self.n = int(n)
        self.moduli = [int(q) for q in moduli]
        self._h = _vp(None)
        create, where = (lib().agx_ntt_plan_create_auto, "plan_create_auto") if tables is None else (lib().agx_ntt_plan_create, "plan_create")
        _check(create(ctypes.byref(self._h), self.n, len(self.moduli), *_table_args(self.moduli, psi, tables)), where)

    @property
    def num_primes(self):
        return len(self.moduli)

    def psi(self, k):
        q, r = _u64(0), _u64(0)
        _check(lib().agx_ntt_plan_get_modulus(self._h, k, ctypes.byref(q), ctypes.byref(r)), "plan_get_modulus")
        return r.value

    def set_variant(self, variant):
        _check(lib().agx_ntt_plan_set_variant(self._h, variant), "plan_set_variant")

    def forward_kernel(self, batch):
        """registry id of the kernel a forward call of `batch` frames per prime runs (-1: the LDS radix-2 kernels)"""
        k = _int(0)
        _check(lib().agx_ntt_plan_forward_kernel(self._h, batch, ctypes.byref(k)), "plan_forward_kernel")
        return k.value

    def forward(self, d_in, d_out, batch, stream=0):
        _check(lib().agx_ntt_forward(self._h, d_in, d_out, batch, stream), "forward")

    def forward_lazy(self, d_in, d_out, batch, stream=0):
        _check(lib().agx_ntt_forward_lazy(self._h, d_in, d_out, batch, stream), "forward_lazy")

    def inverse(self, d_in, d_out, batch, stream=0):
        _check(lib().agx_ntt_inverse(self._h, d_in, d_out, batch, stream), "inverse")

    def forward_range(self, d_in, d_out, batch, prime_first, prime_count, stream=0):
        """forward on the plan primes [prime_first, prime_first + prime_count): d_in, d_out dense [prime_count][batch][n], the words a plan over those
        primes with the same roots would write; in place allowed"""
        _check(lib().agx_ntt_forward_range(self._h, d_in, d_out, batch, prime_first, prime_count, stream), "forward_range")

    def inverse_range(self, d_in, d_out, batch, prime_first, prime_count, stream=0):
        """inverse on the plan primes [prime_first, prime_first + prime_count), as forward_range"""
        _check(lib().agx_ntt_inverse_range(self._h, d_in, d_out, batch, prime_first, prime_count, stream), "inverse_range")

    def forward_strided(self, d_in, d_out, batch, prime_stride, poly_stride, stream=0):
        _check(lib().agx_ntt_forward_strided(self._h, d_in, d_out, batch, prime_stride, poly_stride, stream), "forward_strided")

    def inverse_strided(self, d_in, d_out, batch, prime_stride, poly_stride, stream=0):
        _check(lib().agx_ntt_inverse_strided(self._h, d_in, d_out, batch, prime_stride, poly_stride, stream), "inverse_strided")

    def pointwise(self, d_a, d_b, d_c, batch, stream=0):
        _check(lib().agx_ntt_pointwise(self._h, d_a, d_b, d_c, batch, stream), "pointwise")

    def polymul(self, d_a, d_b, d_c, d_scratch, batch, stream=0):
        _check(lib().agx_ntt_polymul(self._h, d_a, d_b, d_c, d_scratch, batch, stream), "polymul")

    def polymul_ntt(self, d_a, d_bhat, d_c, batch, bhat_batch=None, stream=0):
        """c = a * b with b given by its transform d_bhat (what forward / forward_lazy of this plan wrote); bhat_batch: None = batch
        (one bhat frame per frame) or 1 (one bhat frame per prime, shared by the whole batch)"""
        _check(lib().agx_ntt_polymul_ntt(self._h, d_a, d_bhat, d_c, batch, batch if bhat_batch is None else bhat_batch, stream), "polymul_ntt")

    def rescale(self, d_x, d_out, d_scratch, batch, mode=RESCALE_ROUND, stream=0):
        """exact division by the last modulus on NTT-form frames: d_x [P][batch][n] -> d_out [P-1][batch][n] (may be d_x); d_scratch:
        batch*n words, or d_x's last slab (which is then overwritten); mode: RESCALE_FLOOR or RESCALE_ROUND"""
        _check(lib().agx_ntt_rescale(self._h, d_x, d_out, d_scratch, batch, mode, stream), "rescale")

    def automorphism(self, d_in, d_out, batch, galois_elt, form=FORM_NTT, stream=0):
        """a(X) -> a(X^galois_elt) on every frame, out of place (d_out may not touch d_in): FORM_NTT permutes the words of NTT-form frames,
        FORM_COEFF moves and negates coefficients (inputs in [0,4q), outputs in [0,q)); galois_elt odd, below 2n"""
        _check(lib().agx_ntt_automorphism(self._h, d_in, d_out, batch, galois_elt, form, stream), "automorphism")

    def basis(self, src_first, src_count, dst_first, dst_count, t=1):
        """Basis(self, ...): the fast base conversion from primes [src_first, src_first + src_count) to [dst_first, dst_first + dst_count); t: the
        plaintext modulus its ModDown keeps the value modulo (BGV), 1 for none"""
        return Basis(self, src_first, src_count, dst_first, dst_count, t)

    def basis_aux(self, src_first, src_count, dst_first, dst_count, aux_prime):
        """Basis.with_aux(self, ...): that basis (t = 1) with the plan prime aux_prime, outside both ranges, as its auxiliary prime: the one that
        extend_exact and extend_mont (the exact conversions of a BFV multiplication) need"""
        return Basis.with_aux(self, src_first, src_count, dst_first, dst_count, aux_prime)

    def basis_quotient(self, b_first, b_count, q_first, q_count, aux_prime, t):
        """Basis.with_quotient(self, ...): the basis of basis_aux(b_first, b_count, q_first, q_count, aux_prime) with the constants of Basis.quotient for
        the plaintext modulus t: BFV's divide-and-return in one call"""
        return Basis.with_quotient(self, b_first, b_count, q_first, q_count, aux_prime, t)

    def plain(self, q_first, q_count, gamma_prime, t):
        """Plain(self, ...): BFV's plaintext boundary for Q = primes [q_first, q_first + q_count), the auxiliary prime gamma_prime outside Q and the
        plaintext modulus t in [2, 2^62): scale_up, lift and scale_down"""
        return Plain(self, q_first, q_count, gamma_prime, t)

    def ckks(self, q_first, q_count):
        """Ckks(self, ...): CKKS encoding and decoding on the primes [q_first, q_first + q_count), q_count <= 16; a call may use any prefix of them"""
        return Ckks(self, q_first, q_count)

    def sample_uniform(self, key, nonce, d_out, batch, frame_first=0, prime_first=0, prime_count=None, stream=0):
        """uniform words below q_i on the plan primes [prime_first, prime_first + prime_count) (None: all of the plan's), one launch: d_out
        [prime_count][batch][n]; key: 32 bytes (the caller's seed, host memory), nonce: the 64-bit draw number, never reused under one key for one kind;
        frame f of the call is frame frame_first + f of the draw, so split batches write what one call writes (ChaCha20 with rejection: include/agx_ntt.h)"""
        _check(lib().agx_ntt_sample_uniform(self._h, _key32(key), nonce, d_out, batch, frame_first, *self._prime_range(prime_first, prime_count), stream), "sample_uniform")

    def sample_ternary(self, key, nonce, d_out, batch, frame_first=0, prime_first=0, prime_count=None, form=FORM_NTT, stream=0):
        """coefficients uniform in {-1, 0, +1}, the same value under every prime of the range, as sample_uniform; form: FORM_COEFF, or FORM_NTT = the
        plan's forward on the range in place behind the draw"""
        _check(lib().agx_ntt_sample_ternary(self._h, _key32(key), nonce, d_out, batch, frame_first, *self._prime_range(prime_first, prime_count), form, stream),
               "sample_ternary")

    def sample_cbd(self, key, nonce, eta, d_out, batch, frame_first=0, prime_first=0, prime_count=None, form=FORM_NTT, stream=0):
        """centred-binomial coefficients of variance eta / 2 (1 <= eta <= 32; 21: sigma = 3.24), as sample_ternary"""
        _check(lib().agx_ntt_sample_cbd(self._h, _key32(key), nonce, eta, d_out, batch, frame_first, *self._prime_range(prime_first, prime_count), form, stream),
               "sample_cbd")

    def inner_product(self, d_a, d_bhat, d_c, batch, terms, outputs=1, bhat_batch=None, stream=0):
        """c_o = sum_t a_t o bhat_{t,o} mod q in one launch: d_a [terms][P][batch][n], d_bhat [terms][outputs][P][bhat_batch][n], d_c
        [outputs][P][batch][n]; inputs in [0,4q), c fully reduced, out of place; bhat_batch: None = batch, or 1 (one key frame per prime)"""
        _check(lib().agx_ntt_inner_product(self._h, d_a, d_bhat, d_c, batch, batch if bhat_batch is None else bhat_batch, terms, outputs, stream), "inner_product")

    def inner_product_galois(self, d_a, d_bhat, d_c, batch, terms, galois_elt, outputs=1, bhat_batch=None, stream=0):
        """inner_product with a read through the automorphism X -> X^galois_elt: c_o[i] = sum_t a_t[pi_g(i)] o bhat_{t,o}[i], one launch, no
        permuted copy of a; galois_elt odd, below 2n (1: inner_product itself)"""
        _check(lib().agx_ntt_inner_product_galois(self._h, d_a, d_bhat, d_c, batch, batch if bhat_batch is None else bhat_batch, terms, outputs, galois_elt, stream),
               "inner_product_galois")

    def _prime_range(self, prime_first, prime_count):
        return prime_first, self.num_primes if prime_count is None else prime_count

    def add(self, d_a, d_b, d_c, batch, prime_first=0, prime_count=None, stream=0):
        """c = a + b mod q on the plan primes [prime_first, prime_first + prime_count) (None: all of the plan's), one launch: every operand dense
        [prime_count][batch][n]; inputs in [0,4q), c fully reduced; d_c may be d_a, d_b or both"""
        _check(lib().agx_ntt_add(self._h, d_a, d_b, d_c, batch, *self._prime_range(prime_first, prime_count), stream), "add")

    def sub(self, d_a, d_b, d_c, batch, prime_first=0, prime_count=None, stream=0):
        """c = a - b mod q, as add"""
        _check(lib().agx_ntt_sub(self._h, d_a, d_b, d_c, batch, *self._prime_range(prime_first, prime_count), stream), "sub")

    def negate(self, d_a, d_c, batch, prime_first=0, prime_count=None, stream=0):
        """c = -a mod q (-0 = 0), as add; d_c may be d_a"""
        _check(lib().agx_ntt_negate(self._h, d_a, d_c, batch, *self._prime_range(prime_first, prime_count), stream), "negate")

    def add_galois(self, d_a, d_b, d_c, batch, galois_elt, prime_first=0, prime_count=None, stream=0):
        """c[i] = a[i] + b[pi_g(i)] mod q within every frame: a plus the NTT-form automorphism X -> X^galois_elt of b, one launch, no permuted copy of b;
        d_c may be d_a and may not touch d_b; galois_elt odd, below 2n (1: add itself)"""
        _check(lib().agx_ntt_add_galois(self._h, d_a, d_b, d_c, batch, *self._prime_range(prime_first, prime_count), galois_elt, stream), "add_galois")

    def tensor(self, d_a, d_b, d_c, batch, prime_first=0, prime_count=None, stream=0):
        """(c_0, c_1, c_2) = (a_0 o b_0, a_0 o b_1 + a_1 o b_0, a_1 o b_1) mod q in one launch: d_a, d_b [2][prime_count][batch][n], d_c
        [3][prime_count][batch][n], out of place (d_a may be d_b)"""
        _check(lib().agx_ntt_tensor(self._h, d_a, d_b, d_c, batch, *self._prime_range(prime_first, prime_count), stream), "tensor")

    def mul_add_galois(self, d_w, d_b, d_c, batch, galois_elt=1, w_batch=None, accumulate=False, prime_first=0, prime_count=None, stream=0):
        """c[i] = (c[i] if accumulate) + w[i] o b[pi_g(i)] mod q within every frame, one launch: d_w [prime_count][w_batch][n] (w_batch: None = batch, or 1:
        one frame per prime for the whole batch), d_b and d_c [prime_count][batch][n]; galois_elt = 1 without accumulate is the ranged plaintext product,
        where d_c may be d_b; otherwise d_c touches neither"""
        _check(lib().agx_ntt_mul_add_galois(self._h, d_w, batch if w_batch is None else w_batch, d_b, d_c, batch, *self._prime_range(prime_first, prime_count),
                                            galois_elt, int(accumulate), stream), "mul_add_galois")

    def keyswitch(self, q_count, p_first, p_count, alpha, t=1):
        """KeySwitch(self, ...): the hybrid key switch at level Q = primes [0, q_count) with special primes [p_first, p_first + p_count); t: the
        plaintext modulus its ModDown keeps the value modulo (BGV), 1 for none"""
        return KeySwitch(self, q_count, p_first, p_count, alpha, t)

    def fill_synthetic(self, d_out, batch, first_poly=0, seed=42, stream=0):
        _check(lib().agx_ntt_fill_synthetic(self._h, d_out, batch, first_poly, seed, stream), "fill_synthetic")

    def forward_host_stream(self, in1, in2, num_frames, out=None):
        """host frames through this (single-modulus) plan with overlapped transfers; `out` (optional) is a caller-owned
        uint64 array of num_frames*n elements (a fresh np.zeros array costs a page fault per 4 KiB when it is first written)"""
        out = _out_array(out, num_frames * self.n)
        _check(lib().agx_ntt_forward_host_stream(self._h, _np_ptr(in1), _np_ptr(in2), _np_ptr(out), num_frames), "forward_host_stream")
        return out

    def inverse_host_stream(self, in1, num_frames, out=None):
        out = _out_array(out, num_frames * self.n)
        _check(lib().agx_ntt_inverse_host_stream(self._h, _np_ptr(in1), _np_ptr(out), num_frames), "inverse_host_stream")
        return out

    def close(self):
        if self._h:
            lib().agx_ntt_plan_destroy(self._h)
            self._h = _vp(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Basis:
    """The constants of a fast RNS base conversion (agx_ntt_basis_*) from the plan's primes [src_first, src_first + src_count) to
    [dst_first, dst_first + dst_count).  `plan` is a Plan, or a raw plan handle (a DeviceGroup shard's: one basis per shard); it must
    outlive the basis, and its device must be current here and at every call.  t: a plaintext modulus (agx_ntt_basis_create_plain), a property
    of mod_down alone -- extend writes what it writes with t = 1, and t = 1 is the ordinary basis in every call."""

    def __init__(self, plan, src_first, src_count, dst_first, dst_count, t=1):
        self.plan = plan      # keeps a Plan alive
        self._h = _vp(None)
        handle = plan._h if isinstance(plan, Plan) else plan
        _check(lib().agx_ntt_basis_create_plain(ctypes.byref(self._h), handle, src_first, src_count, dst_first, dst_count, t), "basis_create_plain")

    @classmethod
    def with_aux(cls, plan, src_first, src_count, dst_first, dst_count, aux_prime):
        """the basis of Basis(plan, src_first, src_count, dst_first, dst_count) with an auxiliary prime (agx_ntt_basis_create_aux): plan prime aux_prime,
        outside both ranges.  Every other call behaves on it as on the ordinary basis; extend_exact and extend_mont need it."""
        self = cls.__new__(cls)
        self.plan = plan      # keeps a Plan alive
        self._h = _vp(None)
        handle = plan._h if isinstance(plan, Plan) else plan
        _check(lib().agx_ntt_basis_create_aux(ctypes.byref(self._h), handle, src_first, src_count, dst_first, dst_count, aux_prime), "basis_create_aux")
        return self

    @classmethod
    def with_quotient(cls, plan, b_first, b_count, q_first, q_count, aux_prime, t):
        """the basis of Basis.with_aux(plan, b_first, b_count, q_first, q_count, aux_prime) -- sources B, targets Q, auxiliary prime m, every other call
        unchanged -- with the constants of quotient for the plaintext modulus t (agx_ntt_basis_create_quotient): any 64-bit t >= 1"""
        self = cls.__new__(cls)
        self.plan = plan      # keeps a Plan alive
        self._h = _vp(None)
        handle = plan._h if isinstance(plan, Plan) else plan
        _check(lib().agx_ntt_basis_create_quotient(ctypes.byref(self._h), handle, b_first, b_count, q_first, q_count, aux_prime, t), "basis_create_quotient")
        return self

    def quotient_info(self):
        """(has_quotient, t, launches): whether the basis carries the quotient's constants, their t (0 without), and the kernel launches a quotient call
        takes under the plan's current variant"""
        has, t, launches = _int(0), _u64(0), _int(0)
        _check(lib().agx_ntt_basis_quotient_info(self._h, ctypes.byref(has), ctypes.byref(t), ctypes.byref(launches)), "basis_quotient_info")
        return bool(has.value), t.value, launches.value

    def quotient(self, d_x, d_out, d_scratch, batch, stream=0):
        """steps 4 to 7 of a BFV multiplication in one call: d_x [q_count + b_count + 1][batch][n] in NTT form (the slabs of Q, of B, of m: one component
        of the tensor product) -> d_out [q_count][batch][n] in NTT form: extend_exact of the fast floor of t x / Q, word for word; d_scratch: as many
        words as d_x, or d_x itself (which is then overwritten); d_out touches neither"""
        _check(lib().agx_ntt_basis_quotient(self._h, d_x, d_out, d_scratch, batch, stream), "basis_quotient")

    def aux_info(self):
        """(has_aux, aux_prime, launches_ntt_form): whether the basis has an auxiliary prime, its index in the plan, and the kernel launches a FORM_NTT
        call of extend_exact or extend_mont takes under the plan's current variant"""
        has, prime, launches = _int(0), _u32(0), _int(0)
        _check(lib().agx_ntt_basis_aux_info(self._h, ctypes.byref(has), ctypes.byref(prime), ctypes.byref(launches)), "basis_aux_info")
        return bool(has.value), prime.value, launches.value

    def extend_exact(self, d_x, d_xaux, d_out, batch, form=FORM_NTT, stream=0):
        """the Shenoy-Kumaresan conversion: d_x [src_count][batch][n] and d_xaux [1][batch][n] (the residues modulo the auxiliary prime m), coefficient form,
        lazy values allowed -> d_out [dst_count][batch][n]: (V - alpha D) mod q_j with V = sum_i y_i D_i and alpha = centre((V - r) D^-1 mod m): X' itself for
        every |X'| < ((m - 1) / 2 - src_count) D; out of place, d_x and d_xaux may overlap"""
        _check(lib().agx_ntt_basis_extend_exact(self._h, d_x, d_xaux, d_out, batch, form, stream), "basis_extend_exact")

    def extend_mont(self, d_x, d_out, batch, form=FORM_NTT, stream=0):
        """BEHZ's FastBConv_m~ and small Montgomery reduction: d_x [src_count][batch][n], coefficient form -> d_out [dst_count][batch][n]:
        (V + alpha D) m^-1 mod q_j with y_i = x_i m D_i^-1 mod q_i, V = sum_i y_i D_i and alpha = centre(-V D^-1 mod m): X or X - D; out of place"""
        _check(lib().agx_ntt_basis_extend_mont(self._h, d_x, d_out, batch, form, stream), "basis_extend_mont")

    def info(self):
        """(src_first, src_count, dst_first, dst_count, launches_ntt_form): the ranges, and the kernel launches a FORM_NTT call takes
        under the plan's current variant"""
        v = [_u32(0) for _ in range(4)]
        launches = _int(0)
        _check(lib().agx_ntt_basis_info(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(launches)), "basis_info")
        return tuple(x.value for x in v) + (launches.value,)

    def extend(self, d_x, d_out, batch, form=FORM_NTT, stream=0):
        """d_x [src_count][batch][n], coefficient form, values in [0,4q) -> d_out [dst_count][batch][n]: sum_i y_i D_i mod q_j (y_i = x_i D_i^-1
        mod q_i; no correction term), as coefficients (FORM_COEFF) or transformed as Plan.forward writes it (FORM_NTT); out of place"""
        _check(lib().agx_ntt_basis_extend(self._h, d_x, d_out, batch, form, stream), "basis_extend")

    def mod_down(self, d_xq, d_xp, d_out, d_scratch, batch, stream=0, mode=RESCALE_FLOOR):
        """ModDown on NTT-form frames: d_xq [dst_count][batch][n] and d_xp [src_count][batch][n] as Plan.forward / forward_lazy write them ->
        d_out [dst_count][batch][n] = (xq_j - NTT_j(t (V - h))) D^-1 mod q_j, V = sum_i y_i D_i, y_i = (INTT_i(xp_i) t^-1 + h) D_i^-1 mod q_i, with
        h = floor(D / 2) under RESCALE_ROUND and 0 under RESCALE_FLOOR, t the basis' plaintext modulus; d_out may be d_xq; d_scratch:
        src_count*batch*n words, or d_xp itself (which is then overwritten)"""
        _check(lib().agx_ntt_basis_mod_down_mode(self._h, d_xq, d_xp, d_out, d_scratch, batch, mode, stream), "basis_mod_down_mode")

    def mod_down_launches(self):
        """the kernel launches a mod_down call takes under the plan's current variant"""
        launches = _int(0)
        _check(lib().agx_ntt_basis_mod_down_info(self._h, ctypes.byref(launches)), "basis_mod_down_info")
        return launches.value

    def close(self):
        if self._h:
            lib().agx_ntt_basis_destroy(self._h)
            self._h = _vp(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plain:
    """BFV's plaintext boundary (agx_ntt_plain_*) on a plan: Q = primes [q_first, q_first + q_count), the auxiliary prime gamma = plan prime gamma_prime
    outside Q, the plaintext modulus t in [2, 2^62).  `plan` is a Plan or a raw plan handle (one handle per DeviceGroup shard); it must outlive the handle,
    and its device must be current here and at every call."""

    def __init__(self, plan, q_first, q_count, gamma_prime, t):
        self.plan = plan      # keeps a Plan alive
        self._h = _vp(None)
        handle = plan._h if isinstance(plan, Plan) else plan
        _check(lib().agx_ntt_plain_create(ctypes.byref(self._h), handle, q_first, q_count, gamma_prime, t), "plain_create")

    def info(self):
        """(q_first, q_count, gamma_prime, t, launches_scale_down, launches_ntt_form): the ranges, t, and the kernel launches of a scale_down call and of a
        FORM_NTT scale_up / lift call under the plan's current variant"""
        v = [_u32(0) for _ in range(3)]
        t, down, ntt = _u64(0), _int(0), _int(0)
        _check(lib().agx_ntt_plain_info(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(t), ctypes.byref(down), ctypes.byref(ntt)), "plain_info")
        return tuple(x.value for x in v) + (t.value, down.value, ntt.value)

    def scale_up(self, d_m, d_out, batch, form=FORM_NTT, stream=0):
        """d_m [batch][n], any words, m' = m mod t -> d_out [q_count][batch][n] = floor((2 D m' + t) / (2t)) mod q_i (D m' / t rounded, halves up), as
        coefficients (FORM_COEFF) or transformed as Plan.forward writes it (FORM_NTT); out of place"""
        _check(lib().agx_ntt_plain_scale_up(self._h, d_m, d_out, batch, form, stream), "plain_scale_up")

    def lift(self, d_m, d_out, batch, form=FORM_NTT, stream=0):
        """d_m [batch][n], any words -> d_out [q_count][batch][n]: the centred representative of m mod t (m' below ceil(t / 2), m' - t from there on)
        modulo q_i, forms as scale_up; out of place"""
        _check(lib().agx_ntt_plain_lift(self._h, d_m, d_out, batch, form, stream), "plain_lift")

    def scale_down(self, d_x, d_m, d_scratch, batch, stream=0):
        """the rounding of decryption: d_x [q_count][batch][n] in NTT form (reduced or lazy) -> d_m [batch][n] in [0, t): round(t X / D) mod t wherever the
        fraction lies within 1/2 - q_count / gamma of an integer; d_scratch: q_count*batch*n words, or d_x itself (which is then overwritten)"""
        _check(lib().agx_ntt_plain_scale_down(self._h, d_x, d_m, d_scratch, batch, stream), "plain_scale_down")

    def reduce(self, d_x, d_m, d_scratch, batch, factor=1, stream=0):
        """BGV decryption, the exact centred conversion Q -> t: d_x [q_count][batch][n] in NTT form (reduced or lazy) -> d_m [batch][n] = (factor mod t) X mod t
        in [0, t), X the centred representative modulo D; exact for every t; d_scratch as scale_down's"""
        _check(lib().agx_ntt_plain_reduce(self._h, d_x, d_m, d_scratch, factor, batch, stream), "plain_reduce")

    def close(self):
        if self._h:
            lib().agx_ntt_plain_destroy(self._h)
            self._h = _vp(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """SIMD batching of BFV / BGV (agx_ntt_batch_*): n slots modulo a prime t = 1 (mod 2n), t < 2^62, <-> the plaintext polynomial with those values at
    psi^(e_j), e_j = 5^j mod 2n on row 0 and 2n - e_j on row 1.  The handle owns a one-prime plan under t on the device current here, which must be current at
    every call."""

    def __init__(self, n, t):
        self._h = _vp(None)
        _check(lib().agx_ntt_batch_create(ctypes.byref(self._h), n, t), "batch_create")

    def info(self):
        """(n, t, psi, launches_encode, launches_decode) under the inner plan's current variant"""
        n, t, psi, enc, dec = _u32(0), _u64(0), _u64(0), _int(0), _int(0)
        _check(lib().agx_ntt_batch_info(self._h, ctypes.byref(n), ctypes.byref(t), ctypes.byref(psi), ctypes.byref(enc), ctypes.byref(dec)), "batch_info")
        return n.value, t.value, psi.value, enc.value, dec.value

    def plan(self):
        """the inner plan's raw handle, lent: for products modulo t and agx_ntt_plan_set_variant; the Batch owns it"""
        p = _vp(None)
        _check(lib().agx_ntt_batch_plan(self._h, ctypes.byref(p)), "batch_plan")
        return p.value

    def encode(self, d_z, d_m, batch, stream=0):
        """d_z [batch][n] slots, any words (taken modulo t) -> d_m [batch][n] in [0, t): the polynomial with those slot values; out of place"""
        _check(lib().agx_ntt_batch_encode(self._h, d_z, d_m, batch, stream), "batch_encode")

    def decode(self, d_m, d_z, d_scratch, batch, stream=0):
        """d_m [batch][n] in [0, t) -> d_z [batch][n]: z_j = m(psi^(e_j)); d_scratch: batch*n words, or d_m itself (which is then overwritten)"""
        _check(lib().agx_ntt_batch_decode(self._h, d_m, d_z, d_scratch, batch, stream), "batch_decode")

    def close(self):
        if self._h:
            lib().agx_ntt_batch_destroy(self._h)
            self._h = _vp(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ckks_twiddle(length, j):
    """tw(length, j) = (cos, sin) of 2 pi (5^j mod 4 length) / (4 length) as the kernels read it (agx_ntt_ckks_twiddle): host arithmetic, no device"""
    out = (_dbl * 2)()
    _check(lib().agx_ntt_ckks_twiddle(length, j, out), "ckks_twiddle")
    return out[0], out[1]


class Ckks:
    """CKKS encoding and decoding (agx_ntt_ckks_*) on a plan's primes [q_first, q_first + q_count).  `plan` is a Plan or a raw plan handle (one handle per
    DeviceGroup shard); it must outlive the handle, and its device must be current here and at every call.  Slot j sits at the root zeta^(5^j)."""

    def __init__(self, plan, q_first, q_count):
        self.plan = plan      # keeps a Plan alive
        self._h = _vp(None)
        handle = plan._h if isinstance(plan, Plan) else plan
        _check(lib().agx_ntt_ckks_create(ctypes.byref(self._h), handle, q_first, q_count), "ckks_create")

    def info(self):
        """(q_first, q_count, max_slots, launches_encode_ntt, launches_decode_ntt) under the plan's current variant"""
        v = [_u32(0) for _ in range(3)]
        enc, dec = _int(0), _int(0)
        _check(lib().agx_ntt_ckks_info(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(enc), ctypes.byref(dec)), "ckks_info")
        return tuple(x.value for x in v) + (enc.value, dec.value)

    def encode(self, d_z, slots, scale, d_out, batch, count, form=FORM_NTT, stream=0):
        """d_z [batch][slots] (re, im) doubles -> d_out [count][batch][n]: rint(scale w) mod q_i on the gap grid, w the inverse special FFT of z, as
        coefficients (FORM_COEFF) or transformed as Plan.forward writes it (FORM_NTT); out of place"""
        _check(lib().agx_ntt_ckks_encode(self._h, d_z, slots, scale, d_out, batch, count, form, stream), "ckks_encode")

    def decode(self, d_x, form, count, scale, d_z, slots, d_scratch, batch, stream=0):
        """d_x [count][batch][n] -> d_z [batch][slots] (re, im) doubles: the forward special FFT of the centred coefficients, over scale.  FORM_NTT: reduced
        or lazy words, d_scratch count*batch*n words or d_x itself (then overwritten); FORM_COEFF: fully reduced words, d_scratch may be None"""
        _check(lib().agx_ntt_ckks_decode(self._h, d_x, form, count, scale, d_z, slots, d_scratch, batch, stream), "ckks_decode")

    def close(self):
        if self._h:
            lib().agx_ntt_ckks_destroy(self._h)
            self._h = _vp(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KEYSWITCH_MAX_DIGITS = 16
INNER_MAX_TERMS, INNER_MAX_OUTPUTS = 16, 2


class KeySwitch:
    """One hybrid key switch (agx_ntt_keyswitch_*) on a plan: Q = primes [0, q_count), special primes [p_first, p_first + p_count) with
    p_first >= q_count, digits of alpha primes.  `plan` is a Plan or a raw plan handle (one handle per DeviceGroup shard); it must outlive
    the handle, and its device must be current here and at every call.  t: a plaintext modulus (agx_ntt_keyswitch_create_plain): every call on
    the handle then divides by P keeping the value modulo t (BGV); 1 for none."""

    def __init__(self, plan, q_count, p_first, p_count, alpha, t=1):
        self.plan = plan      # keeps a Plan alive
        self._h = _vp(None)
        handle = plan._h if isinstance(plan, Plan) else plan
        _check(lib().agx_ntt_keyswitch_create_plain(ctypes.byref(self._h), handle, q_count, p_first, p_count, alpha, t), "keyswitch_create_plain")

    def info(self):
        """(q_count, p_first, p_count, alpha, digits, launches): the shape, and the kernel launches of one apply under the plan's current variant"""
        v = [_u32(0) for _ in range(5)]
        launches = _int(0)
        _check(lib().agx_ntt_keyswitch_info(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(launches)), "keyswitch_info")
        return tuple(x.value for x in v) + (launches.value,)

    def scratch_words(self, batch):
        words = _u64(0)
        _check(lib().agx_ntt_keyswitch_scratch_words(self._h, batch, ctypes.byref(words)), "keyswitch_scratch_words")
        return words.value

    def apply(self, d_chat, d_keyhat, d_out, d_scratch, batch, stream=0):
        """d_chat [q_count][batch][n] and d_keyhat [digits][2][A][n] in NTT form (reduced or lazy) -> d_out [2][q_count][batch][n], fully
        reduced; d_scratch: scratch_words(batch) words; no two of the four may touch"""
        _check(lib().agx_ntt_keyswitch_apply(self._h, d_chat, d_keyhat, d_out, d_scratch, batch, stream), "keyswitch_apply")

    def hoisted_words(self, batch):
        """(ext, decompose_scratch, apply_scratch): the sizes in words of the buffers of decompose and apply_decomposed"""
        v = [_u64(0) for _ in range(3)]
        _check(lib().agx_ntt_keyswitch_hoisted_words(self._h, batch, *[ctypes.byref(x) for x in v]), "keyswitch_hoisted_words")
        return tuple(x.value for x in v)

    def decompose(self, d_chat, d_ext, d_scratch, batch, stream=0):
        """the half of apply that depends on the ciphertext alone: d_chat [q_count][batch][n] -> d_ext [digits][A][batch][n], every digit raised to
        the active primes in NTT form; d_scratch: q_count*batch*n words"""
        _check(lib().agx_ntt_keyswitch_decompose(self._h, d_chat, d_ext, d_scratch, batch, stream), "keyswitch_decompose")

    def apply_decomposed(self, d_ext, d_keyhat, d_out, d_scratch, batch, galois_elt, stream=0):
        """the other half, with d_ext (unchanged) read through X -> X^galois_elt: key-switches sigma_g(c) with d_keyhat, a key for sigma_g(s) -> s,
        into d_out [2][q_count][batch][n]; d_scratch: 2*A*batch*n words; galois_elt = 1 after decompose is apply word for word"""
        _check(lib().agx_ntt_keyswitch_apply_decomposed(self._h, d_ext, d_keyhat, d_out, d_scratch, batch, galois_elt, stream), "keyswitch_apply_decomposed")

    def accumulate_decomposed(self, d_ext, d_keyhat, d_acc, batch, galois_elt, d_weight=None, weight_batch=None, accumulate=False, stream=0):
        """the inner-product half of apply_decomposed alone, weighted and accumulating: d_acc [2][A][batch][n] (hoisted_words' apply scratch) = (d_acc if
        accumulate) + d_weight o sum_d pi_g(ext_d) o key_{d,o}, one launch, fully reduced; d_weight [A][weight_batch][n] (weight_batch: None = batch, or 1:
        one frame per prime), None: w = 1.  A sum of rotations is formed here and brought down once by mod_down"""
        wb = 0 if d_weight is None else batch if weight_batch is None else weight_batch
        _check(lib().agx_ntt_keyswitch_accumulate_decomposed(self._h, d_ext, d_keyhat, d_weight, wb, d_acc, batch, galois_elt, int(accumulate), stream),
               "keyswitch_accumulate_decomposed")

    def mod_down(self, d_acc, d_out, batch, stream=0):
        """the ModDown half of apply_decomposed alone: d_out [2][q_count][batch][n] <- d_acc [2][A][batch][n] divided by the special primes; the special
        slabs of d_acc are its scratch and overwritten"""
        _check(lib().agx_ntt_keyswitch_mod_down(self._h, d_acc, d_out, batch, stream), "keyswitch_mod_down")

    def hoisted_info(self):
        """(launches_decompose, launches_apply_decomposed) under the plan's current variant; their sum is info()'s launches"""
        v = [_int(0), _int(0)]
        _check(lib().agx_ntt_keyswitch_hoisted_info(self._h, ctypes.byref(v[0]), ctypes.byref(v[1])), "keyswitch_hoisted_info")
        return v[0].value, v[1].value

    def close(self):
        if self._h:
            lib().agx_ntt_keyswitch_destroy(self._h)
            self._h = _vp(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_block(num_frames, num_shards, index):
    """(first, count) of shard `index` when num_frames frames are dealt to num_shards shards (agx_ntt_shard_range: the reference's
    minibatch sizes, src/kernel/ntt.cpp:526-536, as contiguous blocks); pure arithmetic, no device needed"""
    first, count = _u64(0), _u64(0)
    _check(lib().agx_ntt_shard_range(num_frames, num_shards, index, ctypes.byref(first), ctypes.byref(count)), "shard_range")
    return first.value, count.value


class DeviceGroup:
    """One shard (plan + stream + staging + host thread) per entry of `devices` (agx_ntt_group_*): host frames are dealt in contiguous
    blocks, device-pointer calls take one pointer per shard.  No collective anywhere."""

    def __init__(self, devices, n, moduli, psi=None, tables=None):
        self.n = int(n)
        self.devices = [int(d) for d in devices]
        self.moduli = [int(q) for q in moduli]
        devs = (_int * len(self.devices))(*self.devices)
        self._h = _vp(None)
        create, where = (lib().agx_ntt_group_create_auto, "group_create_auto") if tables is None else (lib().agx_ntt_group_create, "group_create")
        _check(create(ctypes.byref(self._h), devs, len(self.devices), self.n, len(self.moduli), *_table_args(self.moduli, psi, tables)), where)

    @property
    def num_shards(self):
        return len(self.devices)

    def shard(self, index):
        """(device, plan handle, stream handle) of shard `index`; the handles belong to the group"""
        dev, plan, stream = _int(0), _vp(None), _vp(None)
        _check(lib().agx_ntt_group_shard(self._h, index, ctypes.byref(dev), ctypes.byref(plan), ctypes.byref(stream)), "group_shard")
        return dev.value, plan.value, stream.value

    def forward_host(self, in1, in2, num_frames, out=None):
        out = _out_array(out, num_frames * self.n)
        _check(lib().agx_ntt_group_forward_host(self._h, _np_ptr(in1), _np_ptr(in2), _np_ptr(out), num_frames), "group_forward_host")
        return out

    def inverse_host(self, in1, num_frames, out=None):
        out = _out_array(out, num_frames * self.n)
        _check(lib().agx_ntt_group_inverse_host(self._h, _np_ptr(in1), _np_ptr(out), num_frames), "group_inverse_host")
        return out

    def _ptrs(self, ptrs):
        return None if ptrs is None else (_vp * self.num_shards)(*[int(p) if p else None for p in ptrs])

    def _batches(self, batch):
        return (_u64 * self.num_shards)(*[int(b) for b in batch])

    def forward(self, d_in, d_out, batch):
        _check(lib().agx_ntt_group_forward(self._h, self._ptrs(d_in), self._ptrs(d_out), self._batches(batch)), "group_forward")

    def inverse(self, d_in, d_out, batch):
        _check(lib().agx_ntt_group_inverse(self._h, self._ptrs(d_in), self._ptrs(d_out), self._batches(batch)), "group_inverse")

    def polymul(self, d_a, d_b, d_c, batch, d_scratch=None):
        _check(lib().agx_ntt_group_polymul(self._h, self._ptrs(d_a), self._ptrs(d_b), self._ptrs(d_c), self._ptrs(d_scratch), self._batches(batch)), "group_polymul")

    def polymul_ntt(self, d_a, d_bhat, d_c, batch, bhat_batch=None):
        """per shard as Plan.polymul_ntt; bhat_batch: None = batch, or one entry (batch[i] or 1) per shard"""
        _check(lib().agx_ntt_group_polymul_ntt(self._h, self._ptrs(d_a), self._ptrs(d_bhat), self._ptrs(d_c), self._batches(batch),
                                               self._batches(batch if bhat_batch is None else bhat_batch)), "group_polymul_ntt")

    def rescale(self, d_x, d_out, d_scratch, batch, mode=RESCALE_ROUND):
        """per shard as Plan.rescale"""
        _check(lib().agx_ntt_group_rescale(self._h, self._ptrs(d_x), self._ptrs(d_out), self._ptrs(d_scratch), self._batches(batch), mode), "group_rescale")

    def automorphism(self, d_in, d_out, batch, galois_elt, form=FORM_NTT):
        """per shard as Plan.automorphism"""
        _check(lib().agx_ntt_group_automorphism(self._h, self._ptrs(d_in), self._ptrs(d_out), self._batches(batch), galois_elt, form), "group_automorphism")

    def synchronize(self):
        _check(lib().agx_ntt_group_synchronize(self._h), "group_synchronize")

    def close(self):
        if self._h:
            lib().agx_ntt_group_destroy(self._h)
            self._h = _vp(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# sharding of independent frames over ranks lives in distributed.py (no collective on the data path)
from .distributed import Group, aggregate_throughput, shard_range  # noqa: E402,F401
