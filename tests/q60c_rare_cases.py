"""What tests/test_q60c_rare_sub_model.py (CPU), tests/test_gpu_fwd_q60c_rare_sub.py and its child tests/q60c_rare_diag_child.py share: the rule of the
rare last subtract of the n = 4096 forward kernels behind registry id 165 (csrc/modarith.hpp: q60c_tail_bounds, csrc/rb_frame.hpp: kOptQ60cRareSub), in
Python integers, and the frames that force it.

The kernel's last stage leaves every output at t = (v mod 2^60) + (v >> 60) c (reduce_top4, q = 2^60 - c), flags the outputs whose high word is at least
0x0FFFFFFF, and subtracts q -- conditionally, from every register -- only in a wave (2,048 consecutive outputs of a frame) with a flag.  A flag is due
when t >= q, which takes a fully reduced output below 16c (t <= 2^60 - 1 + 15c = q + 16c - 1): never on random residues, so the frames here are built to have such outputs."""
import numpy as np

from q60c_skip_cases import N, reduce_top4

TAIL_HI = 0x0FFFFFFF
WAVE_OUTPUTS = 2048      # the outputs one wave of the 128-thread workgroup stores: [0, 2048) and [2048, 4096) of a frame


def flagged(t):
    """the kernel's 32-bit compare"""
    return (t >> 32) >= TAIL_HI


def csub_q(t, q):
    """csub_select_c(t, 2^64 - q): d = t - q mod 2^64, kept unless its sign bit is set"""
    d = (t - q) % (1 << 64)
    return t if d >> 63 else d


def finish_wave(ts, q):
    """what a wave does with its outputs t: the subtract over all of them if any is flagged, nothing otherwise"""
    return [csub_q(t, q) for t in ts] if any(flagged(t) for t in ts) else list(ts)


def constant_terms(q):
    """a frame whose only non-zero coefficient is the constant term a has a in every output"""
    c = (1 << 60) - q
    return (1, c - 1, c, 15 * c - 1, q - 1)


def forced_frames(q):
    """an all-zero frame (every output is a multiple of q) and one frame per constant term: 6 frames, every lane of both waves takes the cold block"""
    x = np.zeros((1 + len(constant_terms(q)), N), dtype=np.uint64)
    for i, a in enumerate(constant_terms(q)):
        x[1 + i, 0] = a
    return x.reshape(-1)


def planted_outputs(rng, q):
    """three output vectors with entries in [16c, 0x0FFFFFFF 2^32): t < q and no flag, whatever multiple of q the kernel's word carries.  The first gets
    a 0 and a q - 1 among the outputs of wave 0, the second among those of wave 1 (that wave takes the cold block, the other does not); the third keeps
    none, so both waves store t as it is"""
    c = (1 << 60) - q
    y = rng.integers(16 * c, TAIL_HI << 32, size=(3, N), dtype=np.uint64)
    for frame, lo in ((0, 0), (1, WAVE_OUTPUTS)):
        at = lo + rng.choice(WAVE_OUTPUTS, size=2, replace=False)
        y[frame, at[0]] = 0
        y[frame, at[1]] = q - 1
    return y


def planted_frames(orc, rng, q, psi):
    """the inputs whose transform is planted_outputs(): the oracle's inverse transform of them"""
    itw, _ = orc.make_inv_tables(q, psi, N)
    y = planted_outputs(rng, q)
    return orc.inverse(y.reshape(-1), q, itw, N), y.reshape(-1)


__all__ = ["N", "TAIL_HI", "WAVE_OUTPUTS", "reduce_top4", "flagged", "csub_q", "finish_wave", "constant_terms", "forced_frames", "planted_outputs",
           "planted_frames"]
