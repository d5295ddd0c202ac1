"""Self-test of the guarded-arena helpers of gpu_util.py, on the CPU: a stand-in "kernel" applies the oracle's forward transform to the
frames of a host arena, once correctly and once per planted fault; the checker must pass the correct run and name the word of every
fault.  The GPU layout tests (test_gpu_layouts.py) rely on exactly these helpers, so this shows that they can fail."""
import numpy as np
import pytest

from gpu_util import GuardedArena, Layout, arena_faults, arena_for, canary, gather_frames, rand_coeffs, splitmix64, tables_for

N, PRIMES, BATCH = 64, 2, 5


def _standin_forward(orc, tabs, src, src_layout, dst, dst_layout, fault=None):
    """what a strided forward launch does, on host arenas: read the frames of src at src_layout, transform them per prime, write them to
    dst at dst_layout.  fault = (arena, payload index): one more word is written there, as a kernel with a wrong mask would."""
    x = src.frames(src_layout).reshape(src_layout.primes, -1)
    y = np.stack([orc.forward(x[p], t[0], t[2], t[3], src_layout.n) for p, t in enumerate(tabs)])
    dst.place(dst_layout, y)
    if fault is not None:
        arena, index = fault
        arena.words[arena.band + index] ^= np.uint64(1)
    return y.reshape(-1)


def _padded(offset=0):
    return Layout(N, PRIMES, BATCH, prime_stride=BATCH * (N + 1) + 3, poly_stride=N + 1, offset=offset)


def test_canary_is_position_dependent_and_above_every_residue():
    c = canary(0, 1 << 16)
    assert (c >= np.uint64(1 << 63)).all()
    assert np.unique(c).size == c.size
    assert np.array_equal(canary(1000, 24), c[1000:1024])
    # splitmix64's published first outputs for seed 0 are the outputs of states gamma, 2 gamma, ...: index i here is state i + gamma
    assert int(splitmix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF


def test_layout_places_and_gathers_frames():
    lay = Layout(8, 2, 3, prime_stride=40, poly_stride=11, offset=1)
    assert lay.starts().tolist() == [[1, 12, 23], [41, 52, 63]]
    assert lay.span() == 71
    frames = np.arange(2 * 3 * 8, dtype=np.uint64)
    arena = GuardedArena(8, lay.span()).place(lay, frames)
    assert arena.band == 4096 and arena.words.size == 2 * 4096 + 71
    assert np.array_equal(arena.words[4096 + 12:4096 + 20], frames[8:16])
    assert np.array_equal(arena.frames(lay), frames)
    assert np.array_equal(gather_frames(arena.words, arena.band, lay), frames)
    assert arena.address(1) == arena.words.ctypes.data + 8 * 4097
    dense = Layout(8, 2, 3)
    assert (dense.prime_stride, dense.poly_stride, dense.span()) == (24, 8, 48)
    assert dense.at(1).starts()[1, 2] == 1 + 24 + 16


def test_checker_passes_a_correct_run(orc):
    tabs = tables_for(orc, N, 60, PRIMES)
    rng = np.random.default_rng(1)
    x = np.concatenate([rand_coeffs(rng, BATCH * N, t[0], hi_mult=4) for t in tabs])
    lin, lout = _padded(offset=1), _padded(offset=0)
    src, dst = arena_for(None, N, (lin, x)), arena_for(None, N, (lout, None))
    want = _standin_forward(orc, tabs, src, lin, dst, lout)
    assert dst.faults([(lout, None)]) == []
    assert dst.faults([(lout, want)]) == []
    assert src.faults([(lin, x)]) == []
    assert np.array_equal(dst.frames(lout), want)
    # in place, and the interleaved layout (input and output frames alternate in one arena)
    a_in = Layout(N, PRIMES, BATCH, prime_stride=2 * BATCH * N, poly_stride=2 * N, offset=0)
    a_out = a_in.at(N)
    both = arena_for(None, N, (a_in, x), (a_out, None))
    want = _standin_forward(orc, tabs, both, a_in, both, a_out)
    assert both.faults([(a_in, x), (a_out, want)]) == []


FAULTS = [
    # (what, arena, payload index of the planted word, nearest frame (prime, frame), position relative to that frame)
    ("one word behind the last frame", "dst", lambda lay: lay.span(), (PRIMES - 1, BATCH - 1), N),
    ("one word in the gap between two frames", "dst", lambda lay: int(lay.starts()[0, 2]) + N, (0, 2), N),
    ("one word in the gap between two primes", "dst", lambda lay: int(lay.starts()[1, 0]) - 2, (1, 0), -2),
    ("one word before the first frame", "dst", lambda lay: lay.offset - 1, (0, 0), -1),
    ("one word deep in the leading band", "dst", lambda lay: -4000, (0, 0), -4000 - 1),
    ("one input word flipped by an out-of-place call", "src", lambda lay: int(lay.starts()[1, 3]) + 17, (1, 3), 17),
]


@pytest.mark.parametrize("what,where,index_of,owner,rel", FAULTS, ids=[f[0].replace(" ", "_") for f in FAULTS])
def test_checker_names_every_planted_fault(orc, what, where, index_of, owner, rel):
    tabs = tables_for(orc, N, 60, PRIMES)
    rng = np.random.default_rng(2)
    x = np.concatenate([rand_coeffs(rng, BATCH * N, t[0], hi_mult=4) for t in tabs])
    lay = _padded(offset=1)
    src, dst = arena_for(None, N, (lay, x)), arena_for(None, N, (lay, None))
    index = index_of(lay)
    want = _standin_forward(orc, tabs, src, lay, dst, lay, fault=(src if where == "src" else dst, index))
    assert np.array_equal(dst.frames(lay), want), "the planted fault lies outside the output frames: their values alone show nothing"
    faults = (src.faults([(lay, x)]) if where == "src" else dst.faults([(lay, None)]))
    assert len(faults) == 1, what
    f = faults[0]
    assert f["index"] == index, what
    assert (f["prime"], f["frame"], f["rel"]) == (*owner, rel), what
    assert f["got"] == f["want"] ^ 1
    clean = dst if where == "src" else src
    assert clean.faults([(lay, None)]) == []


def test_checker_reports_the_first_few_faults_only():
    lay = Layout(16, 1, 2, poly_stride=20)
    arena = GuardedArena(16, lay.span())
    arena.words[arena.band + 16:arena.band + 20] = 0
    arena.words[-1] = 0
    got = arena_faults(arena.words, arena.band, [(lay, None)], limit=3)
    assert [f["index"] for f in got] == [16, 17, 18]
    assert [(f["frame"], f["rel"]) for f in got] == [(0, 16), (0, 17), (1, -2)]
    assert arena_faults(arena.words, arena.band, [(lay, None)], limit=8)[-1]["index"] == lay.span() + arena.band - 1
