"""agx_ntt_keyswitch_accumulate_decomposed and agx_ntt_mul_add_galois at a size where the grid-stride loop takes a second step (a launch holds at most
16,384 blocks of 256 threads per grid row: TRIP work items), in the 16-byte form and in the 8-byte form.  The moduli are 30-bit primes, so every word is
judged on the device in int64: a product of residues stays below 2^60, the sum of two below 2^61, and old + w t below 2^60 + 2^30."""
import pytest

from gpu_util import moduli_for, ntt_pi, plan_for_moduli
from rns_cases import TRIP

pytestmark = pytest.mark.gpu

N, G = 4096, 5


def _lazy(torch, dev, moduli, frames, seed, shift=0):
    """[len(moduli)][frames][N] words uniform in [0, 4q) on the device behind `shift` words of padding: (the tensor, its view without the padding)"""
    g = torch.Generator(device=dev.device)
    g.manual_seed(seed)
    t = dev.empty(shift + len(moduli) * frames * N)
    v = t[shift:].view(len(moduli), frames * N)
    for i, q in enumerate(moduli):
        v[i] = torch.randint(0, 4 * int(q), (frames * N,), generator=g, device=dev.device, dtype=torch.int64)
    return t, t[shift:].view(len(moduli), frames, N)


def _accumulate_second_step(agx, orc, dev, batch, shift):
    """shape (2, 2, 1, 1): Q two primes, one special prime, two digits; a one-frame weight, accumulating onto lazy old words; shift: 0 = every base 16-byte
    aligned (the pair form), 1 = every base 8 bytes further (the word form)"""
    torch = dev.torch
    moduli = tuple(moduli_for(orc.find_prime, N, [30] * 3))
    plan, _ = plan_for_moduli(agx, orc, N, moduli, inverse=False)
    ks = plan.keyswitch(2, 2, 1, 1)
    A, D = 3, 2
    d_ext, ext = _lazy(torch, dev, moduli * D, batch, 1, shift)            # [D][A][batch][n]
    d_key, key = _lazy(torch, dev, moduli * (2 * D), 1, 2, shift)          # [D][2][A][1][n]
    d_w, w = _lazy(torch, dev, moduli, 1, 3, shift)                        # [A][1][n]
    d_acc, acc = _lazy(torch, dev, moduli * 2, batch, 4, shift)            # [2][A][batch][n]
    assert all(t.data_ptr() % 16 == 0 for t in (d_ext, d_key, d_w, d_acc))
    assert ks.hoisted_words(batch) == (D * A * batch * N, 2 * batch * N, 2 * A * batch * N)
    old = acc.clone()
    guard = torch.full((1,), -1, dtype=torch.int64, device=dev.device)
    if shift:
        d_acc[0] = -1
    at = lambda t: t.data_ptr() + 8 * shift      # noqa: E731
    ks.accumulate_decomposed(at(d_ext), at(d_key), at(d_acc), batch, G, at(d_w), 1, True, dev.stream)
    dev.sync()
    pi = torch.from_numpy(ntt_pi(N, G)).to(dev.device)
    ev, kv, av, ov = ext.view(D, A, batch, N), key.view(D, 2, A, 1, N), acc.view(2, A, batch, N), old.view(2, A, batch, N)
    for j, q in enumerate(moduli):
        q = int(q)
        for o in range(2):
            t = ((ev[0, j] % q)[:, pi] * (kv[0, o, j] % q) + (ev[1, j] % q)[:, pi] * (kv[1, o, j] % q)) % q
            want = (ov[o, j] % q + (w[j] % q) * t) % q
            if not torch.equal(av[o, j], want):
                pytest.fail(f"output {o}, slot {j}: first differing (frame, word) {(av[o, j] != want).nonzero()[:4].tolist()}")
    if shift:
        assert int(d_acc[0]) == int(guard[0]), "the word in front of acc changed"
    ks.close()
    plan.close()


def test_accumulate_second_step_pair_form_every_word(agx, orc, dev):
    """2048 pairs per frame: 2,049 frames are the fewest whose per-slot work passes one trip of the 16-byte form"""
    batch = TRIP // (N // 2) + 1
    assert batch == 2049
    _accumulate_second_step(agx, orc, dev, batch, 0)


def test_accumulate_second_step_word_form_every_word(agx, orc, dev):
    """every base offset by 8 bytes: one word per work item, so 1,025 frames are the fewest past one trip"""
    batch = TRIP // N + 1
    assert batch == 1025
    _accumulate_second_step(agx, orc, dev, batch, 1)


def _mul_add_second_step(agx, orc, dev, batch, shift):
    """two of three 30-bit primes (the range (1, 2)), a one-frame weight, g = 5, accumulating onto lazy old words"""
    torch = dev.torch
    moduli = tuple(moduli_for(orc.find_prime, N, [30] * 3))
    plan, _ = plan_for_moduli(agx, orc, N, moduli, inverse=False)
    sub = moduli[1:]
    d_w, w = _lazy(torch, dev, sub, 1, 5, shift)
    d_b, b = _lazy(torch, dev, sub, batch, 6, shift)
    d_c, c = _lazy(torch, dev, sub, batch, 7, shift)
    assert all(t.data_ptr() % 16 == 0 for t in (d_w, d_b, d_c))
    old = c.clone()
    if shift:
        d_c[0] = -1
    at = lambda t: t.data_ptr() + 8 * shift      # noqa: E731
    plan.mul_add_galois(at(d_w), at(d_b), at(d_c), batch, G, 1, True, 1, 2, dev.stream)
    dev.sync()
    pi = torch.from_numpy(ntt_pi(N, G)).to(dev.device)
    for p, q in enumerate(sub):
        q = int(q)
        want = (old[p] % q + (w[p] % q) * (b[p] % q)[:, pi]) % q
        if not torch.equal(c[p], want):
            pytest.fail(f"prime {p}: first differing (frame, word) {(c[p] != want).nonzero()[:4].tolist()}")
    if shift:
        assert int(d_c[0]) == -1, "the word in front of c changed"
    plan.close()


def test_mul_add_second_step_pair_form_every_word(agx, orc, dev):
    _mul_add_second_step(agx, orc, dev, TRIP // (N // 2) + 1, 0)


def test_mul_add_second_step_word_form_every_word(agx, orc, dev):
    _mul_add_second_step(agx, orc, dev, TRIP // N + 1, 1)
