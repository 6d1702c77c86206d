"""The fp64 reference of the acting kernels (tests/acting_reference.py) against facts that do not come from the kernels: the uniforms'
boundary words, N(0, 1) moments, the keying of the draws, the packed weight layout of include/pgtt_train.h and the bookkeeping rule.  No
GPU; test_gpu_acting_edges.py then holds policy_act_kernel and rollout_record_kernel to the same reference."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acting_reference as ref  # noqa: E402

from phase_guided_terrain_traversal_amd import acting  # noqa: E402

SEED = 0x9E3779B97F4A7C15


def test_uniform_boundary_words():
    """w0 >> 8 == 2^24 - 1: the + 0.5f ties to even, u1 == 1, r == 0, both draws 0.  w0 >> 8 == 0: u1 = 2^-25 (never 0), r = sqrt(50 ln 2).
    An odd w0 >> 8 above 2^23 goes to the even neighbour.  u2 < 1 for every word."""
    top = np.uint32(0xFFFFFFFF)
    for w0 in (top, np.uint32(0xFFFFFF00)):
        u1, _ = ref.uniforms(w0, np.uint32(0x12345678))
        r, even, odd = ref.box_muller(w0, np.uint32(0x12345678))
        assert u1 == np.float32(1.0) and r == 0.0 and even == 0.0 and odd == 0.0
    for w0 in (np.uint32(0), np.uint32(0xFF)):
        u1, _ = ref.uniforms(w0, top)
        r, _, _ = ref.box_muller(w0, top)
        assert float(u1) == 2.0 ** -25 and abs(r - math.sqrt(50 * math.log(2))) < 1e-14
    odd_m = 2 ** 23 + 1                                  # m + 0.5 lies half way between m and m + 1 = 2^23 + 2, the even one
    u1, _ = ref.uniforms(np.uint32(odd_m << 8), np.uint32(0))
    assert float(u1) == (2 ** 23 + 2) * 2.0 ** -24
    u1, _ = ref.uniforms(np.uint32((odd_m + 1) << 8), np.uint32(0))          # an even m stays
    assert float(u1) == (2 ** 23 + 2) * 2.0 ** -24
    u1, _ = ref.uniforms(np.uint32((2 ** 23 - 1) << 8), np.uint32(0))        # below 2^23 the half is representable
    assert float(u1) == (2 ** 23 - 0.5) * 2.0 ** -24
    _, u2 = ref.uniforms(np.uint32(0), top)
    assert float(u2) == 1.0 - 2.0 ** -24
    w = np.random.default_rng(0).integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)
    u1, u2 = ref.uniforms(w, w[::-1])
    assert float(u2.max()) < 1.0 and float(u2.min()) >= 0.0 and float(u1.min()) > 0.0 and float(u1.max()) <= 1.0


def test_draws_have_standard_normal_moments():
    """2^16 Philox blocks = 2^17 draws: mean, second, third and fourth moment within five standard errors of N(0, 1) (variances 1, 2, 15, 96),
    the two halves of a Box-Muller pair uncorrelated (the product of two independent N(0, 1) has variance 1)"""
    n = -(-2 ** 16 // 6)
    eps, _ = ref.draws(SEED, 0, 0, n)
    pairs = eps.reshape(-1, 2)[:2 ** 16]
    x = pairs.reshape(-1)
    m = x.size
    assert m == 2 ** 17
    assert abs(x.mean()) < 5 * math.sqrt(1.0 / m)
    assert abs((x ** 2).mean() - 1.0) < 5 * math.sqrt(2.0 / m)
    assert abs((x ** 3).mean()) < 5 * math.sqrt(15.0 / m)
    assert abs((x ** 4).mean() - 3.0) < 5 * math.sqrt(96.0 / m)
    assert abs((pairs[:, 0] * pairs[:, 1]).mean()) < 5 * math.sqrt(1.0 / (m // 2))


def test_draws_are_paired_and_keyed_by_every_input():
    """actuators 2k and 2k + 1 share a block (eps^2 + eps^2 == r^2); seed low and high word, env id, draw-counter low and high word each
    change every draw; an env-id offset is a shift of the rows, modulo 2^32"""
    n = 64
    eps, r = ref.draws(SEED, 5, 7, n)
    assert eps.shape == (n, 12) and r.shape == (n, 12)
    assert np.array_equal(r[:, 0::2], r[:, 1::2])
    np.testing.assert_allclose(eps[:, 0::2] ** 2 + eps[:, 1::2] ** 2, r[:, 0::2] ** 2, rtol=1e-13, atol=0)
    assert len(np.unique(eps)) == eps.size                      # six different blocks per env
    for other in ((SEED ^ 1, 5, 7), (SEED ^ (1 << 32), 5, 7), (SEED & 0xFFFFFFFF, 5, 7), (SEED, 6 + n, 7), (SEED, 5, 8), (SEED, 5, 7 + 2 ** 32),
                  (SEED, 5, 7 + 2 ** 40)):
        e2, _ = ref.draws(*other, n)
        assert np.all(e2 != eps), other
    e2, _ = ref.draws(SEED, 6, 7, n)
    assert np.array_equal(e2[:-1], eps[1:])
    e2, _ = ref.draws(SEED, 5 + 2 ** 32, 7, n)
    assert np.array_equal(e2, eps)
    c = ref.counters_of(2 ** 31 + 5, 2 ** 40 + 3, 3)
    assert c[2, 4].tolist() == [2 ** 31 + 7, 3, 0x100 ^ 0x50475454, 4]


@pytest.mark.parametrize("k", [1, 15, 17, 176, 177, 209, 224])
def test_pack_linear_is_inverted_by_the_headers_index_formula(k):
    """a layer [out][in] is zero-padded to multiples of 16 and stored as [out / 16][in / 16][g][i][s] = W[16 tile + i][16 kb + 4 g + s]"""
    for n in (512, 24):
        w = torch.arange(1, n * k + 1, dtype=torch.float32).reshape(n, k)
        b = torch.arange(1, n + 1, dtype=torch.float32)
        p, pb = acting.pack_linear(w, b)
        npad, kpad = -(-n // 16) * 16, -(-k // 16) * 16
        assert p.numel() == npad * kpad and pb.numel() == npad
        p = p.numpy()
        W = np.zeros((npad, kpad), np.float32)
        idx = np.arange(p.size)
        s, i, g = idx % 4, (idx // 4) % 16, (idx // 64) % 4
        kb, tile = (idx // 256) % (kpad // 16), idx // (256 * (kpad // 16))
        W[16 * tile + i, 16 * kb + 4 * g + s] = p
        assert np.array_equal(W[:n, :k], w.numpy())
        assert not W[n:].any() and not W[:, k:].any()
        assert np.array_equal(pb.numpy()[:n], b.numpy()) and not pb.numpy()[n:].any()


def test_record_reference_is_the_rule():
    rng = np.random.default_rng(3)
    n, L, T = 500, 13, 4
    reward, up_z = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    done = (rng.random(n) < 0.2).astype(np.float32)
    steps = rng.integers(L - 2, L + 3, n).astype(np.int32)
    epm = rng.normal(size=(24, n)).astype(np.float32)
    sums0 = rng.normal(size=25)
    out = ref.record(reward, done, steps, up_z, epm, 0.5, L, T, [2, 9], sums0)
    d = done.astype(bool)
    want = sums0 + np.concatenate([epm.astype(np.float64)[:, d].sum(1), [d.sum()]])
    np.testing.assert_allclose(out["episode_sums"], want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(out["trunc"], ((steps >= L) & (up_z >= 0)).astype(np.float64)) and 0 < out["trunc"].sum() < n
    assert np.array_equal(out["rew"], reward.astype(np.float64) * 0.5) and np.array_equal(out["done"], done)
    assert out["row"] == 2 and out["counters"].tolist() == [3, 10]
    for t in (-1, T, 2 ** 33):
        o = ref.record(reward, done, steps, up_z, epm, 0.5, L, T, [t, 2 ** 40], sums0)
        assert o["row"] is None and o["counters"].tolist() == [t + 1, 2 ** 40 + 1] and np.array_equal(o["episode_sums"], out["episode_sums"])
    z = ref.record(reward, np.zeros(n), steps, np.full(n, -0.0), epm, 0.5, L, T, [0, 0], sums0)
    assert np.array_equal(z["episode_sums"], sums0) and np.array_equal(z["trunc"], (steps >= L).astype(np.float64))
