"""libpgtt_perceive.so on the GPU at the sizes its contract allows (tests/perceive_edge_cases.py builds the cases, tests/test_perceive_edge_cases.py
checks them without a GPU): 64 channels, K = 1600 = the offset table's size, one, two and three convs, stride 1 first layers, an image and a pair
of activations at the LDS budget, images 256 wide and 256 tall, a one-pixel conv output, 64 prop_rows, Kin of 255, 256 and 257, hidden widths of
16, 128, 144, 272 and 512, obs_dim = 117 with scan_row0 = 0, duplicate prop_rows and prop_rows inside the scan rows, 1, 15, 16, 17 and 33 envs, a
head loop of 233 chunks - through perceive.StudentPerception and, for the host checks, the bare C ABI.

1. Exact cases: one dense layer at a time, every other layer a pass-through, every value a half-integer fp32 holds exactly: `latent`, `est` and
   `obs_out` equal the integer expectation as bits, the rows of obs_out outside the scan rows equal obs as bits, the guard bands stay.
2. Rounding cases: He-initialised weights against fp64 with the bar per element that perceive_edge_cases.bars() carries through the layers.  That
   the bar holds for the reference alone was checked on the CPU before the kernel met it (tests/test_perceive_edge_cases.py asserts it on every
   run): torch's fp32 forward of the same nets, weights and inputs gives a worst error / bar (latent, est) of
       deep5 6.80e-06, 4.16e-08    budget1 1.40e-01, 1.95e-07    budget3 3.16e-05, 2.23e-08    min3 1.33e-01, 1.36e-03
       wide 6.72e-02, 2.73e-05     tall 7.10e-02, 6.78e-06       two 2.25e-03, 5.26e-07        allscan 4.95e-02, 1.75e-04
       deep5:1 6.01e-02, 1.23e-06  deep5:2 4.49e-04, 1.76e-07    budget3:1 6.58e-02, 1.17e-06  budget3:2 1.10e-03, 3.49e-07
       two:1 9.91e-02, 1.53e-06    deep5-k255 6.80e-06, 5.42e-08 deep5-k257 2.59e-04, 4.44e-07 wide-h16 7.42e-02, 6.11e-05
       allscan-h128 4.95e-02, 3.19e-04
   all at most 1.  A worst-case bar grows with every layer it is carried through (a K = 1600 conv multiplies it by sum |w|, some 45), so behind three
   such layers it is loose; the project's forward bar, 2e-5 * (1 + max|want|) per tensor, is therefore asserted beside it: the same CPU run
   gives between 0.0046 and 0.0251 of it for every net above.  On an MI355X the kernels give (latent, est) of the per-element bar
       deep5 1.77e-05, 7.53e-08    budget1 1.40e-01, 5.64e-07    budget3 4.66e-05, 7.19e-08    min3 1.33e-01, 2.76e-03
       wide 6.72e-02, 4.10e-05     tall 7.10e-02, 2.79e-05       two 5.04e-03, 2.47e-06        allscan 4.95e-02, 2.53e-04
       deep5:1 6.01e-02, 5.92e-06  deep5:2 1.86e-03, 4.60e-07    budget3:1 6.58e-02, 6.26e-06  budget3:2 4.36e-03, 9.80e-07
       two:1 1.11e-01, 7.83e-06    deep5-k255 1.77e-05, 8.20e-08 deep5-k257 7.23e-04, 9.16e-07 wide-h16 7.42e-02, 1.63e-04
       allscan-h128 4.95e-02, 2.71e-04
   and between 0.0050 and 0.0760 of the forward bar.  How loose the carried bar is behind deep layers was measured: a library built with the last
   four of the 1600 products of a K = 1600 conv dropped stays inside it on deep5 (0.84 and 0.0012) and is 1348 and 337 times outside the forward
   bar; the exact cases deep5/conv1 and deep5/conv2 fail on it bit for bit.
3. The recurrent twins: the same envelope through pgtt_perceive_recurrent against tests/perceive_memory_reference.py with the bar of
   tests/test_gpu_perceive_memory.py, memory 16 and 256, one tick from a random memory and one with clear_all; one exact case per net (u = 1: m1 is
   m0 as bits, est = W_out m0 + b_out in integers, a cleared env gives b_out and a zero memory); batch independence of both heads in a batch of 33.
   On an MI355X the worst error / bar of the recurrent rounding cases is 0.031 (deep5, the latent).
4. The host checks agree: perceive.check_config and pgtt_perceive_check on 2000 random configs, and what an accepted config comes to.

What the suite notices.  Six libraries were built from sources with one statement altered each, every one of them in bounds, and run against this
module and against the forward, edge, guard, batch and clear tests of test_gpu_perceive.py and test_gpu_perceive_memory.py:
    the last k-step of a conv with K = 1600 dropped               12 cases here fail (every dense K = 1600 conv, bit for bit)    the others pass
    tile 16 of a hidden layer of 17 tiles read as zero             4 cases here fail (every `tall` case)                         the others pass
    prop_rows 62 and 63 exchanged                                 11 cases here fail (every dense fc1 and fc2 behind 64 rows)    the others pass
    m1 = n + u (m0 - n) for (1 - u) n + u m0 in the cell            7 of the 8 recurrent exact cases fail                         the others pass
    z[256] read as zero by the plain head                         25 cases here fail                                             4 of the others fail
    z[256] read as zero by the recurrent head                      8 cases here fail (recurrent rounding, every Kin > 256)       6 of the others fail
No kernel was changed: every case passes on the library as it is."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perceive_edge_cases as pc  # noqa: E402
import perceive_memory_reference as mref  # noqa: E402

from phase_guided_terrain_traversal_amd import acting, perceive  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 12345.25                                                       # no half-integer: never an exact case's value
PAD = 61                                                               # an odd offset: no output is 16-byte aligned


def fake_env(cfg, depth, obs):
    """what StudentPerception reads of an env: the image, the observation, the device"""
    d, o = torch.from_numpy(depth).cuda(), torch.from_numpy(obs).cuda()
    return types.SimpleNamespace(depth=d, depth_camera=types.SimpleNamespace(height=cfg["height"], width=cfg["width"]), buffers={"obs_state": o},
                                 device=d.device, num_envs=d.shape[0], observation_size={"state": cfg["obs_dim"]})


class Rig:
    """a StudentPerception whose outputs (and memory) are views into larger allocations of a sentinel, with guard bands on both sides"""

    def __init__(self, cfg, est, depth, obs, mem=None):
        self.cfg, self.n = cfg, len(depth)
        self.sp = perceive.StudentPerception(fake_env(cfg, depth, obs), est)
        self.widths = {"latent": est.latent_dim, "est": 117, "obs": cfg["obs_dim"]}
        if est.memory:
            self.widths["mem"] = est.memory
        self.bufs = {k: torch.full((PAD + self.n * w + PAD,), GUARD, device="cuda") for k, w in self.widths.items()}
        for k, w in self.widths.items():
            setattr(self.sp, k, self.bufs[k][PAD:PAD + self.n * w].view(self.n, w))
        if est.memory:
            self.sp.mem.copy_(torch.from_numpy(np.asarray(mem, np.float32)))
        self.sp.bind()

    def tick(self, **kw):
        """-> {"latent", "est", "obs", "mem"} as numpy; every output written, every guard band intact"""
        self.sp.tick(**kw)
        torch.cuda.synchronize()
        for k, t in self.bufs.items():
            assert (t[:PAD] == GUARD).all() and (t[-PAD:] == GUARD).all(), k
            assert (t[PAD:-PAD] != GUARD).all(), k
        return {k: getattr(self.sp, k).cpu().numpy() for k in self.widths}

    def close(self):
        self.sp.close()


def run(cfg, est, depth, obs, mem=None, **kw):
    rig = Rig(cfg, est, depth, obs, mem)
    out = rig.tick(**kw)
    rig.close()
    return out


def outside_scan_rows_is_obs(cfg, out, obs):
    r0 = cfg["scan_row0"]
    return np.array_equal(pc.bits(out[:, :r0]), pc.bits(obs[:, :r0])) and np.array_equal(pc.bits(out[:, r0 + 117:]), pc.bits(obs[:, r0 + 117:]))


def within(name, got, want):
    """tests/test_gpu_perceive_memory.py's bar"""
    err, bar = np.abs(got - want).max(), 2e-5 * (1 + np.abs(want).max())
    print(f"{name}: max error {err:.3e}, bar {bar:.3e}, ratio {err / bar:.3f}")
    assert np.isfinite(got).all() and err < bar, (name, err, bar)


# ---------------------------------------------------------------- 1. exact cases
@pytest.mark.parametrize("name", pc.exact_names())
def test_exact_case(name):
    c = pc.exact_case(name)
    got = run(c["cfg"], pc.estimator_of(c), c["depth"], c["obs"])
    for key, g in (("latent", got["latent"]), ("est", got["est"]), ("obs_out", got["obs"])):
        msg = pc.where_wrong(c, key, g)
        assert not msg, msg
    assert outside_scan_rows_is_obs(c["cfg"], got["obs"], c["obs"])


# ---------------------------------------------------------------- 2. rounding cases
@pytest.mark.parametrize("name", pc.ROUNDING)
def test_rounding_case(name):
    cfg, est, depth, obs = pc.rounding_case(name)
    got = run(cfg, est, depth, obs)
    assert all(np.isfinite(v).all() for v in got.values())
    rl, re, fl, fe = pc.ratios(cfg, pc.net_of(est), depth, obs, got["latent"], got["est"])
    print(f"{name} (N = {len(depth)}): worst error / bar: latent {rl:.2e}, est {re:.2e}; against the forward bar 2e-5 (1 + max|want|): {fl:.4f}, {fe:.4f}")
    assert rl <= 1.0 and re <= 1.0
    assert fl < 1.0 and fe < 1.0
    r0 = cfg["scan_row0"]
    assert np.array_equal(pc.bits(got["obs"][:, r0:r0 + 117]), pc.bits(got["est"])) and outside_scan_rows_is_obs(cfg, got["obs"], obs)


# ---------------------------------------------------------------- 3. the recurrent twins
@pytest.mark.parametrize("net,memory", pc.RECURRENT_ROUNDING)
def test_recurrent_rounding(net, memory):
    cfg, n = dict(pc.NETS[net], memory=memory), pc.ENVS[net]
    est = pc.he_init(perceive.ScanEstimator(cfg), 31)
    ref_net = pc.net_of(est)
    depth, obs = pc.random_inputs(cfg, n, 37)
    m0 = np.random.default_rng(39).normal(size=(n, memory)).astype(np.float32)
    rig = Rig(cfg, est, depth, obs, m0)
    r0 = cfg["scan_row0"]
    for tick, kw, mem in (("random mem", {}, m0), ("clear_all", dict(clear_all=True), np.zeros_like(m0))):
        got = rig.tick(**kw)
        lat, m1, e, _ = mref.step(cfg, ref_net, depth, obs, mem)
        for k, want in (("latent", lat), ("mem", m1), ("est", e)):
            within(f"{net} R = {memory}, {tick}: {k}", got[k], want)
        assert np.array_equal(pc.bits(got["obs"][:, r0:r0 + 117]), pc.bits(got["est"])) and outside_scan_rows_is_obs(cfg, got["obs"], obs)
    rig.close()


@pytest.mark.parametrize("net,memory", pc.RECURRENT_EXACT)
def test_recurrent_exact_case(net, memory):
    c = pc.recurrent_exact_case(net, memory)
    got = run(c["cfg"], c["est"], c["depth"], c["obs"], c["mem0"], clear_mask=torch.from_numpy(c["clear"]))
    for k, want in (("mem", c["want_mem"]), ("est", c["want_est"]), ("obs", c["want_obs"])):
        bad = np.argwhere(pc.bits(got[k]) != pc.bits(want))
        assert not len(bad), f"{net} R = {memory} {k}: {len(bad)} wrong, first (env, element) {bad[0].tolist()}: got {got[k][tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"
    cleared = c["clear"] != 0
    assert (pc.bits(got["mem"][cleared]) == 0).all()                  # +0, not -0
    assert np.isfinite(got["latent"]).all()


@pytest.mark.parametrize("memory", [0, 256], ids=["plain", "recurrent"])
def test_batch_independence_at_33(memory):
    """one env of deep5 at positions 0, 16 and 32 of a batch of 33: the bits it has alone"""
    cfg = dict(pc.NETS["deep5"], memory=memory) if memory else pc.NETS["deep5"]
    est = pc.he_init(perceive.ScanEstimator(cfg), 53)
    depth, obs = pc.random_inputs(cfg, 33, 59)
    d1, o1 = pc.random_inputs(cfg, 1, 61)
    mem = np.random.default_rng(67).normal(size=(33, max(memory, 1))).astype(np.float32)
    m1 = np.random.default_rng(71).normal(size=(1, max(memory, 1))).astype(np.float32)
    for pos in (0, 16, 32):
        depth[pos], obs[pos], mem[pos] = d1[0], o1[0], m1[0]
    alone, batch = run(cfg, est, d1, o1, m1), run(cfg, est, depth, obs, mem)
    for k in alone:
        for pos in (0, 16, 32):
            assert np.array_equal(pc.bits(batch[k][pos]), pc.bits(alone[k][0])), (k, pos)
    assert not np.array_equal(pc.bits(batch["est"][1]), pc.bits(alone["est"][0]))


# ---------------------------------------------------------------- 4. the host checks agree (host code only: nothing is launched)
def test_the_host_checks_agree():
    L = perceive.lib()
    meta = lambda *s: torch.empty(*s, device="meta")
    yes = 0
    for cfg, ok in pc.sweep():
        cs = perceive.config_struct(cfg)
        rc = L.pgtt_perceive_check(C.byref(cs))
        assert rc in (0, -1) and (rc == 0) == ok, (cfg, rc, L.pgtt_perceive_last_error())
        if not ok:
            assert L.pgtt_perceive_latent_dim(C.byref(cs)) == -1 and L.pgtt_perceive_packed_floats(C.byref(cs), 3) == -1, cfg
            continue
        yes += 1
        shapes = perceive.conv_shapes(cfg)
        F = shapes[-1][0] * shapes[-1][1] * shapes[-1][2]
        assert L.pgtt_perceive_latent_dim(C.byref(cs)) == F, cfg
        # the sizes of what pack() produces, from the packers themselves on tensors without storage
        want = [perceive.pack_conv(meta(co, shapes[l][0], k, k)).numel() for l, (co, k, _) in enumerate(cfg["conv"])]
        want += [0] * (perceive.MAX_CONV - len(want))
        want.append(acting.pack_linear(meta(cfg["hidden"], F + len(cfg["prop_rows"])), meta(cfg["hidden"]))[0].numel())
        want.append(acting.pack_linear(meta(117, cfg["hidden"]), meta(117))[0].numel())
        assert [L.pgtt_perceive_packed_floats(C.byref(cs), l) for l in range(perceive.NLAYER)] == want, cfg
    print(f"{len(pc.sweep())} configs, {yes} accepted by both checks")
    assert yes >= 200
    # pack() itself on one accepted config of the sweep: the sizes above are its sizes
    cfg = next(c for c, ok in pc.sweep() if ok and len(c["conv"]) == 3)
    ws, _ = perceive.ScanEstimator(cfg).pack()
    cs = perceive.config_struct(cfg)
    assert [w.numel() for w in ws] == [L.pgtt_perceive_packed_floats(C.byref(cs), l) for l in (0, 1, 2, 3, 4)]
