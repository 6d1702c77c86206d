"""libpgtt_perceive.so on the GPU: the forward pass against the fp64 restatement of tests/perceive_reference.py at every remainder path, input
edges, the obs_out assembly and guard bands, batch independence, the refusals of the C ABI, agreement with the torch module that is trained, the
env left untouched, graph capture of a student env under FusedActor, FusedActor(obs=...), scan_target against the observation, and a
distillation smoke run.

The bar of a forward pass is the project's own (check_mlp in tests/test_gpu_acting_edges.py): 2e-5 * (1 + max|want|) per element, for `est` and
for the latent.  That the bar is reachable in fp32 was checked on the CPU before the kernel met it: torch's fp32 forward of the same nets, weights
and inputs against the fp64 reference gives a worst error / bar (latent, est) of 0.0088, 0.0055 (default net, N = 3), 0.0034, 0.0032 (9 x 11, one conv,
N = 1), 0.0087, 0.0078 (20 x 28, three convs, N = 17) and 0.0133, 0.0114 (the same, N = 65)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perceive_reference as ref  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, configs, perceive  # noqa: E402
from phase_guided_terrain_traversal_amd.acting import FusedActor  # noqa: E402
from phase_guided_terrain_traversal_amd.env import Joystick  # noqa: E402
from phase_guided_terrain_traversal_amd.policy import load_policy  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL4 = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy")
DEFAULT = perceive.DEFAULTS
SMALL = dict(height=9, width=11, near=0.1, far=3.0, conv=[(16, 5, 2)], prop_rows=[], hidden=16, obs_dim=171, scan_row0=38)   # 3 x 4 = 12 pixels < a tile
MIXED = dict(height=20, width=28, near=0.1, far=3.0, conv=[(16, 5, 2), (32, 3, 1), (48, 3, 2)], prop_rows=list(range(38)) + [155, 170], hidden=48,
             obs_dim=171, scan_row0=38)
GUARD = 12345.0


def he_init(est, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in est.layers():
            fan_in = m.weight[0].numel()
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return est


def net_of(est):
    f64 = lambda t: t.detach().double().cpu().numpy()
    return {"conv": [(f64(c.weight), f64(c.bias)) for c in est.convs], "fc1": (f64(est.fc1.weight), f64(est.fc1.bias)),
            "fc2": (f64(est.fc2.weight), f64(est.fc2.bias))}


def inputs(cfg, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 3.5, (n, cfg["height"], cfg["width"])).astype(np.float32), rng.normal(size=(n, cfg["obs_dim"])).astype(np.float32))


def fake_env(cfg, depth, obs):
    """what StudentPerception reads of an env: the image, the observation, the device"""
    d, o = torch.from_numpy(depth).cuda(), torch.from_numpy(obs).cuda()
    return types.SimpleNamespace(depth=d, depth_camera=types.SimpleNamespace(height=cfg["height"], width=cfg["width"]), buffers={"obs_state": o},
                                 device=d.device, num_envs=d.shape[0], observation_size={"state": cfg["obs_dim"]})


def run(cfg, est, depth, obs):
    """one call -> (latent, est, obs_out) as numpy"""
    sp = perceive.StudentPerception(fake_env(cfg, depth, obs), est)
    sp.tick()
    torch.cuda.synchronize()
    out = sp.latent.cpu().numpy(), sp.est.cpu().numpy(), sp.obs.cpu().numpy()
    sp.close()
    return out


def check_forward(cfg, est, depth, obs):
    """latent and est inside the bar -> the worst error / bar"""
    lat, got, out = run(cfg, est, depth, obs)
    wl, we, _ = ref.forward(cfg, net_of(est), depth, obs)
    assert np.isfinite(lat).all() and np.isfinite(got).all() and np.isfinite(out).all()
    worst = 0.0
    for name, g, w in (("latent", lat, wl), ("est", got, we)):
        err, bar = np.abs(g - w).max(), 2e-5 * (1 + np.abs(w).max())
        print(f"{name}: max error {err:.3e}, bar {bar:.3e}, ratio {err / bar:.3f}")
        assert err < bar, (name, err, bar)
        worst = max(worst, err / bar)
    return worst


# ---------------------------------------------------------------- 1. forward against fp64
@pytest.mark.parametrize("name,cfg,n", [("default", DEFAULT, 3), ("small", SMALL, 1), ("mixed17", MIXED, 17), ("mixed65", MIXED, 65)])
def test_forward_against_fp64(name, cfg, n):
    est = he_init(perceive.ScanEstimator(cfg), 7)
    check_forward(cfg, est, *inputs(cfg, n, 11))


# ---------------------------------------------------------------- 2. input edges
def test_input_edges():
    cfg = DEFAULT
    est = he_init(perceive.ScanEstimator(cfg), 8)
    h, w = cfg["height"], cfg["width"]
    rng = np.random.default_rng(3)
    depth = np.empty((4, h, w), np.float32)
    depth[0] = cfg["far"]
    depth[1] = 0.01                                                   # below near
    depth[2] = rng.uniform(0.0, 3.5, (h, w))
    depth[2].reshape(-1)[::5] = np.nan
    depth[2].reshape(-1)[1::7] = np.inf
    depth[3] = cfg["far"]
    depth[3].reshape(-1)[::16] = cfg["near"]                          # one near pixel per 16-pixel run
    _, obs = inputs(cfg, 4, 5)
    check_forward(cfg, est, depth, obs)


# ---------------------------------------------------------------- 3. obs_out and guard bands
@pytest.mark.parametrize("method", ["pgtt", "baseline"])
def test_obs_out_and_guards(method):
    cfg = perceive.config(method)
    assert (cfg["obs_dim"], cfg["scan_row0"]) == ((171, 38) if method == "pgtt" else (162, 30))
    est = he_init(perceive.ScanEstimator(cfg), 9)
    depth, obs = inputs(cfg, 3, 13)
    sp = perceive.StudentPerception(fake_env(cfg, depth, obs), est)
    n, od, F, pad = 3, cfg["obs_dim"], est.latent_dim, 64
    bufs = {k: torch.full((pad + n * w + pad,), GUARD, device="cuda") for k, w in (("latent", F), ("est", 117), ("obs", od))}
    sp.latent, sp.est, sp.obs = (bufs[k][pad:-pad].view(n, w) for k, w in (("latent", F), ("est", 117), ("obs", od)))
    sp.bind()
    sp.tick()
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert (t[:pad] == GUARD).all() and (t[-pad:] == GUARD).all(), k
        assert (t[pad:-pad] != GUARD).all(), k
    out, e = sp.obs.cpu().numpy().view(np.int32), sp.est.cpu().numpy().view(np.int32)
    r0 = cfg["scan_row0"]
    assert np.array_equal(out[:, r0:r0 + 117], e)
    assert np.array_equal(out[:, :r0], obs.view(np.int32)[:, :r0]) and np.array_equal(out[:, r0 + 117:], obs.view(np.int32)[:, r0 + 117:])
    sp.close()


# ---------------------------------------------------------------- 4. batch independence
def test_batch_independence():
    cfg = MIXED
    est = he_init(perceive.ScanEstimator(cfg), 10)
    depth, obs = inputs(cfg, 65, 17)
    d1, o1 = inputs(cfg, 1, 19)
    alone_lat, alone, alone_out = run(cfg, est, d1, o1)
    for pos in (0, 16, 64):
        depth[pos], obs[pos] = d1[0], o1[0]
    lat, got, out = run(cfg, est, depth, obs)
    for pos in (0, 16, 64):
        assert np.array_equal(got[pos].view(np.int32), alone[0].view(np.int32)), pos
        assert np.array_equal(lat[pos].view(np.int32), alone_lat[0].view(np.int32)), pos
        assert np.array_equal(out[pos].view(np.int32), alone_out[0].view(np.int32)), pos


# ---------------------------------------------------------------- 5. refusals (host-side validation only: nothing is launched)
def test_refusals():
    L = perceive.lib()
    d = DEFAULT
    bad = {
        "channels_not_16": dict(d, conv=[(16, 5, 2), (24, 3, 2), (32, 3, 2)]),
        "hidden_not_16": dict(d, hidden=500),
        "empty_layer": dict(d, height=9, width=11, conv=[(16, 5, 2), (16, 5, 1)]),
        "prop_row_outside": dict(d, prop_rows=[0, 171]),
        "scan_rows_past_obs": dict(d, scan_row0=55),
        "lds_budget": dict(d, conv=[(32, 3, 1), (16, 3, 2)]),
    }
    for name, cfg in bad.items():
        cs = perceive.config_struct(cfg)
        h = C.c_void_p()
        assert L.pgtt_perceive_check(C.byref(cs)) == -1, name
        assert L.pgtt_perceive_create(C.byref(cs), 0, 3, C.byref(h)) == -1 and not h.value, name
        assert L.pgtt_perceive_last_error(), name
        with pytest.raises(ValueError):
            perceive.check_config(cfg)
    assert L.pgtt_perceive_check(None) == -1
    assert L.pgtt_perceive_check(C.byref(perceive.config_struct(d))) == 0
    # a NULL required pointer: bind refuses and the handle keeps what it had; guard-filled outputs stay as they are
    est = he_init(perceive.ScanEstimator(d), 2)
    depth, obs = inputs(d, 3, 1)
    sp = perceive.StudentPerception(fake_env(d, depth, obs), est)
    for t in (sp.latent, sp.est, sp.obs):
        t.fill_(GUARD)
    good = perceive.PgttPerceiveBuffers()
    good.depth, good.obs = sp.env.depth.data_ptr(), sp.env.buffers["obs_state"].data_ptr()
    for l, w, b in zip(sp._layers, sp._w, sp._b):
        good.w[l], good.b[l] = w.data_ptr(), b.data_ptr()
    good.latent, good.est, good.obs_out = sp.latent.data_ptr(), sp.est.data_ptr(), sp.obs.data_ptr()
    for field in ("depth", "obs", "latent", "est"):
        b = perceive.PgttPerceiveBuffers.from_buffer_copy(good)
        setattr(b, field, None)
        assert L.pgtt_perceive_bind(sp._h, C.byref(b)) == -1, field
    for arr, idx in (("w", 0), ("b", 2), ("w", 3), ("b", 4)):
        b = perceive.PgttPerceiveBuffers.from_buffer_copy(good)
        getattr(b, arr)[idx] = None
        assert L.pgtt_perceive_bind(sp._h, C.byref(b)) == -1, (arr, idx)
    assert L.pgtt_perceive_bind(sp._h, None) == -1 and L.pgtt_perceive(None, None) == -1
    torch.cuda.synchronize()
    for t in (sp.latent, sp.est, sp.obs):
        assert (t == GUARD).all()
    good.obs_out = None                                              # obs_out is optional
    assert L.pgtt_perceive_bind(sp._h, C.byref(good)) == 0
    sp.tick()
    torch.cuda.synchronize()
    assert (sp.obs == GUARD).all() and (sp.est != GUARD).all()
    sp.close()


# ---------------------------------------------------------------- 6. the thing trained is the thing run
@pytest.mark.parametrize("cfg,n", [(DEFAULT, 3), (MIXED, 17)], ids=["default", "mixed"])
def test_torch_module_agrees_with_the_kernel(cfg, n):
    est = he_init(perceive.ScanEstimator(cfg), 12)
    depth, obs = inputs(cfg, n, 23)
    lat, got, out = run(cfg, est, depth, obs)
    g = est.cuda()
    with torch.no_grad():
        d, o = torch.from_numpy(depth).cuda(), torch.from_numpy(obs).cuda()
        tl, te = g.latent(d).cpu().numpy(), g(d, o).cpu().numpy()
        tout = g.assemble(o, g(d, o)).cpu().numpy()
    _, we, _ = ref.forward(cfg, net_of(est), depth, obs)
    assert np.abs(got - te).max() < 2e-5 * (1 + np.abs(we).max())
    assert np.abs(lat - tl).max() < 2e-5 * (1 + np.abs(tl).max())
    assert np.abs(out - tout).max() < 2e-5 * (1 + np.abs(we).max())


# ---------------------------------------------------------------- envs
def make_env(n, seed, student=None, depth=None, cfg=None, **kw):
    terrain = np.load(LEVEL4)
    variant = torch.from_numpy(np.random.default_rng(0).integers(0, terrain.shape[0], n).astype(np.int32))
    env = Joystick("stairs", configs.training_config() if cfg is None else cfg, num_envs=n, terrain=terrain, device="cuda:0", variant=variant,
                   depth=depth, student=student, **kw)
    env.reset(seed)
    return env


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def test_student_needs_depth():
    with pytest.raises(ValueError):
        Joystick("stairs", configs.training_config(), num_envs=4, terrain=np.load(LEVEL4), device="cuda:0", student=perceive.ScanEstimator())


# ---------------------------------------------------------------- 7. the env is untouched
def test_env_is_untouched():
    est = he_init(perceive.ScanEstimator(), 14)
    a, b = make_env(64, 5, student=est, depth={}), make_env(64, 5)
    assert b.student is None and b.student_obs is None and a.student_obs.shape == (64, 171)
    rng = np.random.default_rng(6)
    for t in range(5):
        act = torch.from_numpy(np.tanh(rng.normal(size=(64, 12)) * 0.6).astype(np.float32)).cuda()
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        torch.cuda.synchronize()
        for x, y in ((oa["state"], ob["state"]), (oa["privileged_state"], ob["privileged_state"]), (ra, rb), (da, db), (a.buffers["state"], b.buffers["state"])):
            assert np.array_equal(_bits(x), _bits(y)), t
        # student_obs is the observation with the scan rows replaced by the estimate from the image of this step
        so = _bits(a.student_obs)
        assert np.array_equal(so[:, :38], _bits(oa["state"])[:, :38]) and np.array_equal(so[:, 155:], _bits(oa["state"])[:, 155:])
        assert np.array_equal(so[:, 38:155], _bits(a.student.est)) and np.isfinite(a.student.est.cpu().numpy()).all()
    with torch.no_grad():
        want = est.cuda()(a.depth, a.buffers["obs_state"]).cpu().numpy()
    assert np.abs(a.student.est.cpu().numpy() - want).max() < 2e-5 * (1 + np.abs(want).max())
    a.close(); b.close()


# ---------------------------------------------------------------- 8. graph capture
def _student_actor(seed):
    est = he_init(perceive.ScanEstimator(), 15)
    env = make_env(64, seed, student=est, depth={}, autoreset=True)
    actor = FusedActor(env, T=8, seed=3, obs=env.student_obs)
    pi = load_policy("policy177", "cuda:0")
    actor.load([(m.weight, m.bias) for m in pi.layers], pi.mean, pi.std)
    return env, actor


def test_student_env_under_the_actor_in_a_graph():
    (ea, a), (eb, b) = _student_actor(2), _student_actor(2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.step()
    torch.cuda.current_stream().wait_stream(s)
    b.step()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.step()
    for t in range(3):
        g.replay(); b.step()
        torch.cuda.synchronize()
        for x, y in ((ea.student_obs, eb.student_obs), (ea.buffers["state"], eb.buffers["state"]), (a.action, b.action), (ea.depth, eb.depth),
                     (a.storage["obs"], b.storage["obs"]), (a.storage["logp"], b.storage["logp"])):
            assert np.array_equal(_bits(x), _bits(y)), t
    assert int(a.counters[0]) == int(b.counters[0]) == 4
    # the storage records what the policy saw: the student's rows
    assert not np.array_equal(_bits(a.storage["obs"][3]), _bits(ea.buffers["obs_state"]))
    ea.close(); eb.close()


# ---------------------------------------------------------------- 9. FusedActor(obs=t)
def test_actor_reads_the_given_tensor():
    env = make_env(64, 4, autoreset=True)
    t = torch.from_numpy(np.random.default_rng(8).normal(size=(64, 171)).astype(np.float32)).cuda()
    pi = load_policy("policy177", "cuda:0")
    a, b = FusedActor(env, T=2, seed=1, obs=t), FusedActor(env, T=2, seed=1)
    for actor in (a, b):
        actor.load([(m.weight, m.bias) for m in pi.layers], pi.mean, pi.std)
    before = env.buffers["obs_state"].clone()
    act_a = a.act().clone()
    assert torch.equal(env.buffers["obs_state"], before)
    env.buffers["obs_state"].copy_(t)
    act_b = b.act().clone()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(act_a), _bits(act_b)) and np.array_equal(_bits(a.storage["obs"][0]), _bits(t))
    assert np.array_equal(_bits(a.storage["logp"][0]), _bits(b.storage["logp"][0]))
    with pytest.raises(ValueError):
        FusedActor(env, T=2, obs=t[:, :170])
    env.close()


# ---------------------------------------------------------------- scan_target is the noise-free value of the observation's scan rows
def test_scan_target_against_the_observation():
    cfg = configs.training_config()
    cfg["noise_config"] = dict(cfg["noise_config"], level=0.0)
    env = make_env(64, 9, cfg=cfg)
    rng = np.random.default_rng(2)
    for t in range(3):
        obs, _, _, _ = env.step(torch.from_numpy(np.tanh(rng.normal(size=(64, 12)) * 0.6).astype(np.float32)).cuda())
    got, want = obs["state"][:, 38:155].cpu().numpy(), perceive.scan_target(env).cpu().numpy()
    assert want.min() == 0.0 and want.max() > 0.0
    assert np.abs(got - want).max() <= 2 ** -22 * (1 + np.abs(env.buffers["scan_z"].cpu().numpy()).max())      # one fp32 subtraction each way
    env.close()


# ---------------------------------------------------------------- 10. distillation smoke
def test_distillation_reduces_the_loss_on_unseen_steps():
    import train_student
    torch.manual_seed(0)
    est = perceive.ScanEstimator().cuda()
    env = make_env(64, 3, student=est, depth={}, autoreset=True)
    col = train_student.Collector(env, load_policy("policy177", "cuda:0"), 8, seed=0)
    train = col.collect(1.0)
    held = col.collect(1.0)
    assert train[0].shape == (512, 48, 64) and train[1].shape == (512, 171) and train[2].shape == (512, 117)
    before = train_student.huber(est, held)
    opt = torch.optim.Adam(est.parameters(), lr=1e-3)
    train_student.fit(est, opt, train, 30, 128, torch.Generator(device="cuda").manual_seed(0))
    after = train_student.huber(est, held)
    print(f"huber on 8 unseen steps: {before:.5f} -> {after:.5f}; band rmse {train_student.band_rmse(est, held)}")
    assert after < before
    env.student.load(est)                                            # the kernel now runs the trained weights
    env.student.tick()
    with torch.no_grad():
        want = est(env.depth, env.buffers["obs_state"]).cpu().numpy()
    assert np.abs(env.student.est.cpu().numpy() - want).max() < 2e-5 * (1 + np.abs(want).max())
    env.close()
