"""In-run terrain curriculum (pgtt_curriculum) on the GPU: the decision rule against curriculum.replay on hand-written buffers, the restart is a
plain masked Joystick.reset, thresholds that never move an env leave the step as it is, the labels stay legal under a policy, the ladder does
what it is for, shards / captured graphs / the fused actor reproduce the eager bits, refusals launch nothing, and a short training run."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle
from phase_guided_terrain_traversal_amd import abi, configs, curriculum, mjcf, native, policy
from phase_guided_terrain_traversal_amd.acting import FusedActor
from phase_guided_terrain_traversal_amd.env import Joystick
from phase_guided_terrain_traversal_amd.randomize import domain_randomize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERRAINS = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains")
PUSH = dict(wait=(0.05, 0.3), duration=(0.04, 0.3), velocity=(0.0, 1.5))
I_TRK = abi.REWARD_KEYS.index("tracking_lin_vel")


def _level(name):
    return np.load(os.path.join(TERRAINS, name + ".npy"))


LADDER = [_level("level1"), _level("level2"), _level("level4")]          # 100 + 50 + 100 variants
TABLE, START = curriculum.stack_levels(LADDER)


def _cfg(L=None):
    return configs.training_config() if L is None else configs.with_overrides(configs.training_config(), episode_length=L)


def _dr(n, seed=3, offset=0, total=None, table=TABLE):
    dr = domain_randomize(mjcf.load_model("stairs"), n, seed=seed, terrain=table, env_id_offset=offset, total_envs=total)
    return {"params": torch.from_numpy(dr["params"]), "box_friction": torch.from_numpy(dr["box_friction"])}


def _env(n, cur, cfg=None, ladder=LADDER, dr=True, **kw):
    kw = dict(_dr(n) if dr else {}, **kw)
    return Joystick("stairs", cfg or _cfg(), num_envs=n, terrain=ladder, device="cuda:0", autoreset=True, curriculum=cur, **kw)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _wild(n, gen, scale=3.0):
    """the input tests/test_gpu_acting.py uses to make robots fall: actions far outside [-1, 1]"""
    return torch.tanh(torch.randn(n, 12, device="cuda:0", generator=gen)) * scale


def _legal(env):
    ls = torch.from_numpy(np.asarray(env.level_start)).to(env.device)
    lv, va = env.level.long(), env.buffers["variant"].long()
    L = len(env.level_start) - 1
    ok = (lv >= 0) & (lv < L)
    lc = lv.clamp(0, L - 1)
    return ok & (va >= ls[lc]) & (va < ls[lc + 1])


ALL_KEYS = ("state", "istate", "frame", "scan_z", "obs_state", "obs_priv", "reward", "done", "metrics", "first_state", "first_obs", "ep_metrics",
            "level", "variant")


def test_decision_rule_against_the_host_replay():
    """every branch on every level of a 3-level table, buffers written by hand after a reset: level, variant, curriculum_stats equal
    curriculum.replay fed by oracle.uniform exactly; envs with done == 0 keep every buffer bit"""
    L_EP, seed, off = 100, 11, 640
    cfg = _cfg(L_EP)
    sc = np.float32(cfg["reward_config"]["scales"]["tracking_lin_vel"])
    thr = np.float32(0.65)
    at_thr = np.float32(np.float32(99) * sc) * thr
    cases = [(1, 100, 0.9 * 99 * float(sc), 99), (1, 100, 0.3 * 99 * float(sc), 99), (1, 100, float(at_thr), 99), (1, 100, float(np.nextafter(at_thr, np.float32(0))), 99),
             (1, 99, 0.9 * 98 * float(sc), 98), (1, 20, 5.0, 19), (1, 49, 5.0, 48), (1, 50, 5.0, 49), (1, 100, 0.0, 0), (1, 1, 0.0, 0), (1, 150, 140 * float(sc), 149),
             (0, 100, 0.9 * 99 * float(sc), 99), (0, 3, 0.0, 2), (0, 20, 5.0, 19)]
    reps = 5                                                        # several draws of u per (case, level)
    n = len(cases) * 3 * reps
    env = _env(n, dict(promote_tracking=0.65, demote_length=0.5, init_level=(0, 2)), cfg=cfg, env_id_offset=off, push=PUSH)
    env.reset(seed)
    rows = [(c, l) for c in cases for l in range(3) for _ in range(reps)]
    rng = np.random.default_rng(0)
    level = np.array([l for _, l in rows], np.int32)
    variant = (START[level] + rng.integers(0, START[level + 1] - START[level])).astype(np.int32)
    done = np.array([c[0] for c, _ in rows], np.float32)
    steps = np.array([c[1] for c, _ in rows], np.int32)
    epm = rng.uniform(0, 3, size=(abi.NMETRIC + 2, n)).astype(np.float32)
    epm[I_TRK] = [c[2] for c, _ in rows]; epm[abi.NMETRIC + 1] = [c[3] for c, _ in rows]
    B = env.buffers
    B["done"].copy_(torch.from_numpy(done)); B["ep_metrics"].copy_(torch.from_numpy(epm))
    B["level"].copy_(torch.from_numpy(level)); B["variant"].copy_(torch.from_numpy(variant))
    B["istate"][abi.I_EP_STEPS].copy_(torch.from_numpy(steps))
    B["reward"].copy_(torch.from_numpy(rng.normal(size=n).astype(np.float32))); B["metrics"].copy_(torch.from_numpy(rng.normal(size=(abi.NMETRIC, n)).astype(np.float32)))
    torch.cuda.synchronize()
    before = {k: B[k].clone() for k in ALL_KEYS + ("push_state", "xfrc")}
    epoch = B["istate"][abi.I_RNG_CTR].cpu().numpy()
    u = np.array([oracle.uniform(seed, off + e, int(epoch[e]), abi.RS_CURRICULUM, 0) for e in range(n)], np.float32)
    want = curriculum.replay(done, steps, epm, level, variant, u, START, L_EP, sc, 0.65, 0.5)
    assert want["stats"][abi.CS_PROMOTED] > 0 and want["stats"][abi.CS_DEMOTED] > 0
    env.curriculum_step()
    torch.cuda.synchronize()
    assert np.array_equal(B["level"].cpu().numpy(), want["level"])
    assert np.array_equal(B["variant"].cpu().numpy(), want["variant"])
    assert np.array_equal(B["curriculum_stats"].cpu().numpy(), want["stats"])
    keep = torch.from_numpy(done == 0).cuda()
    for k, old in before.items():
        new = B[k]
        if new.shape[0] == n and new.ndim >= 1 and (new.ndim == 1 or k in ("scan_z", "obs_state", "obs_priv", "first_obs")):
            assert _same(new[keep], old[keep]), k
        else:
            assert _same(new[..., keep], old[..., keep]), k
    fin = ~keep
    # the step's own outputs of a finished env stay as the step wrote them; its sums and counters are the fresh reset's
    for k in ("reward", "done"):
        assert _same(B[k][fin], before[k][fin]), k
    assert _same(B["metrics"][:, fin], before["metrics"][:, fin])
    assert float(B["ep_metrics"][:, fin].abs().sum()) == 0.0 and int(B["istate"][abi.I_EP_STEPS][fin].abs().sum()) == 0
    assert bool((B["istate"][abi.I_RNG_CTR][fin] == before["istate"][abi.I_RNG_CTR][fin] + 1).all())
    st = env.curriculum_stats()
    assert st["finished"] == int((done != 0).sum()) and st["promoted"] == want["stats"][abi.CS_PROMOTED] and int(B["curriculum_stats"].abs().sum()) == 0
    env.close()


@pytest.mark.parametrize("layout", ["quad", "oct", "hex"])
def test_the_restart_is_joystick_reset(layout):
    """a twin without curriculum, given the labels the curriculum chose and a plain masked reset at the same epoch, holds the same bits in the
    reset envs, and over the next 20 steps under the same actions.  (The twin's reset clears done / reward / metrics of the reset envs, which the
    curriculum leaves as the step wrote them: they are copied over, being the step's outputs, not the restart's.)"""
    n, seed = 256, 9
    cfg = _cfg(25)
    lv, va = curriculum.initial_labels(1, 0, n, START, (0, 2))
    kw = dict(layout=layout, push=PUSH, variant=torch.from_numpy(va))
    a = _env(n, dict(promote_tracking=0.2, demote_length=0.9), cfg=cfg, level=torch.from_numpy(lv), **kw)
    b = _env(n, None, cfg=cfg, **kw)
    a.reset(seed); b.reset(seed)
    gen = torch.Generator("cuda:0").manual_seed(2)
    restarts = 0
    for t in range(40):
        act = _wild(n, gen, 1.5)
        a.step(act, curriculum=False); b.step(act)
        for k in ("state", "istate", "obs_state", "obs_priv", "reward", "done", "metrics", "ep_metrics", "push_state", "xfrc"):
            assert _same(a.buffers[k], b.buffers[k]), (t, k)
        done = a.buffers["done"] > 0
        if not bool(done.any()):
            continue
        restarts += int(done.sum())
        out = {k: a.buffers[k].clone() for k in ("reward", "done", "metrics")}
        a.curriculum_step()
        assert bool(_legal(a).all())
        for k in out:
            assert _same(a.buffers[k], out[k]), (t, k)                   # left as the step wrote them
        b.buffers["variant"].copy_(a.buffers["variant"])
        b.reset(seed, mask=done)
        for k in ("state", "istate", "first_state", "ep_metrics", "push_state", "xfrc"):
            assert _same(a.buffers[k][..., done], b.buffers[k][..., done]), (t, k)
            assert _same(a.buffers[k], b.buffers[k]), (t, k)
        for k in ("first_obs", "obs_state", "obs_priv"):
            assert _same(a.buffers[k], b.buffers[k]), (t, k)
        for k in out:
            b.buffers[k].copy_(out[k])
    assert restarts > n // 4, restarts
    st = a.curriculum_stats()
    assert st["finished"] == restarts and st["promoted"] + st["demoted"] > 0
    a.close(); b.close()


def test_thresholds_that_never_move_an_env_leave_the_step_alone():
    """a ladder of one-variant levels, promote_tracking = 1 (the tracking mean is below 1), demote_length = 0: every decision is "stay", and env by
    env the reward / done rows equal a plain autoreset twin's up to and including that env's first done"""
    n, seed, T = 512, 4, 60            # quad layout: there an env's roundings do not depend on its neighbours in the wave, which part ways after their first done
    l4 = _level("level4")
    ladder = [l4[0:1], l4[1:2], l4[2:3]]
    cfg = _cfg(30)
    dr = _dr(n, table=l4[0:3])
    a = Joystick("stairs", cfg, num_envs=n, terrain=ladder, device="cuda:0", autoreset=True, layout="quad",
                 curriculum=dict(promote_tracking=1.0, demote_length=0.0, init_level=1), **dr)
    b = Joystick("stairs", cfg, num_envs=n, terrain=ladder, device="cuda:0", autoreset=True, layout="quad", variant=torch.ones(n, dtype=torch.int32), **dr)
    assert bool((a.buffers["variant"] == 1).all())
    a.reset(seed); b.reset(seed)
    gen = torch.Generator("cuda:0").manual_seed(5)
    live = torch.ones(n, dtype=torch.bool, device="cuda:0")
    ndone = 0
    for t in range(T):
        act = _wild(n, gen, 1.5)
        a.step(act); b.step(act)
        for k in ("reward", "done"):
            assert _same(a.buffers[k][live], b.buffers[k][live]), (t, k)
        d = a.buffers["done"] > 0
        ndone += int((d & live).sum())
        live &= ~d
    assert ndone == n and not bool(live.any())                       # episode_length 30 < 60 steps: every env finished once
    st = a.curriculum_stats()
    assert st["promoted"] == 0 and st["demoted"] == 0 and st["finished"] >= n and bool((a.level == 1).all()) and bool((a.buffers["variant"] == 1).all())
    a.close(); b.close()


def test_labels_stay_legal_under_a_policy():
    """300 steps of policy177, episode_length 100, [level01, level4, level13], full DR, 4096 envs: after every step each env's variant lies in its
    level's range and the counters' totals equal the host's count of done flags"""
    n = 4096
    ladder = [_level("level01"), _level("level4"), _level("level13")]
    table, start = curriculum.stack_levels(ladder)
    net = policy.load_policy("policy177", device="cuda:0")
    env = _env(n, dict(promote_tracking=0.65, demote_length=0.5, init_level=(0, 2)), cfg=_cfg(100), ladder=ladder, dr=False, **_dr(n, table=table))
    env.reset(1)
    ok = torch.ones((), dtype=torch.bool, device="cuda:0")
    ndone = torch.zeros((), dtype=torch.int64, device="cuda:0")
    with torch.no_grad():
        for t in range(300):
            _, _, done, _ = env.step(net(env.buffers["obs_state"]))
            ok &= _legal(env).all()
            ndone += (done > 0).sum()
    assert bool(ok)
    st = env.curriculum_stats()
    print("labels: finished", st["finished"], "promoted", st["promoted"], "demoted", st["demoted"], "per level", st["finished_per_level"], "mean level", st["mean_level"])
    assert st["finished"] == int(ndone) == sum(st["finished_per_level"]) and st["finished"] >= 2 * n
    env.close()


def _run_ladder(cur, actions, n=2048, steps=300):
    """all envs start on level 1 of [level1, level4, level13], episode_length 100 -> the env and its stats"""
    ladder = [_level("level1"), _level("level4"), _level("level13")]
    table, _ = curriculum.stack_levels(ladder)
    env = _env(n, dict(cur, init_level=1), cfg=_cfg(100), ladder=ladder, dr=False, **_dr(n, table=table))
    env.reset(2)
    net = policy.load_policy("policy177", device="cuda:0")
    gen = torch.Generator("cuda:0").manual_seed(3)
    zero = torch.zeros(n, 12, device="cuda:0")
    with torch.no_grad():
        for t in range(steps):
            act = net(env.buffers["obs_state"]) if actions == "policy" else (zero if actions == "zero" else _wild(n, gen))
            env.step(act)
    st = env.curriculum_stats()
    st["above"] = float((env.level > 1).float().mean())
    env.close()
    return st


def test_the_ladder_does_what_it_is_for():
    """three monotone statements.  Falling early is provoked by the wild actions of tests/test_gpu_acting.py (3 x tanh of normal draws)."""
    s0 = _run_ladder(dict(promote_tracking=0.0, demote_length=0.5), "policy")
    print("promote_tracking 0, policy177: share of envs above level 1 after 300 steps", s0["above"], s0)
    assert s0["above"] >= 0.5
    sp = _run_ladder(dict(promote_tracking=0.65, demote_length=0.5), "policy")
    sz = _run_ladder(dict(promote_tracking=0.65, demote_length=0.5), "zero")
    print("promote_tracking 0.65: promoted under policy177", sp["promoted"], "under zero actions", sz["promoted"])
    assert sz["promoted"] < sp["promoted"]
    sw = _run_ladder(dict(promote_tracking=0.65, demote_length=1.0), "wild")
    print("wild actions, demote_length 1: demoted", sw["demoted"], "mean level", sw["mean_level"], "finished", sw["finished"])
    assert sw["demoted"] > 0 and sw["mean_level"] <= 1.0


@pytest.mark.parametrize("layout", ["quad", "oct", "hex"])
def test_shards_reproduce_the_single_handle(layout):
    """two handles of 2048 envs at env_id_offset 0 / 2048 hold the 4096-env handle's level, variant and state bits over 150 steps"""
    n, h, seed = 4096, 2048, 6
    cfg = _cfg(40)
    cur = dict(promote_tracking=0.3, demote_length=0.6, init_level=(0, 2), seed=8)
    full = _env(n, cur, cfg=cfg, layout=layout)
    parts = []
    for lo in (0, h):
        kw = {k: v[..., lo:lo + h].contiguous() for k, v in _dr(n).items()}
        parts.append(_env(h, cur, cfg=cfg, layout=layout, dr=False, env_id_offset=lo, **kw))
    assert torch.equal(full.level, torch.cat([p.level for p in parts]))
    full.reset(seed); [p.reset(seed) for p in parts]
    gen = torch.Generator("cuda:0").manual_seed(1)
    same = torch.ones((), dtype=torch.bool, device="cuda:0")
    for t in range(150):
        a = _wild(n, gen, 1.2)
        full.step(a); parts[0].step(a[:h].contiguous()); parts[1].step(a[h:].contiguous())
        for k in ("state", "level", "variant", "done"):
            cat = torch.cat([parts[0].buffers[k], parts[1].buffers[k]], dim=-1)
            same &= (_bits(full.buffers[k]) == _bits(cat)).all()
    assert bool(same)
    sf, s0, s1 = full.curriculum_stats(), parts[0].curriculum_stats(), parts[1].curriculum_stats()
    assert sf["finished"] == s0["finished"] + s1["finished"] > n and sf["promoted"] == s0["promoted"] + s1["promoted"] and sf["promoted"] + sf["demoted"] > 0
    full.close(); [p.close() for p in parts]


def test_captured_step_with_curriculum_replays_the_eager_bits():
    n = 256
    cur = dict(promote_tracking=0.3, demote_length=0.6, init_level=(0, 2))
    a, b = (_env(n, cur, cfg=_cfg(15), push=PUSH) for _ in range(2))
    a.reset(4); b.reset(4)
    act = _wild(n, torch.Generator("cuda:0").manual_seed(0), 1.2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.step(act)
    torch.cuda.current_stream().wait_stream(s)
    b.step(act)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.step(act)
    for t in range(60):
        g.replay(); b.step(act)
        for k in ("state", "obs_priv", "level", "variant", "done", "ep_metrics", "curriculum_stats"):
            assert _same(a.buffers[k], b.buffers[k]), (t, k)
    torch.cuda.synchronize()
    assert a.curriculum_stats()["finished"] > n
    a.close(); b.close()


def test_fused_actor_records_before_the_curriculum():
    """FusedActor.step with the curriculum on (step -> record -> curriculum) reports the finished-episode sums that torch ops compute from done /
    ep_metrics read BEFORE the curriculum call on a twin driven by the same actions"""
    from phase_guided_terrain_traversal_amd import ppo
    n, T, L = 1000, 40, 13
    cur = dict(promote_tracking=0.3, demote_length=0.6, init_level=(0, 2))
    a, b = (_env(n, cur, cfg=_cfg(L)) for _ in range(2))
    a.reset(3); b.reset(3)
    torch.manual_seed(1)
    model = ppo.ActorCritic().cuda()
    fa, fb = (FusedActor(e, T=T, seed=2, reward_scaling=0.5) for e in (a, b))
    for f in (fa, fb):
        f.load_sequential(model.policy, torch.zeros(171, device="cuda"), torch.ones(171, device="cuda"))
    sums = torch.zeros(abi.NMETRIC + 3, device="cuda", dtype=torch.float64)
    ref_done = torch.zeros(T, n, device="cuda")
    for t in range(T):
        fa.step()
        fb.act()
        _, reward, done, info = b.step(fb.action, curriculum=False)
        epm = info["episode_metrics"].double()
        sums[:abi.NMETRIC] += (epm[:abi.NMETRIC] * done).sum(1); sums[abi.NMETRIC] += (epm[abi.NMETRIC] * done).sum()
        sums[abi.NMETRIC + 1] += (epm[abi.NMETRIC + 1] * done).sum(); sums[abi.NMETRIC + 2] += done.sum()
        ref_done[t] = done
        fb.record()
        b.curriculum_step()
        assert _same(a.buffers["state"], b.buffers["state"]) and _same(a.level, b.level), t
    torch.cuda.synchronize()
    assert torch.equal(fa.storage["done"], ref_done) and float(ref_done.sum()) > n
    assert float(sums[abi.NMETRIC + 1]) > 0                           # the length sums were read before the restart cleared them
    assert torch.allclose(fa.episode_sums.double(), sums, rtol=2e-5, atol=1e-4), (fa.episode_sums, sums)
    a.close(); b.close()


def test_refusals_launch_nothing():
    L = native.lib()
    n = 64
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    env = _env(n, dict(init_level=(0, 2)))
    cur_ok = abi.curriculum_struct(env.curriculum, env.buffers["level"].data_ptr(), env.buffers["curriculum_stats"].data_ptr())
    # pgtt_bind without variant / ep_metrics while the curriculum is on; pgtt_set_curriculum without a level buffer, with bad settings, on such buffers
    for missing in ("variant", "ep_metrics"):
        b = abi.PgttBuffers()
        for name, _ in abi.PgttBuffers._fields_:
            t = env.buffers.get(name)
            setattr(b, name, None if t is None or name == missing else t.data_ptr())
        assert L.pgtt_bind(env._h, C.byref(b)) == -1 and missing.encode() in L.pgtt_last_error()
        assert L.pgtt_set_curriculum(env._h, None) == 0 and L.pgtt_bind(env._h, C.byref(b)) == 0        # off: such buffers are fine ...
        assert L.pgtt_set_curriculum(env._h, C.byref(cur_ok)) == -1 and missing.encode() in L.pgtt_last_error()      # ... but not for switching it on
        assert L.pgtt_curriculum(env._h, stream()) == -2                 # still off
        env._bind()
        assert L.pgtt_set_curriculum(env._h, C.byref(cur_ok)) == 0
    bad = abi.curriculum_struct(env.curriculum, None, None)
    assert L.pgtt_set_curriculum(env._h, C.byref(bad)) == -1 and b"level buffer" in L.pgtt_last_error()
    bad = abi.curriculum_struct(dict(env.curriculum, promote_tracking=1.5), env.buffers["level"].data_ptr(), None)
    assert L.pgtt_set_curriculum(env._h, C.byref(bad)) == -1 and b"threshold" in L.pgtt_last_error()
    plain = Joystick("stairs", _cfg(), num_envs=n, terrain=LADDER, device="cuda:0", autoreset=False, variant=torch.zeros(n, dtype=torch.int32))
    assert L.pgtt_set_curriculum(plain._h, C.byref(cur_ok)) == -1 and b"autoreset" in L.pgtt_last_error()
    plain.close()
    env._set_curriculum()                                                # a refused call leaves the handle as it was; this one is the good one again
    snap = lambda e: {k: e.buffers[k].clone() for k in ALL_KEYS if k in e.buffers}

    def untouched(e, s):
        torch.cuda.synchronize()
        return all(_same(e.buffers[k], v) for k, v in s.items())
    # the first reset checks the labels: a level outside [0, L), a variant outside its level's range
    good = {k: env.buffers[k].clone() for k in ("level", "variant")}
    for k, i, v in (("level", 5, 3), ("level", 5, -1), ("variant", 7, int(START[-1]) - 1 if int(good["level"][7]) != 2 else 0)):
        env.buffers[k][i] = v
        s = snap(env)
        assert L.pgtt_reset(env._h, 0, 0, None, stream()) == -1, (k, v)
        assert b"level" in L.pgtt_last_error() and untouched(env, s)
        env.buffers[k].copy_(good[k])
    # a table whose T is not level_start[L]
    env.set_terrain(TABLE[:-1])
    s = snap(env)
    assert L.pgtt_reset(env._h, 0, 0, None, stream()) == -1 and b"level_start" in L.pgtt_last_error() and untouched(env, s)
    env.set_terrain(TABLE)
    env.reset(0)
    # pgtt_curriculum / pgtt_set_curriculum_deferred on a handle without curriculum: PGTT_E_STATE, nothing written
    quiet = _env(n, None, variant=torch.zeros(n, dtype=torch.int32))
    quiet.reset(0)
    quiet.buffers["done"].fill_(1.0)
    s = snap(quiet)
    assert L.pgtt_curriculum(quiet._h, stream()) == -2 and untouched(quiet, s)
    assert L.pgtt_set_curriculum_deferred(quiet._h, 1) == -2
    assert quiet.level is None and "curriculum_stats" not in quiet.buffers and "level" not in quiet.buffers
    with pytest.raises(native.PgttError):
        quiet.curriculum_stats()
    env.close(); quiet.close()


def test_a_stacked_table_with_level_start_is_the_same_ladder():
    """the form train.py uses - ONE stacked table, curriculum=dict(..., level_start=...), level= / variant= from domain_randomize - builds the L-level
    ladder the list form builds; a stacked table without level_start, or with one that does not fit, is refused"""
    n = 256
    dr = domain_randomize(mjcf.load_model("stairs"), n, seed=3, terrain=TABLE, level_start=START, init_level=(0, 2))
    kw = dict(params=torch.from_numpy(dr["params"]), box_friction=torch.from_numpy(dr["box_friction"]), variant=torch.from_numpy(dr["variant"]),
              level=torch.from_numpy(dr["level"]))
    cur = dict(promote_tracking=0.0, demote_length=0.5, init_level=(0, 2))
    a = Joystick("stairs", _cfg(20), num_envs=n, terrain=TABLE, device="cuda:0", autoreset=True, curriculum=dict(cur, level_start=[int(v) for v in START]), **kw)
    b = Joystick("stairs", _cfg(20), num_envs=n, terrain=LADDER, device="cuda:0", autoreset=True, curriculum=dict(cur, seed=3), **{k: kw[k] for k in ("params", "box_friction")})
    for e in (a, b):
        assert len(e.level_start) - 1 == 3 and e.curriculum["level_start"] == [0, 100, 150, 250]
        assert abi.curriculum_struct(e.curriculum).levels == 3
    assert set(a.level.tolist()) == {0, 1, 2}
    assert torch.equal(a.level, b.level) and torch.equal(a.buffers["variant"], b.buffers["variant"])       # one seed, one set of labels
    a.reset(1); b.reset(1)
    zero = torch.zeros(n, 12, device="cuda:0")
    for t in range(45):                                               # episode_length 20, promote_tracking 0: every truncated episode moves up
        a.step(zero); b.step(zero)
    assert _same(a.buffers["state"], b.buffers["state"]) and torch.equal(a.level, b.level)
    st = a.curriculum_stats()
    assert st["promoted"] > 0 and st["finished"] >= 2 * n and bool(_legal(a).all())
    for bad in (dict(cur), dict(cur, level_start=[0, 100, 150]), dict(cur, level_start=[0, 100, 150, 251]), dict(cur, level_start=[5, 100, 150, 250])):
        with pytest.raises(ValueError):
            Joystick("stairs", _cfg(20), num_envs=n, terrain=TABLE, device="cuda:0", autoreset=True, curriculum=bad, **kw)
    with pytest.raises(ValueError):
        Joystick("stairs", _cfg(20), num_envs=n, terrain=LADDER, device="cuda:0", autoreset=True, curriculum=dict(cur, level_start=[0, 100, 250]), **kw)
    a.close(); b.close()


def test_a_short_training_run_and_its_evaluation():
    """train.py over a three-level ladder, the envs starting on levels 1 .. 2: the untrained policy falls early, so envs are demoted, and the mean
    level stays inside (0, 2]: neither can happen on a ladder of fewer levels (a one-level ladder reports level 0, demoted 0, and its reset refuses
    an initial level of 1)"""
    files = "level1,level4,level7"
    ck = os.path.join(ROOT, "checks_stairs", "checkpoint_977")
    shutil.rmtree(ck, ignore_errors=True)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--terrain_files", files, "--curriculum", "--num_envs", "8192", "--num_timesteps", str(4 * 20 * 8192),
                            "--num_evals", "3", "--index", "977", "--curriculum_init", "1,2"], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("steps ")]
        print("\n".join(lines))
        assert lines
        demoted = 0
        for l in lines:
            m = re.search(r"level\s+([0-9.]+)\s+promoted\s+(\d+)\s+demoted\s+(\d+)", l)
            assert m and np.isfinite(float(m.group(1))) and 0.0 < float(m.group(1)) <= 2.0, l
            demoted += int(m.group(3))
        assert demoted > 0, lines
        e = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--checkpoint_folder", ck, "--terrain_files", files, "--level", "1"],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert e.returncode == 0, e.stderr[-3000:]
        assert "survivors" in e.stdout
    finally:
        shutil.rmtree(ck, ignore_errors=True)
