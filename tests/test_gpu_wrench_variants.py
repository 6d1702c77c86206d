"""The twelve physics_kernel<MODE_STEP_XFRC, ...> translation units, each launched with a non-zero wrench and held to fp64.

How a test case selects its unit (launch_physics in csrc/pgtt_api.hip): the launcher table is searched for (subs, mode, dr, terrain) with
  subs    = 1 / 2 / 4 for Joystick(layout="quad" / "oct" / "hex") (PgttConfig.lane_layout; 16 / 8 / 4 envs per wave),
  mode    = MODE_STEP_XFRC because a wrench buffer is bound (Joystick(xfrc=True): PgttBuffers.xfrc != NULL) and the call is a step,
  dr      = 1 when a params buffer is bound (Joystick(params=...)), else the kernel reads masses, torso COM and qpos0 from the model constants,
  terrain = 1 when a terrain table is resident (task "stairs" with level4), 0 on task "flat_terrain".
So layout x dr x task below are the twelve units.  N = 50 envs everywhere: no multiple of 4, 8 or 16, so every layout's last wave is partly
filled (the lanes without an env read the last env's rows and store nothing), and quad still runs four waves.

  a. contact-free twins, one substep: qacc_odd - qacc_even = M^-1 J^T w in fp64, 1e-5 of max |want| (the bar of tests/test_gpu_push.py); a third
     of the pairs carry a pure force of PURE_FORCE newtons perpendicular to the torso's COM offset, on which a kernel that took the arm at the
     body origin would miss the bar by more than a factor 10 (checked on the host before the launch);
  b. mid-stance, one substep: the device's qacc is the fp64 minimiser of oracle.forward's convex problem with qfrc_smooth += J^T w, to the bars of
     parity_explain; the minimiser WITHOUT the wrench must miss them on >= 90 % of the envs checked;
  c. one launch of four substeps = four launches of one substep, as bits, with a wrench held over them (R0 turns in between: the wrench is
     reloaded and re-projected in every substep); a third of the columns carry no wrench and reproduce the zero-wrench launch as bits, every
     other column differs from it;
  d. an all-zero wrench buffer computes the bits of the default path in the nine variants that tests/test_gpu_push.py does not cover.

Each case prints its figures (`WRENCH ...`, pytest -s); DESIGN.md 11 records them."""
import functools
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle
from phase_guided_terrain_traversal_amd import abi, configs, mjcf, policy
from phase_guided_terrain_traversal_amd.env import Joystick
from phase_guided_terrain_traversal_amd.randomize import domain_randomize

import parity_explain as px
from wrench_reference import _hold_action, _minimiser, _model_for, torso_wrench_qfrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERRAIN = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
N = 50
CASES = list(itertools.product(("quad", "oct", "hex"), (False, True), ("flat_terrain", "stairs")))
IDS = [f"{lay}-{'dr' if dr else 'nodr'}-{'level4' if task == 'stairs' else 'flat'}" for lay, dr, task in CASES]
# the force on the pure-force pairs of (a).  60 N, the scale of the other pairs' forces, is enough and was not raised: over the torso's COM offset
# (|base_ipos| = 2.2 cm in the model, +- 5 cm per axis with DR) it makes a torque without which `want` is off by at least 0.22 (model constants) /
# 0.31 (DR rows of seed 5) of its largest entry on every such pair (host arithmetic, no GPU), where the resolving-power check asks for 1e-4
PURE_FORCE = 60.0
BAR_A = 1e-5
OUT_KEYS = ("state", "istate", "frame", "obs_state", "obs_priv", "reward", "done", "metrics")


def _kw(task, dr, n, seed):
    """Joystick keywords of a variant: the terrain table and per-env variant labels on "stairs"; the DR rows (and per-box friction) only with dr"""
    model = mjcf.load_model(task)
    terrain = TERRAIN if task == "stairs" else None
    d = domain_randomize(model, n, seed=seed, terrain=terrain)
    kw = {}
    if dr:
        kw["params"] = torch.from_numpy(d["params"])
    if terrain is not None:
        kw.update(terrain=TERRAIN, variant=torch.from_numpy(d["variant"]))
        if dr:
            kw["box_friction"] = torch.from_numpy(d["box_friction"])
    return kw


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _highest_top(boxes):
    """largest world z reached by a box of the table [B][pos xyz, quat wxyz, half-size xyz], or by the floor (z = 0); the unused rows of a variant
    (unit cubes parked at x = y = z >= 100, terrain_gen.py) are not terrain and do not count"""
    boxes = boxes[np.abs(boxes[:, 0:3]).max(1) < 50.0]
    w, x, y, z = (boxes[:, 3 + i].astype(np.float64) for i in range(4))
    nn = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / nn, x / nn, y / nn, z / nn
    row_z = np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)          # third row of R
    return max(0.0, float((boxes[:, 2] + (np.abs(row_z) * boxes[:, 7:10]).sum(1)).max(initial=0.0)))


def _env_model(model, kw, e):
    """the fp64 model dict of env e: the DR'd one with a params buffer, the model constants without"""
    return _model_for(model, kw["params"].numpy()[:, e]) if "params" in kw else model


@functools.lru_cache(maxsize=None)
def _twins(dr, task):
    """the host side of (a), once per (dr, task) and shared by the three layouts, which only read it: Joystick keywords with twin model rows,
    twin states, the odd twins' wrenches, what the kernel has to compute (want[:, p] = M^-1 J^T w of pair p, fp64), and whether the test could
    tell a wrong arm (resolve: over the pure-force pairs, the smallest distance of M^-1 J^T w with the arm at the body origin from `want`,
    relative to max |want|)"""
    n = N
    model = mjcf.load_model(task)
    kw = _kw(task, dr, n, seed=5)
    if dr:
        kw["params"][:, 1::2] = kw["params"][:, 0::2]            # twins share their model rows
    if "variant" in kw:
        kw["variant"][1::2] = kw["variant"][0::2]
    rng = np.random.default_rng(0)
    rngj = np.asarray(model["jnt_range"], np.float64)
    qpos, qvel = np.zeros((19, n), np.float32), np.zeros((18, n), np.float32)
    w = np.zeros((6, n), np.float32)
    pure = np.zeros(n // 2, bool)
    for p, e in enumerate(range(0, n, 2)):
        q = np.zeros(19)
        q[2] = 1.0 + (_highest_top(TERRAIN[int(kw["variant"][e])]) if "variant" in kw else 0.0)
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(0, 0.6)
        q[3] = np.cos(ang / 2); q[4:7] = np.sin(ang / 2) * ax
        q[7:] = 0.5 * (rngj[:, 0] + rngj[:, 1]) + rng.uniform(-0.1, 0.1, 12) * (rngj[:, 1] - rngj[:, 0])
        v = np.zeros(18); v[:6] = rng.normal(size=6) * 0.3
        qpos[:, e] = qpos[:, e + 1] = q; qvel[:, e] = qvel[:, e + 1] = v
        w[0:3, e + 1] = rng.normal(size=3) * 60.0
        w[3:6, e + 1] = rng.normal(size=3) * 6.0
        if p % 3 == 0:
            m = _env_model(model, kw, e)
            xpos, xquat, xmat, xipos, ximat = mjcf.kinematics_np(m, qpos[:, e].astype(np.float64))
            r = xipos[0] - xpos[0]                               # the COM offset in the world frame
            u = rng.normal(size=3); u -= (u @ r) / (r @ r) * r
            w[0:3, e + 1] = PURE_FORCE * u / np.linalg.norm(u); w[3:6, e + 1] = 0.0
            pure[p] = True
    want = np.zeros((18, n // 2))
    resolve = np.inf
    for p, e in enumerate(range(0, n, 2)):
        m = _env_model(model, kw, e)
        q = qpos[:, e].astype(np.float64)
        M = mjcf.mass_matrix_np(m, q, body_mass=m["body_mass"], body_ipos=m["body_ipos"], armature=m["dof_armature"])
        want[:, p] = np.linalg.solve(M, torso_wrench_qfrc(m, q, w[:, e + 1]))
        if pure[p]:
            wrong = np.linalg.solve(M, torso_wrench_qfrc(m, q, w[:, e + 1], at_origin=True))
            resolve = min(resolve, np.abs(wrong - want[:, p]).max() / np.abs(want[:, p]).max())
    return dict(kw=kw, model=model, qpos=qpos, qvel=qvel, w=w, pure=pure, want=want, resolve=float(resolve))


@pytest.mark.parametrize("layout,dr,task", CASES, ids=IDS)
def test_contact_free_twins_differ_by_minv_jt_w(layout, dr, task):
    """(a) twin envs 1 m above the highest box top of their variant (the floor on flat ground), hinges mid-range, tilt up to 0.6 rad, hold actions,
    one mjx.step per call: the odd twin's wrench (force N(0, 60 N), torque N(0, 6 N m); every third pair a pure force of PURE_FORCE perpendicular
    to the COM offset) moves its last-substep qacc by M^-1 J^T w, J at the torso COM, fp64.  Without DR the COM, masses and qpos0 are the model's."""
    n = N
    tw = _twins(dr, task)
    kw, model, qpos, w, pure, want = (tw[k] for k in ("kw", "model", "qpos", "w", "pure", "want"))
    # ---- on the host, before anything is launched: enough pure-force pairs, and on every one of them the arm at the body origin is more than 10
    #      bars away from the arm at the COM (tests/test_wrench_reference.py asserts the same without a GPU)
    assert pure.sum() * 4 >= n // 2
    assert tw["resolve"] > 10 * BAR_A, tw["resolve"]
    assert (np.abs(want[6:]).max(0) > 0).all()                   # the hinges feel the push through M^-1, not through J^T w
    # ---- device
    cfg = configs.training_config(); cfg["ctrl_dt"] = cfg["sim_dt"]
    env = Joystick(task, cfg, num_envs=n, device="cuda:0", layout=layout, xfrc=True, **kw)
    assert ("params" in env.buffers) == dr
    env.reset(1)
    S = env.buffers["state"]
    st = S.cpu().numpy()
    st[abi.S_QPOS:abi.S_QPOS + 19] = qpos; st[abi.S_QVEL:abi.S_QVEL + 18] = tw["qvel"]; st[abi.S_QWARM:abi.S_QWARM + 18] = 0
    S.copy_(torch.from_numpy(st))
    env.xfrc.copy_(torch.from_numpy(w))
    env.physics(torch.from_numpy(_hold_action(model, qpos, cfg)).cuda())
    torch.cuda.synchronize()
    qacc = env.buffers["state"][abi.S_QWARM:abi.S_QWARM + 18].cpu().numpy().astype(np.float64)
    assert (env.buffers["frame"].cpu().numpy()[abi.F_CONTACT:abi.F_CONTACT + 4] == 0).all()          # contact-free
    err = np.array([np.abs(qacc[:, e + 1] - qacc[:, e] - want[:, p]).max() / np.abs(want[:, p]).max() for p, e in enumerate(range(0, n, 2))])
    print(f"WRENCH a {layout} dr={int(dr)} {task}: worst rel err {err.max():.2e} (pure-force pairs {err[pure].max():.2e}), bar {BAR_A:.0e}, "
          f"arm-at-origin distance {tw['resolve']:.2e}, pure force {PURE_FORCE} N")
    env.close()
    assert err.max() < BAR_A, (err.max(), int(err.argmax()))


@functools.lru_cache(maxsize=None)
def _mid_stance(layout, dr, task):
    """40 steps of policy177 in a default handle of the variant (no wrench buffer): the Joystick keywords, state, istate and the policy's next
    action, on the host; computed once per variant and shared by (b) and (c), which only read it"""
    net = policy.load_policy("policy177", device="cuda:0")
    kw = _kw(task, dr, N, seed=11)
    walk = Joystick(task, configs.training_config(), num_envs=N, device="cuda:0", autoreset=True, layout=layout, **kw)
    walk.reset(3)
    with torch.no_grad():
        for _ in range(40):
            walk.step(net(walk.buffers["obs_state"]))
        act = net(walk.buffers["obs_state"]).float().contiguous()
    torch.cuda.synchronize()
    out = dict(kw=kw, state=walk.buffers["state"].cpu(), istate=walk.buffers["istate"].cpu(), act=act.cpu())
    walk.close()
    return out


def _pushed_handle(layout, task, mid, w, substeps):
    """a handle with a wrench buffer on the mid-stance state, its control step made of `substeps` mjx.steps (1: with the debug buffers)"""
    cfg = configs.training_config()
    if substeps == 1:
        cfg["ctrl_dt"] = cfg["sim_dt"]
    assert round(cfg["ctrl_dt"] / cfg["sim_dt"]) == substeps
    env = Joystick(task, cfg, num_envs=N, device="cuda:0", layout=layout, xfrc=True, debug_contacts=substeps == 1, **mid["kw"])
    env.reset(3)
    env.buffers["state"].copy_(mid["state"]); env.buffers["istate"].copy_(mid["istate"])
    env.xfrc.copy_(torch.from_numpy(w))
    return env


@pytest.mark.parametrize("layout,dr,task", CASES, ids=IDS)
def test_wrench_with_contacts_is_the_convex_minimiser(layout, dr, task):
    """(b) mid-stance states pushed for one substep (force N(0, 40 N), torque N(0, 4 N m)): the device's qacc is the minimiser of the convex
    problem of oracle.forward (qM, efc_J, efc_D, efc_aref) with qfrc_smooth += J^T w, to the bars of parity_explain (envs whose solve stopped
    before the iteration cap); and the minimiser of the problem WITHOUT the wrench is off the device's qacc on >= 90 % of them"""
    n = N
    mid = _mid_stance(layout, dr, task)
    kw = mid["kw"]
    rng = np.random.default_rng(2)
    w = np.concatenate([rng.normal(size=(3, n)) * 40.0, rng.normal(size=(3, n)) * 4.0]).astype(np.float32)
    env = _pushed_handle(layout, task, mid, w, 1)
    assert ("params" in env.buffers) == dr
    cfg = env.config
    act = mid["act"].cuda()
    st0 = mid["state"].numpy().astype(np.float64)
    env.physics(act)
    torch.cuda.synchronize()
    qacc = env.buffers["state"][abi.S_QWARM:abi.S_QWARM + 18].cpu().numpy().astype(np.float64)
    niter = env.buffers["dbg_niter"].cpu().numpy() & 0xFFFF
    env.close()
    model = mjcf.load_model(task)
    ms = abi.model_struct(model)
    key = np.asarray(model["key_qpos"], np.float32)
    act_np = mid["act"].numpy()
    prm = kw["params"].numpy() if dr else None
    var = kw["variant"].numpy() if "variant" in kw else None
    bf = kw["box_friction"].numpy() if "box_friction" in kw else None
    checked, off, with_contacts, blind = 0, 0, 0, 0
    for e in range(n):
        if niter[e] >= int(model["iterations"]):
            continue
        ctrl = (key[7:] + act_np[e] * np.float32(cfg["action_scale"])).astype(np.float64)
        qpos = st0[abi.S_QPOS:abi.S_QPOS + 19, e]
        D = oracle.forward(ms, qpos, st0[abi.S_QVEL:abi.S_QVEL + 18, e], ctrl, warm=st0[abi.S_QWARM:abi.S_QWARM + 18, e],
                           boxes=None if var is None else TERRAIN[var[e]], box_friction=None if bf is None else bf[:, e],
                           params=None if prm is None else prm[:, e])
        jtw = torso_wrench_qfrc(_env_model(model, kw, e), qpos, w[:, e])
        dv, rel = px.off_minimiser(qacc[:, e], _minimiser(D, D["qfrc_smooth"] + jtw), cfg["sim_dt"])
        checked += 1
        off += px.is_off(dv, rel)
        with_contacts += int((np.asarray(D["efc_active"]) != 0).any())
        blind += not px.is_off(*px.off_minimiser(qacc[:, e], _minimiser(D, D["qfrc_smooth"]), cfg["sim_dt"]))
    print(f"WRENCH b {layout} dr={int(dr)} {task}: checked {checked} / {n}, with contacts {with_contacts}, off {off}, "
          f"no-wrench minimiser off on {checked - blind} / {checked}")
    assert checked >= n // 2 and with_contacts >= checked // 2, (checked, with_contacts)
    # the cap of the parity suite's W: a contact whose distance is within rounding of 0 may be in one problem and not the other
    assert off <= 1 + checked // 50, (off, checked)
    # resolving power: a kernel that dropped the wrench would be caught
    assert checked - blind >= 0.9 * checked, (blind, checked)


@pytest.mark.parametrize("layout,dr,task", CASES, ids=IDS)
def test_four_substeps_with_a_wrench_are_four_launches(layout, dr, task):
    """(c) one launch of the control step's kernel (4 substeps) ends on the bits of four one-substep launches of the same kernel instance, with
    the same wrench bound (the state round-trips through HBM instead of registers, the wrench is read again either way); columns e % 3 == 2
    carry no wrench: they end on the bits of the launch with an all-zero buffer, every other column differs from that launch"""
    n = N
    mid = _mid_stance(layout, dr, task)
    rng = np.random.default_rng(6)
    w = np.concatenate([rng.normal(size=(3, n)) * 40.0, rng.normal(size=(3, n)) * 4.0]).astype(np.float32)
    quiet = np.arange(n) % 3 == 2
    w[:, quiet] = 0.0
    act = mid["act"].cuda()
    A = _pushed_handle(layout, task, mid, w, 4)
    A.physics(act)
    torch.cuda.synchronize()
    fin = A.buffers["state"][:55].cpu().numpy()
    B = _pushed_handle(layout, task, mid, w, 1)
    for _ in range(4):
        B.physics(act)
    torch.cuda.synchronize()
    rep = B.buffers["state"][:55].cpu().numpy()
    B.close()
    A.buffers["state"].copy_(mid["state"]); A.buffers["istate"].copy_(mid["istate"]); A.xfrc.zero_()
    A.physics(act)
    torch.cuda.synchronize()
    zero = A.buffers["state"][:55].cpu().numpy()
    A.close()
    assert np.isfinite(fin).all()
    fb, rb, zb = fin.view(np.int32), rep.view(np.int32), zero.view(np.int32)
    moved = (fb != zb).any(0)
    print(f"WRENCH c {layout} dr={int(dr)} {task}: columns differing between 1 x 4 and 4 x 1 substeps {int((fb != rb).any(0).sum())}, "
          f"wrenched columns that moved {int(moved[~quiet].sum())} / {int((~quiet).sum())}, zero columns that moved {int(moved[quiet].sum())} / {int(quiet.sum())}")
    assert np.array_equal(rb, fb), np.abs(rep - fin).max()
    assert moved[~quiet].all(), np.flatnonzero(~moved & ~quiet)
    assert not moved[quiet].any(), np.flatnonzero(moved & quiet)


@pytest.mark.parametrize("layout,dr,task", [c for c in CASES if not (c[1] and c[2] == "stairs")],
                         ids=[i for i, c in zip(IDS, CASES) if not (c[1] and c[2] == "stairs")])
def test_zero_wrench_is_the_default_path(layout, dr, task):
    """(d) a bound all-zero xfrc computes the bits of xfrc = NULL in the nine variants other than DR + level4 (tests/test_gpu_push.py has those):
    10 steps of random actions with autoreset, every output buffer each step"""
    n = N
    kw = _kw(task, dr, n, seed=3)
    a = Joystick(task, configs.training_config(), num_envs=n, device="cuda:0", autoreset=True, layout=layout, **kw)
    b = Joystick(task, configs.training_config(), num_envs=n, device="cuda:0", autoreset=True, layout=layout, xfrc=True, **kw)
    assert a.xfrc is None and b.xfrc is not None and float(b.xfrc.abs().sum()) == 0.0
    a.reset(7); b.reset(7)
    rng = np.random.default_rng(8)
    for t in range(10):
        act = torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.5).astype(np.float32)).cuda()
        a.step(act); b.step(act)
        for k in OUT_KEYS:
            assert _same(a.buffers[k], b.buffers[k]), (t, k)
    torch.cuda.synchronize()
    assert float(b.xfrc.abs().sum()) == 0.0
    a.close(); b.close()
