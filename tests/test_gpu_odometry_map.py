"""The elevation map on the estimated pose of pgtt_elevation_odometry (include/pgtt_elevation.h, "Odometry drift"), on the GPU.
  1. Composition at zero settings: a map bound to pose_est and points_est has the bits of a map bound to the true state and the LiDAR's points, for
     the plain tick, the points tick, the fill, the variance tick (both sources) and the follow call behind a sensor of period 3.
  2. Composition under an error set by hand: the image tick under pose_est is held to tests/elevation_reference.py fed the DEVICE's pose_est, with
     that file's exclusions and the caps of tests/test_gpu_elevation.py (at most 5 % of the touched cells and of the scan points left out; the bar
     2e-5 (1 + |reference|)).  The poses are chosen by rejection on the CPU so that the base and every scan point, under the true and under the
     estimated pose, lie at least 1e-4 m from a cell border: the reference alone then stays inside the caps.
  3. The env: Joystick(elevation=dict(odometry=...)) with both sources."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_reference as ref  # noqa: E402
import odometry_reference as oref  # noqa: E402
from test_gpu_elevation import EPS, RES, VARIANTS, Tally, _bits, compare, make_env  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, elevation  # noqa: E402

pytestmark = pytest.mark.gpu

ZERO = dict(oref.ZERO)
MARGIN = 1e-4                                    # tests/test_gpu_elevation_fill.py's
OUTS = ("map", "origin", "est", "known", "obs", "var", "est_var", "filled_est", "filled_dist", "filled_obs", "filled_map", "filled_dist_map")
LIDAR = dict(n_az=32, n_el=8)


def same_bits(a, b, where):
    n = 0
    for k in OUTS:
        if hasattr(a, k):
            assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), (k, where)
            n += 1
    return n


# ---------------------------------------------------------------- 1. composition at zero settings
def test_zero_settings_compose_to_the_same_bits():
    """8 envs, a 48 x 32 image, G = 24, the reset and 6 steps on level4, env 5 thrown on its back in step 3 so that use_done clears a map"""
    n = 8
    env = make_env(n, 5, depth=dict(width=48, height=32), lidar=LIDAR, autoreset=True)
    slow = make_env(n, 5, depth=dict(width=48, height=32, every=3), autoreset=True)
    kinds = {"plain, fill": (env, dict(fill=8, dense=True)), "points, fill": (env, dict(source="lidar", fill=8, dense=True)),
             "variance": (env, dict(variance=True)), "variance, points": (env, dict(source="lidar", variance=True)),
             "follow": (slow, dict(follow_sensor=True))}
    maps = {k: (elevation.ElevationMap(e, grid=24, **kw, odometry=ZERO), elevation.ElevationMap(e, grid=24, **kw), e) for k, (e, kw) in kinds.items()}
    rng = np.random.default_rng(8)
    compared = 0
    for t in range(7):
        if t > 0:
            if t == 3:
                for e in (env, slow):
                    e.buffers["state"][abi.S_QPOS + 3:abi.S_QPOS + 7, 5] = torch.tensor([0.0, 1.0, 0.0, 0.0], device="cuda:0")
            act = torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda()
            env.step(act); slow.step(act)
        for name, (with_odo, without, e) in maps.items():
            for m in (with_odo, without):
                m.tick(clear_all=t == 0, use_done=t > 0, force=t == 0)
            torch.cuda.synchronize()
            compared += same_bits(with_odo, without, (name, t))
            assert torch.equal(with_odo.pose_est, e.buffers["state"][:7]), (name, t)                     # by ==
            assert (with_odo.odo[:, 0:4] == 0).all() and int(with_odo.odo_counter.item()) == t + 1
            if with_odo.source == "lidar":
                assert np.array_equal(with_odo.points_est.cpu().numpy(), e.lidar_scanner.points.cpu().numpy(), equal_nan=True), (name, t)
        if t == 3:
            assert env.buffers["done"][5] != 0
    assert compared == 7 * (10 + 10 + 7 + 7 + 5)
    assert not hasattr(maps["plain, fill"][1], "pose_est") and maps["plain, fill"][1].odometry is None
    assert torch.isfinite(maps["plain, fill"][0].map).any() and torch.isfinite(maps["follow"][0].map).any()
    for a, b, _ in maps.values():
        a.close(); b.close()
    env.close(); slow.close()


# ---------------------------------------------------------------- 2. composition under an error
ERR, PSI = np.array([0.13, -0.07, 0.02], np.float32), np.float32(0.1)


def estimated(qpos):
    """the pose estimate of a true pose [7] (fp32 values) under ERR and PSI, as the fp64 reference states it, rounded to fp32 as the device stores it"""
    est = np.concatenate([qpos[0:3] + ERR.astype(float), oref.qz_mul(np.array([float(PSI)]), qpos[3:7, None])[:, 0]])
    return est.astype(np.float32).astype(float)


def safe(qpos, res):
    return min(ref.border_margin(qpos[None, :2], res)[0], ref.border_margin(ref.scan_points(qpos), res).min()) >= MARGIN


def test_image_tick_under_a_drifted_pose():
    G, res32 = 64, float(np.float32(RES))
    env = make_env(3, 11, variant=VARIANTS, depth=dict(width=48, height=32))
    rng = np.random.default_rng(5)
    for _ in range(6):
        env.step(torch.from_numpy(np.tanh(rng.normal(size=(3, 12)) * 0.4).astype(np.float32)).cuda())
    torch.cuda.synchronize()
    S = env.buffers["state"]
    q = S[:7].cpu().numpy().astype(float)
    tries = 0
    for e in range(3):                                               # rejection, on the CPU: the base moved by up to a cell
        while True:
            tries += 1
            cand = q[:, e].copy()
            cand[0:2] = (cand[0:2] + rng.uniform(-RES, RES, 2)).astype(np.float32)
            if safe(cand, res32) and safe(estimated(cand), res32):
                q[:, e] = cand
                break
    S[:7] = torch.from_numpy(q.astype(np.float32)).cuda()
    env.depth_camera.tick(force=True)
    em = elevation.ElevationMap(env, grid=G, res=RES, odometry=ZERO)
    truth = elevation.ElevationMap(env, grid=G, res=RES)
    cam = env.depth_camera.config
    cfg = dict(fovy=cam.fovy_deg, near=cam.near, far=cam.far, mount_pos=tuple(cam.mount_pos), mount_quat=tuple(cam.mount_quat), res=RES, alpha=1.0,
               self_half=elevation.DEFAULTS["self_half"])
    img, obs = env.depth.cpu().numpy(), env.buffers["obs_state"].cpu().numpy()
    state32 = S[:7].cpu().numpy()
    states, doubtful, tally = [ref.new_state(G) for _ in range(3)], [set() for _ in range(3)], Tally()
    for t in range(2):
        if t == 1:
            em.odo[:, 0:3] = torch.from_numpy(ERR).cuda()
            em.odo[:, 3] = float(PSI)
        em.tick(clear_all=t == 0)
        truth.tick(clear_all=t == 0)
        torch.cuda.synchronize()
        pose = em.pose_est.cpu().numpy()
        odo = em.odo.cpu().numpy()
        if t == 0:
            assert np.array_equal(pose, state32) and (odo[:, 0:4] == 0).all() and (odo[:, 7:9] == 0).all()
        else:
            # a step of length 0 under zero sigmas leaves the error that was set, and the estimate is the fp64 one to a few roundings
            assert np.array_equal(odo[:, 0:3], np.tile(ERR, (3, 1))) and (odo[:, 3] == PSI).all()
            want_pose = np.stack([estimated(state32[:, e].astype(float)) for e in range(3)], 1)
            assert np.abs(pose - want_pose).max() <= 4 * 2.0 ** -24 * np.abs(want_pose).max()
        got = {k: getattr(em, k).cpu().numpy().copy() for k in ("map", "origin", "est", "known", "obs")}
        for e in range(3):
            want = ref.tick(states[e], pose[:, e].astype(float), img[e], cfg, clear=t == 0)
            want["obs_in"] = obs[e]
            wc = ref.world_cells(want["origin"], G)
            doubtful[e] -= {tuple(c) for c in wc[want["touched"]]}                         # alpha = 1: a touched cell is replaced
            doubtful[e] &= {tuple(c) for c in wc.reshape(-1, 2)}
            doubtful[e] |= ref.doubtful_cells(want, cfg["res"], EPS)
            compare(got, e, want, doubtful[e], tally, G)
            states[e] = (want["map"], want["origin"])
    cells, scan = tally.shares()
    print(f"drifted pose, 48x32 G={G}: {tries} poses tried, touched {tally.touched}, left out {tally.touched_out} ({100 * cells:.2f} %), scan left out "
          f"{tally.scan_out} of {tally.scan} ({100 * scan:.2f} %), worst error / bar: map {tally.worst_map:.3f}, est {tally.worst_est:.3f}; est held as it "
          f"stands in {tally.est_strict} of {tally.est_ticks} env-ticks")
    assert tally.touched >= 20 and tally.est_strict >= 1 and cells <= 0.05 and scan <= 0.05
    # the error is seen by the map: 13 and 7 cm are more than three and one cell
    assert not np.array_equal(em.origin.cpu().numpy(), truth.origin.cpu().numpy())
    assert not np.array_equal(_bits(em.est), _bits(truth.est))
    em.close(); truth.close(); env.close()


# ---------------------------------------------------------------- 3. the env
def sensors(source):
    return dict(lidar=LIDAR) if source == "lidar" else dict(depth=dict(width=48, height=32))


def with_map(source, **kw):
    return dict({} if source == "depth" else dict(source="lidar"), grid=24, **kw)


@pytest.mark.parametrize("source", ["depth", "lidar"])
def test_env_with_zero_settings_has_the_bits_of_an_env_without(source):
    n = 8
    a = make_env(n, 5, **sensors(source), elevation=with_map(source, odometry=ZERO), autoreset=True)
    b = make_env(n, 5, **sensors(source), elevation=with_map(source), autoreset=True)
    assert b.odometry_error is None and b.odometry_pose is None and a.odometry_error.shape == (n, 4) and a.odometry_pose.shape == (7, n)
    assert a.odometry_error.data_ptr() == a.elevation_map.odo.data_ptr()                      # a view
    rng = np.random.default_rng(6)
    for t in range(6):
        if t > 0:
            act = torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda()
            a.step(act); b.step(act)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(a.elevation_obs), _bits(b.elevation_obs)) and np.array_equal(_bits(a.elevation_known), _bits(b.elevation_known)), t
        assert torch.equal(a.odometry_pose, a.buffers["state"][:7]) and (a.odometry_error == 0).all()
    assert (a.elevation_known != 0).any()
    a.close(); b.close()


@pytest.mark.parametrize("source", ["depth", "lidar"])
def test_env_with_the_defaults_drifts_and_an_episodes_end_clears_it(source):
    n = 8
    a = make_env(n, 5, **sensors(source), elevation=with_map(source, odometry=True), autoreset=True)
    b = make_env(n, 5, **sensors(source), elevation=with_map(source, odometry=True), autoreset=True)
    assert a.elevation_map.odometry == elevation.ODOMETRY_DEFAULTS
    torch.cuda.synchronize()
    assert (a.odometry_error == 0).all() and torch.equal(a.odometry_pose, a.buffers["state"][:7])                     # after reset()
    assert (a.elevation_map.odo[:, 7:9] != 0).all()                                           # the episode's draws
    rng = np.random.default_rng(6)
    for t in range(1, 6):
        if t == 5:                                                                            # env 5 on its back: its episode ends in this step
            for env in (a, b):
                env.buffers["state"][abi.S_QPOS + 3:abi.S_QPOS + 7, 5] = torch.tensor([0.0, 1.0, 0.0, 0.0], device="cuda:0")
        act = torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda()
        a.step(act); b.step(act)
        torch.cuda.synchronize()
        for x, y in ((a.elevation_obs, b.elevation_obs), (a.elevation_map.odo, b.elevation_map.odo), (a.odometry_pose, b.odometry_pose)):
            assert np.array_equal(_bits(x), _bits(y)), t                                      # two envs built alike
        if t == 4:
            assert (a.odometry_error[:, 0:2] != 0).any(1).all() and (a.odometry_error[:, 3] != 0).all()
            before = a.elevation_map.odo[:, 7:9].clone()
    done = a.buffers["done"].cpu().numpy() != 0
    err = a.odometry_error.cpu().numpy()
    assert done[5] and (err[done] == 0).all() and (err[~done][:, 3] != 0).all()
    assert torch.equal(a.odometry_pose[:, 5], a.buffers["state"][:7, 5])
    assert (a.elevation_map.odo[5, 7:9] != before[5]).all() and torch.equal(a.elevation_map.odo[~torch.from_numpy(done).cuda(), 7:9], before[~torch.from_numpy(done).cuda()])
    assert int(a.elevation_map.odo_counter.item()) == 6
    a.close(); b.close()


# ---------------------------------------------------------------- 4. evaluate.py
def test_evaluate_reports_the_drift_and_is_unchanged_without_the_flag(capsys):
    """--odometry_drift adds two keys and one printed line; all-zero values give the figures of a run without the flag, which has neither"""
    import evaluate
    base = ["--policy", "policy177", "--terrain_file", "level4", "--elevation"]
    run = lambda *extra, verbose=False: evaluate.run_evaluation(evaluate.make_parser().parse_args(base + list(extra)), num_eval_envs=32, verbose=verbose)
    plain = run(verbose=True)
    said = capsys.readouterr().out
    assert "odometry_e_xy" not in plain and "odometry" not in said and len(said.strip().splitlines()) == 2
    zero = run("--odometry_drift", "0,0,0,0,0")
    assert zero.pop("odometry_e_xy") == 0 and zero.pop("odometry_psi") == 0 and zero == plain
    drift = run("--odometry_drift", verbose=True)
    said = capsys.readouterr().out.strip().splitlines()
    assert len(said) == 3 and said[2].startswith("odometry drift at the end") and said[:2] == [str(drift["episode_reward"]), str([drift["survivors"]])]
    assert 0.01 < drift["odometry_e_xy"] < 1.0 and 0.005 < drift["odometry_psi"] < 0.5          # 20 s at the defaults: centimetres, hundredths of a radian
