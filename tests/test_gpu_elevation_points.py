"""pgtt_elevation_points on the GPU: the kernel's points instantiation against the fp64 statement of tests/elevation_points_reference.py under
the rules of tests/test_gpu_elevation.py (its `compare`, EPS = 2e-5, its caps of 5 %), the kernel's other paths, batch independence, determinism,
the four clears, the call-order refusals, graph capture, both sources on one handle, and Joystick(lidar=..., elevation=dict(source="lidar")).

The device and the reference read the same fp32 points, so a cell is in doubt only when a point lies within 2e-5 m of a cell border or of
changing sides of the self-filter box."""
import ctypes as C
import os
import sys
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_points_reference as pref  # noqa: E402
import elevation_reference as ref  # noqa: E402
from test_gpu_elevation import EPS, FAR_CELLS, NTICK, RES, VARIANTS, Tally, _bits, compare, make_env, recorded  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, elevation, lidar  # noqa: E402

pytestmark = pytest.mark.gpu

ANGLES = ((-180.0, 180.0), (-85.0, 10.0))
PATTERNS = {1024: (64, 16), 96: (16, 6)}
OUT = ("map", "origin", "est", "known", "obs")


@lru_cache(maxsize=None)
def recorded_points(P):
    """NTICK consecutive (state [NSTATE, 3], points [3, P, 3], obs [3, 171]) of three envs on three variants of level4, as numpy: the scene of
    test_gpu_elevation.recorded() - the poses after six small random actions, the bases moved by hand between the ticks, inside a cell, by five
    cells, by more than G cells - seen by the chin LiDAR of lidar.DEFAULTS with the robot in view, at 64 x 16 (P = 1024) or 16 x 6 rays (P = 96);
    P = 1000 is the first 1000 points of the 1024.  Computed once per pattern and shared."""
    if P == 1000:
        return [(S, pts[:, :1000].copy(), obs) for S, pts, obs in recorded_points(1024)]
    n_az, n_el = PATTERNS[P]
    env = make_env(3, 11, variant=VARIANTS, lidar=dict(n_az=n_az, n_el=n_el, az_deg=ANGLES[0], el_deg=ANGLES[1]))
    rng = np.random.default_rng(5)
    for _ in range(6):
        env.step(torch.from_numpy(np.tanh(rng.normal(size=(3, 12)) * 0.4).astype(np.float32)).cuda())
    S = env.buffers["state"]
    xy = S[0:2].cpu().numpy().astype(float)
    xy[:, 2] = (-1.3, -0.7)
    cells = np.floor(xy / RES)
    frac = np.tile(np.array([[0.37], [0.61]]), (1, 3))
    small, several, far = None, np.array([5, -3]), np.array([FAR_CELLS, 0])
    moves = [None, (small, several, far), (-several, -far, small)]
    out = []
    for t in range(NTICK):
        for e, mv in enumerate(moves[t] or ()):
            if mv is None:
                frac[:, e] = (0.57, 0.41)
            else:
                cells[:, e] += mv
        S[0:2] = torch.from_numpy(((cells + frac) * RES).astype(np.float32)).cuda()
        env.lidar_scanner.tick(force=True)
        torch.cuda.synchronize()
        out.append((S.cpu().numpy().copy(), env.lidar_points.cpu().numpy().copy(), env.buffers["obs_state"].cpu().numpy().copy()))
    env.close()
    return out


def shrunk(ticks, scale):
    """the same clouds drawn toward each base in x and y (in fp32: what the device and the reference both read), so that a small window is hit"""
    if scale == 1.0:
        return ticks
    out = []
    for S, pts, obs in ticks:
        p = pts.copy()
        base = S[0:2].T[:, None, :].astype(np.float32)                               # [3, 1, 2]
        p[..., :2] = base + np.float32(scale) * (p[..., :2] - base)
        out.append((S, p, obs))
    return out


class Rig:
    """what ElevationMap(source="lidar") reads of an env - state, points, observation, done - as tensors the test fills, and the map on them"""

    def __init__(self, n, P, obs_dim=171, **settings):
        dev = torch.device("cuda:0")
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)
        scanner = types.SimpleNamespace(points=torch.full((n, P, 3), float("nan"), device=dev), config=types.SimpleNamespace(every=1))
        self.env = types.SimpleNamespace(lidar_scanner=scanner, buffers={"state": z(abi.NSTATE, n), "obs_state": z(n, obs_dim), "done": z(n)}, device=dev,
                                         num_envs=n, observation_size={"state": obs_dim}, config=dict(scan_dist_x=0.1, scan_dist_y=0.1), method="pgtt")
        self.map = elevation.ElevationMap(self.env, source="lidar", **settings)

    def put(self, state, points, obs=None):
        self.env.buffers["state"].copy_(torch.from_numpy(np.ascontiguousarray(state)))
        self.env.lidar_scanner.points.copy_(torch.from_numpy(np.ascontiguousarray(points)))
        if obs is not None:
            self.env.buffers["obs_state"].copy_(torch.from_numpy(np.ascontiguousarray(obs)))

    def tick(self, **kw):
        self.map.tick(**kw)
        torch.cuda.synchronize()
        return {k: getattr(self.map, k).cpu().numpy().copy() for k in OUT}

    def close(self):
        self.map.close()


def run_sequence(rig, ticks, cfg, G, tally):
    """test_gpu_elevation.run_sequence with the points reference"""
    states = [pref.new_state(G) for _ in range(3)]
    doubtful = [set() for _ in range(3)]
    for t, (S, pts, obs) in enumerate(ticks):
        rig.put(S, pts, obs)
        got = rig.tick(clear_all=t == 0)
        for e in range(3):
            want = pref.tick(states[e], S[:7, e], pts[e], cfg, clear=t == 0)
            want["obs_in"] = obs[e]
            wc = pref.world_cells(want["origin"], G)
            if cfg["alpha"] == 1.0:
                doubtful[e] -= {tuple(c) for c in wc[want["touched"]]}
            doubtful[e] &= {tuple(c) for c in wc.reshape(-1, 2)}
            doubtful[e] |= pref.doubtful_cells(want, cfg["res"], EPS)
            compare(got, e, want, doubtful[e], tally, G)
            states[e] = (want["map"], want["origin"])


# ---------------------------------------------------------------- 1. parity
# G = 8 / 9 and G = 24 are windows of 0.32 m and 0.96 m around the base; the chin LiDAR's nearest floor returns lie 0.3 m ahead of it and its returns from
# the robot's own legs are what the self filter is for.  Those cases draw the cloud toward the base in x and y, by 0.4, so that it lands in the
# window, and run without the self filter (G < 24, the kernel's other path) or with a small box (G = 24); G = 64 takes the cloud as it is, with the
# default box.  The factor is chosen from the count of points alone, as test_gpu_elevation chooses its camera positions: a point is within 2e-5 m
# of a border with probability 4 x 2e-5 / 0.04 = 0.2 %, and puts up to four cells in doubt, which with alpha = 0.5 stay in doubt for the
# sequence, so the share left out grows with the points per cell.  Drawn in by 0.15, seven of ten points of a 1024-ray scan fall into the 64 cells
# of G = 8 and 5.2 - 5.5 % of the touched cells are left out with alpha = 0.5 (by the reference alone: the device reads the same points); drawn in
# by 0.4, a third as many land there and 2.6 - 3.2 % are.
# G = 9 is the odd size, where a map is not a whole number of 16-byte runs; P = 1000 is no multiple of the 256 lanes and P = 96 less than one pass.
CASES = [(G, a, P) for G in (8, 9, 24, 64) for a in (1.0, 0.5) for P in (96, 1000, 1024)]


def case_setup(G):
    if G < 24:
        return 0.4, dict(grid=G, res=RES, self_half=(0.0, 0.0, 0.0))
    if G == 24:
        return 0.4, dict(grid=G, res=RES, self_half=(0.12, 0.1, 0.45))
    return 1.0, dict(grid=G, res=RES, self_half=(0.45, 0.25, 0.45))


@pytest.mark.parametrize("G,alpha,P", CASES)
def test_parity(G, alpha, P):
    """Left out per case, three envs and three ticks pooled, alpha = 1 / alpha = 0.5 where they differ.  The device reads the points the reference
    reads, so these are the reference's own shares and the same in every run (measured on an MI355X, the device agreeing on every compared cell):

         G      P    touched cells   left out, cells              left out, scan points (of 1053)
         8     96        175          0         0.00 %             3        0.28 %
         8   1000        434         12 / 13    2.76 / 3.00 %      5        0.47 %
         8   1024        444         12 / 13    2.70 / 2.93 %      5        0.47 %
         9     96        233          0         0.00 %             3        0.28 %
         9   1000        569         15 / 18    2.64 / 3.16 %      5 / 6    0.47 / 0.57 %
         9   1024        579         15 / 18    2.59 / 3.11 %      5 / 6    0.47 / 0.57 %
        24     96        256          0         0.00 %             3        0.28 %
        24   1000       1271         20 / 24    1.57 / 1.89 %      7 / 8    0.66 / 0.76 %
        24   1024       1298         20 / 24    1.54 / 1.85 %      7 / 8    0.66 / 0.76 %
        64     96        198          1         0.51 %             4        0.38 %
        64   1000       2103         11 / 14    0.52 / 0.67 %     13        1.23 %
        64   1024       2127         11 / 14    0.52 / 0.66 %     13        1.23 %

    against the caps of 5 % each.  The worst error on the compared cells is 0.001 of the bar (the fuse with alpha = 0.5; with alpha = 1 a cell is
    one of the points, bit for bit), on `est` 0.001 of it; `est` was held as it stands in every env-tick with a known compared point."""
    scale, settings = case_setup(G)
    settings["alpha"] = alpha
    ticks = shrunk(recorded_points(P), scale)
    rig = Rig(3, P, **settings)
    tally = Tally()
    run_sequence(rig, ticks, dict(res=RES, alpha=alpha, self_half=settings["self_half"]), G, tally)
    rig.close()
    cells, scan = tally.shares()
    print(f"points G={G} alpha={alpha} P={P}: touched {tally.touched}, left out {tally.touched_out} ({100 * cells:.2f} %), scan left out {tally.scan_out} of "
          f"{tally.scan} ({100 * scan:.2f} %), worst error / bar: map {tally.worst_map:.3f}, est {tally.worst_est:.3f}; est held as it stands in "
          f"{tally.est_strict} of {tally.est_ticks} env-ticks")
    assert tally.touched >= 20, "the case would be vacuous"
    assert tally.est_strict >= 1, "the subtraction of the minimum was never checked"
    assert cells <= 0.05 and scan <= 0.05


# ---------------------------------------------------------------- 2. the kernel's other paths
def test_points_that_are_all_nan_and_the_self_filter_off():
    ticks = recorded_points(1024)
    S, pts, obs = ticks[0]
    G = 64
    rig = Rig(3, 1024, grid=G, res=RES, alpha=1.0, self_half=(0.0, 0.0, 0.0))
    bad = pts.copy()
    bad[0] = np.nan                                                               # no return at all
    bad[1, :, 0] = np.inf                                                         # one coordinate not finite in every row
    rig.put(S, bad, obs)
    got = rig.tick(clear_all=True)
    assert np.isnan(got["map"][0]).all() and np.isnan(got["map"][1]).all()
    assert (got["est"][:2] == 0).all() and (got["known"][:2] == 0).all() and np.isfinite(got["est"]).all() and not np.isinf(got["map"]).any()
    # env 2, the filter off: the robot's own returns are in the map, and the reference agrees
    cfg = dict(res=RES, alpha=1.0, self_half=(0.0, 0.0, 0.0))
    want = pref.tick(pref.new_state(G), S[:7, 2], pts[2], cfg, clear=True)
    want["obs_in"] = obs[2]
    tally = Tally()
    compare(got, 2, want, pref.doubtful_cells(want, RES, EPS), tally, G)
    filtered = pref.tick(pref.new_state(G), S[:7, 2], pts[2], dict(cfg, self_half=(0.45, 0.25, 0.45)), clear=True)
    assert want["touched"].sum() > filtered["touched"].sum() > 20
    rig.close()


# ---------------------------------------------------------------- 3. batch independence, determinism
def _two_ticks(n, P, ticks, cols, **settings):
    rig = Rig(n, P, **settings)
    for t in range(2):
        S, pts, obs = ticks[t]
        rig.put(S[:, cols], pts[cols], obs[cols])
        got = rig.tick(clear_all=t == 0)
    rig.close()
    return got


def test_batch_independence_and_determinism():
    ticks = recorded_points(1000)
    settings = dict(grid=64, res=RES, alpha=0.5, self_half=(0.45, 0.25, 0.45))
    three = _two_ticks(3, 1000, ticks, [0, 1, 2], **settings)
    again = _two_ticks(3, 1000, ticks, [0, 1, 2], **settings)
    big = _two_ticks(8, 1000, ticks, [0] + [1] * 6 + [2], **settings)
    for k in three:
        assert np.array_equal(_bits(three[k]), _bits(again[k])), k                     # determinism
    assert (~np.isnan(three["map"])).sum() > 50
    for e, pos in ((0, 0), (2, 7)):
        alone = _two_ticks(1, 1000, ticks, [e], **settings)
        for k in three:
            assert np.array_equal(_bits(three[k][e]), _bits(alone[k][0])), (k, e)
            assert np.array_equal(_bits(three[k][e]), _bits(big[k][pos])), (k, e)


# ---------------------------------------------------------------- 4. clears
@pytest.mark.parametrize("name,kw,done,cleared", [("clear_all", dict(clear_all=True), (0, 0, 0), (1, 1, 1)),
                                                  ("mask", dict(clear_mask=(0, 1, 0)), (0, 0, 0), (0, 1, 0)),
                                                  ("use_done", dict(use_done=True), (0, 1, 0), (0, 1, 0)),
                                                  ("done_not_used", dict(use_done=False), (1, 1, 1), (0, 0, 0))])
def test_clears(name, kw, done, cleared):
    S, pts, obs = recorded_points(96)[0]
    rig = Rig(3, 96, grid=64, res=RES, alpha=1.0, self_half=(0.45, 0.25, 0.45))
    rig.put(S, pts, obs)
    first = rig.tick(clear_all=True)                                              # the origin is the pose's from here on: nothing is stale
    rig.map.map.fill_(5.0)
    rig.env.buffers["done"].copy_(torch.tensor(done, dtype=torch.float32))
    if "clear_mask" in kw:
        kw = dict(kw, clear_mask=torch.tensor(kw["clear_mask"], dtype=torch.uint8))
    got = rig.tick(**kw)
    touched = ~np.isnan(first["map"])
    assert touched.sum() > 20
    for e in range(3):
        if cleared[e]:                                                            # cleared BEFORE integrating: this tick's cells and nothing else
            assert np.array_equal(_bits(got["map"][e]), _bits(first["map"][e])), (name, e)
        else:
            assert (got["map"][e][~touched[e]] == 5.0).all() and np.array_equal(_bits(got["map"][e][touched[e]]), _bits(first["map"][e][touched[e]])), (name, e)
    rig.close()


# ---------------------------------------------------------------- 5. call order; both sources on one handle
def _raw_handle(camera, n, G=64):
    L = elevation.lib()
    cfg = elevation.config_struct(camera["width"], camera["height"], camera["fovy"], camera["near"], camera["far"], camera["mount_pos"], camera["mount_quat"],
                                  grid=G, res=RES, alpha=1.0, self_half=(0.45, 0.25, 0.45))
    h = C.c_void_p()
    assert L.pgtt_elevation_create(C.byref(cfg), 0, n, C.byref(h)) == 0
    dev = "cuda:0"
    t = dict(map=torch.full((n, G, G), float("nan"), device=dev), origin=torch.zeros((n, 2), dtype=torch.int32, device=dev),
             est=torch.full((n, 117), -7.0, device=dev), known=torch.zeros((n, 117), dtype=torch.uint8, device=dev), obs=torch.full((n, 171), -7.0, device=dev))
    return L, h, t


def _buffers(t, state, obs, depth=None):
    b = elevation.PgttElevationBuffers()
    b.state, b.obs, b.depth = state.data_ptr(), obs.data_ptr(), None if depth is None else depth.data_ptr()
    b.map, b.origin, b.est, b.known, b.obs_out = (t[k].data_ptr() for k in ("map", "origin", "est", "known", "obs"))
    return b


def test_order_refusals_and_both_sources_on_one_handle():
    camera, ticks = recorded(16, 12)
    S, img, obs = ticks[0]
    pts = recorded_points(96)[0][1]
    dev = "cuda:0"
    state, image, obs_d, points = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (S, img, obs, pts))
    stream = torch.cuda.current_stream().cuda_stream
    L, h, t = _raw_handle(camera, 3)
    # before any bind; after the image's bind: the points entry is refused
    assert L.pgtt_elevation_points(h, None, 1, 0, stream) == -2 and L.pgtt_elevation_last_error()
    assert L.pgtt_elevation_bind(h, C.byref(_buffers(t, state, obs_d, image))) == 0
    assert L.pgtt_elevation_points(h, None, 1, 0, stream) == -2
    # bind_points: points and P are required, the other buffers as for bind
    assert L.pgtt_elevation_bind_points(h, C.byref(_buffers(t, state, obs_d)), None, 96) == -1
    assert L.pgtt_elevation_bind_points(h, C.byref(_buffers(t, state, obs_d)), points.data_ptr(), 0) == -1
    b = _buffers(t, state, obs_d)
    b.map = None
    assert L.pgtt_elevation_bind_points(h, C.byref(b), points.data_ptr(), 96) == -1
    b = _buffers(t, state, obs_d)
    b.obs = None
    assert L.pgtt_elevation_bind_points(h, C.byref(b), points.data_ptr(), 96) == -1              # obs_out without obs
    torch.cuda.synchronize()
    assert (t["est"] == -7.0).all() and (t["obs"] == -7.0).all()                               # nothing was launched so far
    # bound without an image: the image entry is refused, the points entry runs
    assert L.pgtt_elevation_bind_points(h, C.byref(_buffers(t, state, obs_d)), points.data_ptr(), 96) == 0
    assert L.pgtt_elevation(h, None, 1, 0, stream) == -2 and L.pgtt_elevation_last_error()
    torch.cuda.synchronize()
    assert (t["est"] == -7.0).all()
    assert L.pgtt_elevation_points(h, None, 1, 0, stream) == 0
    torch.cuda.synchronize()
    assert (t["est"] != -7.0).all() and (~torch.isnan(t["map"])).sum() > 20
    from_points = {k: v.clone() for k, v in t.items()}
    # bound with both: pgtt_elevation() is what it is on a handle bound the old way, and the points entry what it was
    assert L.pgtt_elevation_bind_points(h, C.byref(_buffers(t, state, obs_d, image)), points.data_ptr(), 96) == 0
    assert L.pgtt_elevation(h, None, 1, 0, stream) == 0
    L2, h2, t2 = _raw_handle(camera, 3)
    assert L2.pgtt_elevation_bind(h2, C.byref(_buffers(t2, state, obs_d, image))) == 0 and L2.pgtt_elevation(h2, None, 1, 0, stream) == 0
    torch.cuda.synchronize()
    assert (~torch.isnan(t2["map"])).sum() > 20
    for k in t:
        assert np.array_equal(_bits(t[k]), _bits(t2[k])), k
    assert L.pgtt_elevation_points(h, None, 1, 0, stream) == 0
    torch.cuda.synchronize()
    for k in t:
        assert np.array_equal(_bits(t[k]), _bits(from_points[k])), k
    # pgtt_elevation_bind afterwards unbinds the points
    assert L.pgtt_elevation_bind(h, C.byref(_buffers(t, state, obs_d, image))) == 0 and L.pgtt_elevation_points(h, None, 1, 0, stream) == -2
    L.pgtt_elevation_destroy(h); L.pgtt_elevation_destroy(h2)
    with pytest.raises(ValueError, match="LiDAR"):
        elevation.ElevationMap(types.SimpleNamespace(lidar_scanner=None), source="lidar")
    with pytest.raises(ValueError, match="source"):
        elevation.ElevationMap(types.SimpleNamespace(), source="sonar")


# ---------------------------------------------------------------- 6. graph capture
def test_graph_capture():
    """one tick captured on a stream and replayed twice equals two eager ticks bit for bit (one kernel node: no parallel branches)"""
    S, pts, obs = recorded_points(1024)[0]
    settings = dict(grid=64, res=RES, alpha=0.5, self_half=(0.45, 0.25, 0.45))
    a, b = Rig(3, 1024, **settings), Rig(3, 1024, **settings)
    for r in (a, b):
        r.put(S, pts, obs)
        r.map.map.fill_(0.25)                                                     # alpha = 0.5 moves every touched cell at every tick
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.map.tick()
    torch.cuda.current_stream().wait_stream(s)
    b.map.tick()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.map.tick()
    torch.cuda.synchronize()
    for t in range(2):
        before = b.map.map.clone()
        g.replay(); b.map.tick()
        torch.cuda.synchronize()
        for k in OUT:
            assert np.array_equal(_bits(getattr(a.map, k)), _bits(getattr(b.map, k))), (k, t)
        assert not torch.equal(torch.nan_to_num(before), torch.nan_to_num(b.map.map))
    a.close(); b.close()


# ---------------------------------------------------------------- 7. the env
def test_env_integration():
    n, G = 8, 64
    lid = dict(n_az=32, n_el=8)
    a = make_env(n, 5, lidar=lid, elevation=dict(source="lidar"), autoreset=True)
    b = make_env(n, 5, autoreset=True)
    assert b.lidar_scanner is None and b.lidar is None and b.lidar_points is None and b.elevation_map is None
    assert a.depth_camera is None and a.lidar.shape == (n, 256) and a.lidar_points.shape == (n, 256, 3) and a.elevation_map.source == "lidar"
    alone = lidar.LidarScanner(a, **lidar.settings(lid))
    cfg = dict(res=RES, alpha=1.0, self_half=elevation.DEFAULTS["self_half"])
    states, doubtful, tally = [pref.new_state(G) for _ in range(n)], [set() for _ in range(n)], Tally()
    rng = np.random.default_rng(6)
    ended = 0
    for t in range(4):                                                            # the reset, then three steps
        if t > 0:
            if t == 2:                                                            # env 5 on its back: its episode ends in this step
                for env in (a, b):
                    env.buffers["state"][abi.S_QPOS + 3:abi.S_QPOS + 7, 5] = torch.tensor([0.0, 1.0, 0.0, 0.0], device="cuda:0")
            act = torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda()
            oa, ra, da, _ = a.step(act)
            ob, rb, db, _ = b.step(act)
            pairs = [(oa["state"], ob["state"]), (oa["privileged_state"], ob["privileged_state"]), (ra, rb), (da, db)]
        else:
            pairs = []
        torch.cuda.synchronize()
        assert set(a.buffers) == set(b.buffers)
        for x, y in pairs + [(a.buffers[k], b.buffers[k]) for k in a.buffers]:
            assert np.array_equal(_bits(x), _bits(y)), t
        assert np.array_equal(_bits(alone.tick(force=True)), _bits(a.lidar)) and np.array_equal(_bits(alone.points), _bits(a.lidar_points))
        obs = a.buffers["obs_state"].cpu().numpy()
        eo = _bits(a.elevation_obs)
        assert np.array_equal(eo[:, :38], _bits(obs)[:, :38]) and np.array_equal(eo[:, 155:], _bits(obs)[:, 155:])
        assert np.array_equal(eo[:, 38:155], _bits(a.elevation_map.est))
        # est follows the points reference fed with env.lidar_points; an env that was reset, or whose episode just ended, holds this tick's points alone
        got = {k: getattr(a.elevation_map, k).cpu().numpy() for k in OUT}
        S, pts, done = a.buffers["state"].cpu().numpy(), a.lidar_points.cpu().numpy(), a.buffers["done"].cpu().numpy()
        for e in range(n):
            clear = t == 0 or done[e] != 0
            ended += int(t > 0 and done[e] != 0)
            want = pref.tick(states[e], S[:7, e], pts[e], cfg, clear=clear)
            want["obs_in"] = obs[e]
            wc = pref.world_cells(want["origin"], G)
            doubtful[e] = set() if clear else doubtful[e] - {tuple(c) for c in wc[want["touched"]]}
            doubtful[e] &= {tuple(c) for c in wc.reshape(-1, 2)}
            doubtful[e] |= pref.doubtful_cells(want, RES, EPS)
            compare(got, e, want, doubtful[e], tally, G)
            if clear:
                out = np.array([[tuple(wc[i, j]) in doubtful[e] for j in range(G)] for i in range(G)])
                assert np.array_equal(~np.isnan(got["map"][e])[~out], want["touched"][~out]), (t, e)
            states[e] = (want["map"], want["origin"])
    cells, scan = tally.shares()
    print(f"env integration: touched {tally.touched}, left out {tally.touched_out} ({100 * cells:.2f} %), scan left out {tally.scan_out} of {tally.scan} "
          f"({100 * scan:.2f} %), worst error / bar: map {tally.worst_map:.3f}, est {tally.worst_est:.3f}; episodes ended {ended}")
    assert ended >= 1 and tally.touched > 200 and cells <= 0.05 and scan <= 0.05
    assert a.elevation_known.sum() > 0 and (a.elevation_map.est > 0).any()
    # reset(mask) clears the masked envs' maps; set_terrain is forwarded to the scanner and every map forgets
    a.elevation_map.map.fill_(9.0)
    a.reset(5, mask=torch.tensor([1, 0, 0, 1, 0, 0, 0, 0], dtype=torch.uint8))
    torch.cuda.synchronize()
    m = a.elevation_map.map.cpu().numpy()
    for e in range(n):
        assert (m[e] == 9.0).any() != (e in (0, 3)) and np.isnan(m[e]).any() == (e in (0, 3)), e
    before = _bits(a.lidar).copy()
    a.set_terrain(a.terrain[::-1].copy())
    a.lidar_scanner.tick(force=True)
    torch.cuda.synchronize()
    assert torch.isnan(a.elevation_map.map).all() and not np.array_equal(_bits(a.lidar), before)
    alone.close(); a.close(); b.close()
    assert a.lidar_scanner is None and a.elevation_map is None
