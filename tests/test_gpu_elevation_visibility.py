"""pgtt_elevation_visibility on the GPU (include/pgtt_elevation.h, "Visibility clean-up"): the kernel against the fp64 statement of
tests/elevation_visibility_reference.py, the points source, flat ground, a jump of the estimate, the skip rule and a garbage origin, the variance
layer, batch independence and graph capture, degenerate inputs and the env.

The bound of a cell is a minimum over samples, so one sample that a rounding error moves across a cell border, across the end guard or in and out
of the self box changes it by far more than a rounding error.  The reference says which cells that can happen to: it returns the bound over the
samples that are sure and over all that are possible, and a cell is compared where the two agree (the bound), or where both give one verdict and
the height is further than the bar from the threshold (the verdict).  The bar is the project's forward bar, 2e-5 (1 + |z|); at most 5 % of the cells
with a bound may be left out, per case, for either.  Measured shares: test_kernel_against_the_reference's docstring and DESIGN.md 27."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_visibility_reference as vref  # noqa: E402
import odometry_reference as oref  # noqa: E402
from test_elevation_visibility import (CAM, CAP, CASES, JUMP, JUMP_SIZE, Q0, VIS, case_setup, image, jump_scenario, prepare,  # noqa: E402
                                       ref_cfg)
from test_gpu_elevation import EPS, RES, VARIANTS, _bits, make_env, recorded  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, depth as depth_mod, elevation  # noqa: E402

pytestmark = pytest.mark.gpu

ZERO = dict(oref.ZERO)
LIDAR = dict(n_az=32, n_el=8)
OUTS = ("map", "origin", "est", "known", "obs", "cleared", "bound", "var")


class Rig:
    """what ElevationMap reads of an env - state, image or points, observation, done, the sensors' configs, dt and the global id - as tensors the
    test fills, and the map on them"""

    def __init__(self, n, camera, points=None, sensor_pos=(0.0, 0.0, 0.0), **settings):
        dev = torch.device("cuda:0")
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)
        cc = depth_mod.config_struct(camera["width"], camera["height"], camera["fovy"], camera["near"], camera["far"], 0, camera["mount_pos"],
                                     camera["mount_quat"])
        self.env = types.SimpleNamespace(depth=z(n, camera["height"], camera["width"]), depth_camera=types.SimpleNamespace(config=cc),
                                         buffers={"state": z(abi.NSTATE, n), "obs_state": z(n, 171), "done": z(n)}, device=dev, num_envs=n,
                                         observation_size={"state": 171}, config=dict(scan_dist_x=0.1, scan_dist_y=0.1), method="pgtt", dt=0.02,
                                         env_id_offset=0)
        if points is not None:
            self.env.lidar_scanner = types.SimpleNamespace(points=z(n, points, 3), config=types.SimpleNamespace(every=1, mount_body=0, mount_pos=sensor_pos))
            settings["source"] = "lidar"
        self.map = elevation.ElevationMap(self.env, **settings)

    def put(self, state, image=None, points=None):
        self.env.buffers["state"].copy_(torch.from_numpy(np.ascontiguousarray(state)))
        if image is not None:
            self.env.depth.copy_(torch.from_numpy(np.ascontiguousarray(image)))
        if points is not None:
            self.env.lidar_scanner.points.copy_(torch.from_numpy(np.ascontiguousarray(points)))

    def out(self):
        torch.cuda.synchronize()
        return {k: getattr(self.map, k).cpu().numpy().copy() for k in OUTS if hasattr(self.map, k)}

    def close(self):
        self.map.close()


def state_of(qpos, n):
    S = np.zeros((abi.NSTATE, n), np.float32)
    S[:7] = np.asarray(qpos, np.float32).reshape(7, -1)
    return S


def hold(got, before, e, want, tally=None):
    """one env of one clean-up against the reference's `want`: the bound where it is decided, the verdict where it is decided, the bits of what was
    kept, the count"""
    b = got["bound"][e].astype(float)
    dec = want["bound_decided"]
    assert np.array_equal(np.isnan(b)[dec], np.isnan(want["bound_sure"])[dec]), "bound: NaN pattern"
    cmp = dec & ~np.isnan(want["bound_sure"])
    worst = 0.0
    if cmp.any():
        ratio = np.abs(b[cmp] - want["bound_sure"][cmp]) / (EPS * (1 + np.abs(want["bound_sure"][cmp])))
        worst = float(ratio.max())
        assert worst <= 1, ("bound", worst)
    # an undecided bound lies between the two the reference gives
    und = ~dec & ~np.isnan(b)
    assert (b[und] >= want["bound_any"][und] - EPS * (1 + np.abs(b[und]))).all()
    gone = np.isnan(got["map"][e]) & ~np.isnan(before[e])
    vd = want["verdict_decided"]
    assert np.array_equal(gone[vd], want["clear_sure"][vd]), "verdict"
    assert np.array_equal(_bits(got["map"][e])[~gone], _bits(before[e])[~gone]), "a kept cell changed"
    assert int(got["cleared"][e]) == int(gone.sum()), "cleared"
    if tally is not None:
        tally["n"] += int(want["has_bound"].sum())
        tally["bound"] += int((want["has_bound"] & ~dec).sum())
        tally["verdict"] += int((want["has_bound"] & ~vd).sum())
        tally["cleared"] += int(gone.sum())
        tally["worst"] = max(tally["worst"], worst)


def new_tally():
    return dict(n=0, bound=0, verdict=0, cleared=0, worst=0.0)


def ticked_and_prepared(rig, seed0=100):
    """one real tick (clear_all: the clean-up in front of it skips every env), then the host's preparation of the map -> the prepared maps [N, G, G]"""
    rig.map.tick(clear_all=True)
    torch.cuda.synchronize()
    assert (rig.map.cleared == 0).all()
    if hasattr(rig.map, "bound"):
        assert torch.isnan(rig.map.bound).all()
    m = rig.map.map.cpu().numpy()
    before = np.stack([prepare(m[e], seed0 + e) for e in range(m.shape[0])])
    rig.map.map.copy_(torch.from_numpy(before))
    return before


# ---------------------------------------------------------------- 1. the kernel against the reference
@pytest.mark.parametrize("width,height,G,stride", CASES)
def test_kernel_against_the_reference(width, height, G, stride):
    """Undecided on an MI355X, per case (three envs pooled; stride 1 / stride 3), against the cap of 5 % each:

        image   G    cells with a bound   bound undecided              verdict undecided   cleared
        16x12   8        190 / 143        0 / 0                        0 / 0               20 / 15
        16x12   9        238 / 172        0 / 0                        0 / 0               21 / 15
        16x12  24        695 / 383        2 (0.29 %) / 0               0 / 0               50 / 26
        16x12  64       1318 / 555        4 (0.30 %) / 0               0 / 0               84 / 38
        48x32   8        191 / 189        4 (2.09 %) / 0               0 / 0               21 / 21
        48x32   9        241 / 238        4 (1.66 %) / 0               0 / 0               25 / 25
        48x32  24        806 / 741        4 (0.50 %) / 2 (0.27 %)      0 / 0               74 / 70
        48x32  64       1798 / 1434       18 (1.00 %) / 11 (0.77 %)    0 / 0              167 / 135

    The worst error of a decided bound is 0.006 of the bar.  The reference alone, on the CPU (tests/test_elevation_visibility.py): 0.00 - 3.31 % of
    the bounds, 0.00 - 0.12 % of the verdicts."""
    camera, ticks = recorded(width, height)
    camera, settings = case_setup(camera, G)
    vis = dict(VIS, stride=stride)
    rig = Rig(3, camera, **settings, visibility=vis, dense_bound=True)
    S, img, _ = ticks[0]
    rig.put(S, img)
    before = ticked_and_prepared(rig)
    rig.map.clean()
    got = rig.out()
    cfg, tally = ref_cfg(camera, settings), new_tally()
    for e in range(3):
        want = vref.visibility((before[e], got["origin"][e]), S[:7, e].astype(float), cfg, vis, depth=img[e], eps=EPS)
        hold(got, before, e, want, tally)
    rig.close()
    sb, sv = tally["bound"] / max(tally["n"], 1), tally["verdict"] / max(tally["n"], 1)
    print(f"{width}x{height} G={G} stride={stride}: {tally['n']} cells with a bound, undecided bound {tally['bound']} ({100 * sb:.2f} %), undecided verdict "
          f"{tally['verdict']} ({100 * sv:.2f} %), cleared {tally['cleared']}, worst bound error / bar {tally['worst']:.3f}")
    assert tally["n"] >= 20 and tally["cleared"] >= 1, "the case would be vacuous"
    assert sb <= CAP and sv <= CAP


# ---------------------------------------------------------------- 2. the points source
def test_points_source_with_the_lidar():
    env = make_env(3, 11, variant=VARIANTS, lidar=LIDAR)
    rng = np.random.default_rng(5)
    for _ in range(6):
        env.step(torch.from_numpy(np.tanh(rng.normal(size=(3, 12)) * 0.4).astype(np.float32)).cuda())
    G, vis = 64, dict(VIS, stride=1)
    mount = tuple(env.lidar_scanner.config.mount_pos)
    em = elevation.ElevationMap(env, grid=G, res=RES, source="lidar", visibility=vis, dense_bound=True)
    rig = types.SimpleNamespace(map=em)
    before = ticked_and_prepared(rig)
    em.clean()
    got = Rig.out(rig)
    S, pts = env.buffers["state"].cpu().numpy(), env.lidar_scanner.points.cpu().numpy()
    cfg = dict(fovy=90.0, near=0.1, far=1.0, mount_pos=(0, 0, 0), mount_quat=(1, 0, 0, 0), res=RES, alpha=1.0, self_half=elevation.DEFAULTS["self_half"])
    tally = new_tally()
    for e in range(3):
        want = vref.visibility((before[e], got["origin"][e]), S[:7, e].astype(float), cfg, dict(vis, sensor_pos=mount), points=pts[e], eps=EPS)
        hold(got, before, e, want, tally)
    sb, sv = tally["bound"] / max(tally["n"], 1), tally["verdict"] / max(tally["n"], 1)
    print(f"LiDAR 32x8 G={G}: {tally['n']} cells with a bound, undecided bound {tally['bound']} ({100 * sb:.2f} %), undecided verdict {tally['verdict']} "
          f"({100 * sv:.2f} %), cleared {tally['cleared']}, worst bound error / bar {tally['worst']:.3f}")
    assert tally["n"] >= 20 and tally["cleared"] >= 1 and sb <= CAP and sv <= CAP
    # the points in another order: the same bits
    perm = torch.from_numpy(np.random.default_rng(2).permutation(pts.shape[1])).cuda()
    env.lidar_scanner.points.copy_(env.lidar_scanner.points[:, perm].clone())
    em.map.copy_(torch.from_numpy(before))
    em.clean()
    again = Rig.out(rig)
    for k in ("map", "bound", "cleared"):
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k
    em.close(); env.close()


# ---------------------------------------------------------------- 3. flat ground, exact pose
def test_flat_ground_clears_nothing_and_moves_no_bit():
    camera = dict(CAM, width=48, height=32)
    settings = dict(grid=64, res=RES, alpha=1.0, self_half=(0.45, 0.25, 0.45))
    a, b = Rig(2, camera, **settings, visibility=True), Rig(2, camera, **settings)
    assert a.map.visibility["stride"] == elevation.VISIBILITY_DEFAULTS["stride"] and not hasattr(b.map, "cleared") and b.map.visibility is None
    for t in range(5):
        qs = [Q0 + np.array([0.03 * t, 0.011 * t * (-1) ** e, 0, 0, 0, 0, 0]) for e in range(2)]
        S = state_of(np.stack(qs, 1), 2)
        img = np.stack([image(S[:7, e].astype(float), camera, w=48, h=32) for e in range(2)])
        for r in (a, b):
            r.put(S, img)
            r.map.tick(clear_all=t == 0)
        ga, gb = a.out(), b.out()
        assert (ga["cleared"] == 0).all(), t
        for k in ("map", "origin", "est", "known", "obs"):
            assert np.array_equal(_bits(ga[k]), _bits(gb[k])), (k, t)
    assert (~np.isnan(ga["map"])).sum() > 200
    a.close(); b.close()


# ---------------------------------------------------------------- 4. a jump of the estimate
def test_a_jump_of_the_estimate_clears_the_old_risers():
    q, img, cfg, G = jump_scenario()
    camera = dict(width=JUMP_SIZE[0], height=JUMP_SIZE[1], fovy=cfg["fovy"], near=cfg["near"], far=cfg["far"], mount_pos=cfg["mount_pos"], mount_quat=cfg["mount_quat"])
    vis = dict(VIS, stride=1)
    rig = Rig(2, camera, grid=G, res=RES, alpha=1.0, self_half=cfg["self_half"], odometry=ZERO, visibility=vis, dense_bound=True)
    rig.put(state_of(np.stack([q, q], 1), 2), np.stack([img, img]))
    rig.map.tick(clear_all=True)
    before = rig.out()
    assert np.array_equal(before["cleared"], [0, 0])
    rig.map.odo[0, 0] = float(JUMP)                                              # env 0's estimate jumps three cells ahead; env 1 keeps the truth
    stream = torch.cuda.current_stream().cuda_stream
    elevation.check(rig.map._lib.pgtt_elevation_odometry(rig.map._h, None, 0, 0, stream))
    rig.map.clean()
    got = rig.out()
    pose = rig.map.pose_est.cpu().numpy().astype(float)
    assert pose[0, 0] == float(np.float32(q[0]) + JUMP) and pose[0, 1] == q[0]
    decided = []
    for e in range(2):
        want = vref.visibility((before["map"][e], before["origin"][e]), pose[:, e], cfg, vis, depth=img, eps=EPS)
        hold(got, before["map"], e, want)
        decided.append(int((want["clear_sure"] & want["verdict_decided"]).sum()))
    print(f"jump of three cells: cleared {got['cleared'].tolist()}, of them by a decided verdict of the reference {decided}")
    assert decided[0] >= 1 and got["cleared"][0] >= decided[0] and got["cleared"][0] > got["cleared"][1]
    assert got["cleared"].sum() > 0
    rig.close()


# ---------------------------------------------------------------- 5. the skip rule, a garbage origin
def test_skip_rule_and_garbage_origin():
    camera, ticks = recorded(16, 12)
    G = 24
    camera, settings = case_setup(camera, G)
    rig = Rig(3, camera, **settings, visibility=dict(VIS, stride=1), dense_bound=True)
    S, img, _ = ticks[0]
    rig.put(S, img)
    rig.map.tick(clear_all=True)
    for kw, done, skipped in ((dict(clear_all=True), (0, 0, 0), (1, 1, 1)), (dict(clear_mask=torch.tensor([0, 1, 0], dtype=torch.uint8)), (0, 0, 0), (0, 1, 0)),
                              (dict(use_done=True), (1, 0, 1), (1, 0, 1)), (dict(use_done=False), (1, 1, 1), (0, 0, 0))):
        rig.map.map.fill_(5.0)                                                   # five metres: every cell under a ray is contradicted
        rig.map.cleared.fill_(-7)
        rig.env.buffers["done"].copy_(torch.tensor(done, dtype=torch.float32))
        rig.map.clean(**kw)
        got = rig.out()
        for e in range(3):
            if skipped[e]:
                assert (got["map"][e] == 5.0).all() and got["cleared"][e] == 0 and np.isnan(got["bound"][e]).all(), (kw, e)
            else:
                assert got["cleared"][e] > 10 and got["cleared"][e] == np.isnan(got["map"][e]).sum() == (~np.isnan(got["bound"][e])).sum(), (kw, e)
    rig.close()
    # a handle never ticked, garbage in `origin`, the map and the bound inside guard rows
    for G in (9, 24):
        rig = Rig(3, camera, **dict(settings, grid=G), visibility=dict(VIS, stride=1), dense_bound=True)
        big_m = torch.full((5, G, G), 7.0, device="cuda:0")
        big_b = torch.full((5, G, G), 7.0, device="cuda:0")
        big_m[1:4] = 5.0
        rig.map.map, rig.map.bound = big_m[1:4], big_b[1:4]
        lo, hi = -2 ** 31, 2 ** 31 - 1
        rig.map.origin.copy_(torch.tensor([[lo, hi], [hi, lo], [hi, 12]], dtype=torch.int32))
        rig.map.bind()
        rig.put(S, img)
        rig.map.clean()
        torch.cuda.synchronize()
        assert (big_m[0] == 7.0).all() and (big_m[4] == 7.0).all() and (big_b[0] == 7.0).all() and (big_b[4] == 7.0).all()
        assert (big_m[1:4] == 5.0).all() and torch.isnan(big_b[1:4]).all() and (rig.map.cleared == 0).all()      # a window a world away holds no sample
        assert np.array_equal(rig.map.origin.cpu().numpy(), [[lo, hi], [hi, lo], [hi, 12]])                     # origin is not written
        rig.close()


# ---------------------------------------------------------------- 6. the variance layer
def test_variance_layer():
    camera, ticks = recorded(48, 32)
    G = 64
    settings = dict(grid=G, res=RES, alpha=1.0, self_half=(0.45, 0.25, 0.45))
    rig = Rig(3, camera, **settings, variance=True, visibility=dict(VIS, stride=1, sigmas=3.0), dense_bound=True)
    S, img, _ = ticks[0]
    rig.put(S, img)
    rig.map.tick(clear_all=True)
    clean = rig.out()
    assert np.array_equal(np.isnan(clean["map"]), np.isnan(clean["var"]))
    # a first clean-up on the map as ticked gives the bound layer; then one crafted cell per env: h above bound + margin, h - 3 sqrt(v) below it
    rig.map.clean()
    first = rig.out()
    slots = []
    for e in range(3):
        ok = np.argwhere(~np.isnan(first["bound"][e]) & ~np.isnan(first["map"][e]))
        i, j = ok[len(ok) // 2]
        slots.append((e, i, j))
        rig.map.map[e, i, j] = float(first["bound"][e, i, j]) + VIS["margin"] + 0.02
        rig.map.var[e, i, j] = 0.02 ** 2
    kept = rig.map.map.clone()
    rig.map.clean()
    got = rig.out()
    for e, i, j in slots:
        assert not np.isnan(got["map"][e, i, j]) and got["var"][e, i, j] == np.float32(0.02 ** 2)        # 3 sigma = 0.06 m: not contradicted
    rig.map.visibility["sigmas"] = 0.0
    rig.map.bind()
    rig.map.map.copy_(kept)
    rig.map.clean()
    got = rig.out()
    for e, i, j in slots:
        assert np.isnan(got["map"][e, i, j]) and np.isnan(got["var"][e, i, j])
    # raised cells: var goes with map
    before = np.stack([prepare(clean["map"][e], 100 + e) for e in range(3)])
    rig.map.map.copy_(torch.from_numpy(before))
    rig.map.var.copy_(torch.from_numpy(np.where(np.isnan(before), np.nan, 1e-4).astype(np.float32)))
    rig.map.clean()
    got = rig.out()
    assert got["cleared"].sum() > 20 and np.array_equal(np.isnan(got["map"]), np.isnan(got["var"]))
    assert np.array_equal(got["cleared"], (np.isnan(got["map"]) & ~np.isnan(before)).sum((1, 2)))
    rig.close()


# ---------------------------------------------------------------- 7. batch independence, determinism, graph capture
def _one_clean(n, camera, settings, S, img, cols):
    rig = Rig(n, camera, **settings, visibility=dict(VIS, stride=1), dense_bound=True)
    rig.put(S[:, cols], img[cols])
    rig.map.tick(clear_all=True)
    torch.cuda.synchronize()
    m = rig.map.map.cpu().numpy()
    rig.map.map.copy_(torch.from_numpy(np.stack([prepare(m[i], 100 + c) for i, c in enumerate(cols)])))
    rig.map.clean()
    got = rig.out()
    rig.close()
    return got


def test_batch_independence_and_determinism():
    camera, ticks = recorded(48, 32)
    camera, settings = case_setup(camera, 24)                                    # the camera 0.5 m back: its rays cross the window of 24 cells
    S, img, _ = ticks[0]
    three, again = _one_clean(3, camera, settings, S, img, [0, 1, 2]), _one_clean(3, camera, settings, S, img, [0, 1, 2])
    big = _one_clean(65, camera, settings, S, img, [0] + [1] * 63 + [2])
    for k in three:
        assert np.array_equal(_bits(three[k]), _bits(again[k])), k
    assert three["cleared"].sum() > 10
    for e, pos in ((0, 0), (2, 64)):
        alone = _one_clean(1, camera, settings, S, img, [e])
        for k in three:
            assert np.array_equal(_bits(three[k][e]), _bits(alone[k][0])), (k, e)
            assert np.array_equal(_bits(three[k][e]), _bits(big[k][pos])), (k, e)


def test_graph_capture():
    """odometry + clean-up + tick captured on a stream and replayed three times equals three eager sequences, bit for bit"""
    camera, ticks = recorded(48, 32)
    settings = dict(grid=64, res=RES, alpha=0.5, self_half=(0.45, 0.25, 0.45))
    S, img, _ = ticks[0]
    a, b = (Rig(3, camera, **settings, odometry=ZERO, visibility=dict(VIS, stride=1), dense_bound=True) for _ in range(2))
    for r in (a, b):
        r.put(S, img)
        r.map.tick(clear_all=True)
    torch.cuda.synchronize()
    start = np.stack([prepare(m, 100 + e) for e, m in enumerate(a.map.map.cpu().numpy())])
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
    for r in (a, b):
        r.map.map.copy_(torch.from_numpy(start))
    for t in range(3):
        g.replay(); b.map.tick()
        ga, gb = a.out(), b.out()
        for k in ga:
            assert np.array_equal(_bits(ga[k]), _bits(gb[k])), (k, t)
        if t == 0:
            assert ga["cleared"].sum() > 10
    a.close(); b.close()


# ---------------------------------------------------------------- 8. degenerate inputs
def test_degenerate_inputs():
    camera, ticks = recorded(16, 12)
    G = 24
    camera, settings = case_setup(camera, G)
    S, img, _ = ticks[0]
    cfg = ref_cfg(camera, settings)
    for stride in (1, 1000):                                                     # a stride larger than the image: pixel (0, 0) alone casts a ray
        vis = dict(VIS, stride=stride)
        rig = Rig(3, camera, **settings, visibility=vis, dense_bound=True)
        bad = img.copy()
        bad[0] = np.nan
        bad[1] = camera["far"]
        bad[2].reshape(-1)[1::5] = np.nan
        bad[2].reshape(-1)[2::7] = np.inf
        bad[2].reshape(-1)[3::11] = -np.inf
        rig.put(S, bad)
        rig.map.map.fill_(5.0)
        rig.map.origin.copy_(torch.from_numpy(np.floor(S[:2].T.astype(float) / float(np.float32(RES))).astype(np.int32)))
        before = rig.map.map.cpu().numpy()
        rig.map.clean()
        got = rig.out()
        assert (got["cleared"][:2] == 0).all() and np.isnan(got["bound"][:2]).all() and (got["map"][:2] == 5.0).all()
        want = vref.visibility((before[2], got["origin"][2]), S[:7, 2].astype(float), cfg, vis, depth=bad[2], eps=EPS)
        hold(got, before, 2, want)
        assert not np.isinf(got["bound"]).any() and (stride > 1 or got["cleared"][2] > 5)
        rig.close()
    # a camera mounted straight down: Lh is about 0 at the image's centre and below the first sample around it
    import depth_reference as dref
    down = dict(CAM, width=5, height=5, mount_quat=tuple(dref.pitch_quat(90.0).astype(np.float32).astype(float)))
    vis = dict(VIS, stride=1, end_guard=0.0)
    rig = Rig(1, down, grid=G, res=RES, self_half=(0, 0, 0), visibility=vis, dense_bound=True)
    S1 = state_of(Q0, 1)
    dimg = image(Q0, down, w=5, h=5)[None]
    rig.put(S1, dimg)
    rig.map.map.fill_(5.0)
    rig.map.origin.copy_(torch.from_numpy(np.floor(S1[:2].T.astype(float) / float(np.float32(RES))).astype(np.int32)))
    before = rig.map.map.cpu().numpy()
    rig.map.clean()
    got = rig.out()
    want = vref.visibility((before[0], got["origin"][0]), S1[:7, 0].astype(float), down, vis, depth=dimg[0], eps=EPS)
    hold(got, before, 0, want)
    assert np.isfinite(got["bound"][~np.isnan(got["bound"])]).all()
    rig.close()
    # points with NaN, inf and 1e30
    P = 40
    rig = Rig(1, down, points=P, sensor_pos=(0.1, 0.0, 0.05), grid=G, res=RES, self_half=(0, 0, 0), visibility=dict(VIS, stride=1), dense_bound=True)
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.uniform(-0.6, 0.6, (P, 2)), np.zeros((P, 1))], 1).astype(np.float32)
    pts[0] = np.nan; pts[1, 1] = np.inf; pts[2, 0] = -np.inf; pts[3] = (1e30, 0.0, 0.0); pts[4] = (1e30, -1e30, 1e30); pts[5, 2] = np.nan
    rig.put(S1, points=pts[None])
    rig.map.map.fill_(5.0)
    rig.map.origin.copy_(torch.from_numpy(np.floor(S1[:2].T.astype(float) / float(np.float32(RES))).astype(np.int32)))
    before = rig.map.map.cpu().numpy()
    rig.map.clean()
    got = rig.out()
    want = vref.visibility((before[0], got["origin"][0]), S1[:7, 0].astype(float), down, dict(VIS, stride=1, sensor_pos=(0.1, 0.0, 0.05)), points=pts, eps=EPS)
    hold(got, before, 0, want)
    assert got["cleared"][0] > 5 and not np.isinf(got["bound"]).any()
    rig.close()


# ---------------------------------------------------------------- 9. the env
@pytest.mark.parametrize("source", ["depth", "lidar"])
def test_env_integration(source):
    sensors = dict(lidar=LIDAR) if source == "lidar" else dict(depth=dict(width=48, height=32))
    base = dict(grid=24) if source == "depth" else dict(grid=24, source="lidar")
    n = 8
    a = make_env(n, 5, **sensors, elevation=dict(base, visibility=True, odometry=dict(sigma_xy=0.2, sigma_yaw=0.1)), autoreset=True)
    b = make_env(n, 5, **sensors, autoreset=True)
    assert b.elevation_cleared is None and a.elevation_cleared.shape == (n,) and a.elevation_cleared.dtype == torch.int32
    assert a.elevation_cleared.data_ptr() == a.elevation_map.cleared.data_ptr()                    # a view
    assert a.elevation_map.visibility == dict(margin=0.05, end_guard=1.5 * 0.04, stride=elevation.VISIBILITY_DEFAULTS["stride"], sigmas=0.0)
    rng = np.random.default_rng(6)
    total = 0
    for t in range(8):
        act = torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda()
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        torch.cuda.synchronize()
        pairs = [(oa["state"], ob["state"]), (oa["privileged_state"], ob["privileged_state"]), (ra, rb), (da, db), (a.buffers["state"], b.buffers["state"])]
        pairs.append((a.depth, b.depth) if source == "depth" else (a.lidar_scanner.points, b.lidar_scanner.points))
        for x, y in pairs:
            assert np.array_equal(_bits(x), _bits(y)), t
        c = a.elevation_cleared.cpu().numpy()
        assert (c >= 0).all() and (c <= 24 * 24).all()
        total += int(c.sum())
    print(f"env, {source}: {total} cells forgotten in 8 steps of {n} envs under ten times the default drift")
    assert np.isfinite(a.elevation_map.est.cpu().numpy()).all()
    a.close(); b.close()


def test_evaluate_gains_one_key_and_one_line(capsys):
    import evaluate
    base = ["--policy", "policy177", "--terrain_file", "level4", "--elevation"]
    run = lambda *extra: evaluate.run_evaluation(evaluate.make_parser().parse_args(base + list(extra)), num_eval_envs=32, verbose=True)
    plain = run()
    said = capsys.readouterr().out.strip().splitlines()
    assert "visibility_cleared_per_step" not in plain and len(said) == 2 and not any("visibility" in s for s in said)
    vis = run("--elevation_visibility")
    said = capsys.readouterr().out.strip().splitlines()
    assert set(vis) - set(plain) == {"visibility_cleared_per_step"} and set(plain) <= set(vis)
    assert len(said) == 3 and said[2].startswith("visibility clean-up:") and said[:2] == [str(vis["episode_reward"]), str([vis["survivors"]])]
    assert 0 <= vis["visibility_cleared_per_step"] <= 64 * 64
