"""pgtt_elevation_follow on the GPU: the map behind a sensor of any period (include/pgtt_elevation.h, "Following a slower sensor").

A fresh call is held to pgtt_elevation() / pgtt_elevation_points() on a twin handle, bit for bit: it is the same kernel behind a gate.  A hold call
computes nothing but `est`, one fp32 subtraction of two of the map's values, so it is held bit for bit to tests/elevation_follow_reference.hold on
the device's OWN map; what the device computes in fp32 is which cell a scan point falls into (a three-term sum of magnitude <= 20 m and one
division: a few ulp(20) ~ 1e-5 m), and the poses (test_elevation_follow.poses, whose margin is asserted there without a GPU) keep every scan point
1e-4 m from a cell border, so no point is left out of any comparison.  The rig's counter is the SENSOR's: the test writes c + 1 into it, what the
sensor's own call leaves behind, except where a real camera or LiDAR ticks in front of the map (the schedule, the captured step, the env).
Every output of the rig's map sits between guard bands of sentinels."""
import ctypes as C
import os
import sys
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_fill_reference as fref  # noqa: E402
import elevation_follow_reference as fol  # noqa: E402
import elevation_reference as ref  # noqa: E402
from test_elevation_follow import BASE_CELLS, MARGIN, MOVES, RES32, poses  # noqa: E402
from test_gpu_elevation import RES, _bits, case_setup, make_env, recorded  # noqa: E402
from test_gpu_elevation_fill import same_floats  # noqa: E402
from test_gpu_learn_kernels import Guarded  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, depth as depth_mod, elevation  # noqa: E402

pytestmark = pytest.mark.gpu

OUT = ("map", "origin", "est", "known", "obs")
GRIDS = (8, 9, 24, 64)
NPTS = 64
E_ARG, E_STATE = -1, -2
CFG = dict(res=RES, scan_dist_x=0.1, scan_dist_y=0.1)


class FollowRig:
    """what ElevationMap reads of an env - state, image or points, observation, done, the sensor's config and COUNTER - as tensors the test fills,
    and the map on them with its outputs between guard bands.  map_front = 20 floats keeps the map's rows on 16-byte boundaries (the 16-byte runs of
    an even G), 19 does not (the dword path)."""

    def __init__(self, n, camera, every=1, follow=True, points=False, map_front=20, obs_dim=171, **settings):
        dev = torch.device("cuda:0")
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)
        cc = depth_mod.config_struct(camera["width"], camera["height"], camera["fovy"], camera["near"], camera["far"], 0, camera["mount_pos"],
                                     camera["mount_quat"], every=every if follow else 1)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.env = types.SimpleNamespace(depth=z(n, camera["height"], camera["width"]), depth_camera=types.SimpleNamespace(config=cc, counter=self.counter),
                                         buffers={"state": z(abi.NSTATE, n), "obs_state": z(n, obs_dim), "done": z(n)}, device=dev, num_envs=n,
                                         observation_size={"state": obs_dim}, config=dict(scan_dist_x=0.1, scan_dist_y=0.1), method="pgtt")
        self.points = points
        if points:
            self.env.lidar_scanner = types.SimpleNamespace(points=torch.full((n, NPTS, 3), float("nan"), device=dev), counter=self.counter,
                                                           config=types.SimpleNamespace(every=every if follow else 1))
            settings = dict(settings, source="lidar")
        self.map = m = elevation.ElevationMap(self.env, follow_sensor=follow, **settings)
        G = m.grid
        self.guards = dict(map=Guarded(n, G, G, front=map_front), origin=Guarded(n, 2, dtype=torch.int32, fill=-77777), est=Guarded(n, 117),
                           known=Guarded(n, 117, dtype=torch.uint8, fill=201, front=21, back=17), obs=Guarded(n, obs_dim, front=17))
        for k, g in self.guards.items():
            setattr(m, k, g.view)
        m.map.fill_(float("nan")); m.origin.zero_(); m.est.zero_(); m.known.zero_(); m.obs.zero_()
        m.bind()

    def put(self, state=None, data=None, obs=None, qpos=None):
        if state is not None:
            self.env.buffers["state"].copy_(torch.from_numpy(np.ascontiguousarray(state, np.float32)))
        if qpos is not None:                                                  # [n, 7]: the base rows alone
            self.env.buffers["state"][:7] = torch.from_numpy(np.ascontiguousarray(np.asarray(qpos, np.float32).T)).cuda()
        if data is not None:
            (self.env.lidar_scanner.points if self.points else self.env.depth).copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32)))
        if obs is not None:
            self.env.buffers["obs_state"].copy_(torch.from_numpy(np.ascontiguousarray(obs)))

    def call(self, c=0, force=False, **kw):
        """one call of the map behind a sensor call that found its counter at c"""
        self.counter.fill_(c + 1)
        self.map.tick(force=force, **kw)
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        return {k: getattr(self.map, k).cpu().numpy().copy() for k in OUT}

    def intact(self):
        return all(g.guards_intact() for g in self.guards.values())

    def close(self):
        assert self.intact()
        self.map.close()


def same(a, b, keys=OUT, rows=None, msg=None):
    for k in keys:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(_bits(x), _bits(y)), (k, msg)


def setup(G, alpha=0.5):
    camera, ticks = recorded(16, 12)
    camera, settings = case_setup(camera, G, alpha)
    return camera, settings, ticks


def cloud(rng, qpos, G):
    """NPTS world points around each base, some rows without a return -> [n, NPTS, 3] fp32"""
    n = len(qpos)
    p = np.concatenate([qpos[:, None, :2] + rng.uniform(-0.6, 0.6, (n, NPTS, 2)) * min(1.0, G * RES / 1.0), rng.normal(size=(n, NPTS, 1)) * 0.2], -1)
    p[:, ::7] = np.nan
    return p.astype(np.float32)


def crafted(rng, n, G, share=0.6):
    """[n, G, G] fp32 maps of ordinary values that know `share` of their cells"""
    m = rng.normal(size=(n, G, G)).astype(np.float32)
    m[rng.random((n, G, G)) >= share] = np.nan
    return m


def state_of(qpos, n=None):
    S = np.zeros((abi.NSTATE, len(qpos)), np.float32)
    S[:7] = np.asarray(qpos, np.float32).T
    return S


@lru_cache(maxsize=None)
def observations(n=3):
    return np.random.default_rng(77).normal(size=(n, 171)).astype(np.float32)


# ---------------------------------------------------------------- 1. every = 1 is the tick
@pytest.mark.parametrize("G", GRIDS)
def test_every_1_is_the_tick(G):
    camera, settings, ticks = setup(G)
    a, b = FollowRig(3, camera, every=1, **settings), FollowRig(3, camera, follow=False, **settings)
    for t, (S, img, obs) in enumerate(ticks):                                 # the base moves between the ticks: inside its cell, by 5, by 97 cells
        a.put(S, img, obs); b.put(S, img, obs)
        ga, gb = a.call(c=t, clear_all=t == 0), b.call(c=t, clear_all=t == 0)
        same(ga, gb, msg=t)
    assert (~np.isnan(ga["map"])).sum() > 5 and a.map.follow_sensor and not b.map.follow_sensor
    a.close(); b.close()


@pytest.mark.parametrize("G", GRIDS)
def test_every_1_is_the_points_tick(G):
    camera, settings, _ = setup(G, alpha=0.5)
    rng = np.random.default_rng(G)
    a, b = FollowRig(3, camera, every=1, points=True, **settings), FollowRig(3, camera, follow=False, points=True, **settings)
    p = poses()
    for t, name in enumerate(("base", "same", "five")):
        pts = cloud(rng, p[name], G)
        for r in (a, b):
            r.put(state_of(p[name]), pts, observations())
        ga, gb = a.call(c=t, clear_all=t == 0), b.call(c=t, clear_all=t == 0)
        same(ga, gb, msg=t)
    assert (~np.isnan(ga["map"])).sum() > 5 and a.map.alpha == 0.5
    a.close(); b.close()


# ---------------------------------------------------------------- 2. a hold behind a fresh call at the same pose
@pytest.mark.parametrize("G,front", [(g, 20) for g in GRIDS] + [(24, 19)])
def test_a_hold_at_the_same_pose(G, front):
    camera, settings, ticks = setup(G)
    rig = FollowRig(3, camera, every=3, map_front=front, **settings)
    rig.put(state_of(poses()["base"]), ticks[0][1], observations())
    fresh = rig.call(c=0, clear_all=True)
    rig.map.est.fill_(-3.0); rig.map.known.fill_(7); rig.map.obs.fill_(-5.0)
    held = rig.call(c=1)
    same(fresh, held)
    assert np.array_equal(fresh["origin"], BASE_CELLS)
    if G >= 24:
        assert fresh["known"].sum() > 10 and (fresh["est"] > 0).any()
    rig.close()


# ---------------------------------------------------------------- 3. holds with the base moved
@pytest.mark.parametrize("G,front", [(g, 20) for g in GRIDS] + [(24, 19)])
def test_holds_with_the_base_moved(G, front):
    camera, settings, ticks = setup(G)
    rig = FollowRig(3, camera, every=5, map_front=front, **settings)
    p = poses()
    rig.put(state_of(p["base"]), ticks[0][1], observations())
    rig.call(c=0, clear_all=True)                                             # the origins are the device's own
    rig.map.map.copy_(torch.from_numpy(crafted(np.random.default_rng(G), 3, G)))
    before = rig.read()
    known = 0
    for c, name in enumerate(("same", "one", "five", "far"), start=1):
        rig.put(qpos=p[name])
        got = rig.call(c=c)
        same(before, got, keys=("map", "origin"), msg=name)
        for e in range(3):
            want = fol.hold((got["map"][e], got["origin"][e]), p[name][e], CFG, obs=observations()[e])
            assert want["scan"]["margin"].min() >= MARGIN
            assert np.array_equal(got["known"][e] != 0, want["known"]), (name, e)
            assert np.array_equal(_bits(got["est"][e]), _bits(want["est"])), (name, e)
            assert np.array_equal(_bits(got["obs"][e]), _bits(want["obs_out"])), (name, e)
            assert set(np.unique(got["known"][e])) <= {0, 1}
            if name == "far":
                assert not want["known"].any() and (got["est"][e] == 0).all()
            elif name in ("same", "one"):
                known += int(want["known"].sum())
                assert want["known"].any() and (want["est"] > 0).any(), (name, e)
    assert known > (100 if G >= 24 else 10)
    assert (p["base"][2][:2] < 0).all() and (before["origin"][2] < 0).all()     # one env at negative x and y
    rig.close()


# ---------------------------------------------------------------- 4. the schedule, behind a real camera
class Twin:
    """an ElevationMap without follow_sensor on the buffers and the image of a real env whose camera has a period above 1: ticked by the test at the
    fresh calls and at no other"""

    def __init__(self, env, **settings):
        cc = env.depth_camera.config
        one = depth_mod.config_struct(cc.width, cc.height, cc.fovy_deg, cc.near, cc.far, 0, tuple(cc.mount_pos), tuple(cc.mount_quat), every=1)
        self.env = types.SimpleNamespace(depth=env.depth, depth_camera=types.SimpleNamespace(config=one), buffers=env.buffers, device=env.device,
                                         num_envs=env.num_envs, observation_size=env.observation_size, config=env.config, method=env.method)
        self.map = elevation.ElevationMap(self.env, **settings)


def walk(env, cells, frac):
    """put every base at fraction `frac` of world cell cells[e] ([n, 2])"""
    env.buffers["state"][0:2] = torch.from_numpy(((np.asarray(cells) + frac) * RES).astype(np.float32).T.copy()).cuda()


def maps_of(em):
    torch.cuda.synchronize()
    return {k: getattr(em, k).cpu().numpy().copy() for k in OUT}


@pytest.mark.parametrize("every", (2, 3))
def test_the_schedule(every):
    env = make_env(3, 11, variant=[0, 2, 7], depth=dict(width=16, height=12, every=every))
    settings = dict(grid=64, res=RES, alpha=0.5, self_half=(0.45, 0.25, 0.45))
    a, b = elevation.ElevationMap(env, follow_sensor=True, **settings), Twin(env, **settings).map
    assert a.sensor_every == every and a.sensor_counter is env.depth_camera.counter
    env.depth_camera.counter.zero_()                                          # make_env's reset ticked the camera: the schedule starts here
    cells = np.floor(env.buffers["state"][0:2].cpu().numpy().T.astype(float) / RES)
    prev = None
    for c in range(7):
        cells[:, 0] += 1
        walk(env, cells, 0.37)
        env.depth_camera.tick()
        a.tick(clear_all=c == 0)
        if c % every == 0:
            b.tick(clear_all=c == 0)
        ga, gb = maps_of(a), maps_of(b)
        same(ga, gb, keys=("map", "origin"), msg=c)                           # the twin did nothing in between
        if c % every == 0:
            same(ga, gb, msg=c)
            assert prev is None or not np.array_equal(_bits(prev["map"]), _bits(ga["map"])), c
            assert np.array_equal(ga["origin"], cells), c
        else:
            same(prev, ga, keys=("map", "origin"), msg=c)
            assert not np.array_equal(ga["origin"], cells)
            for e in range(3):                                                # the scan comes from the held map, at the pose of this step
                S = env.buffers["state"][:7, e].cpu().numpy().astype(float)
                want = fol.hold((ga["map"][e], ga["origin"][e]), S, CFG)
                keep = want["scan"]["margin"] >= MARGIN
                assert np.array_equal(ga["known"][e][keep] != 0, want["known"][keep]), (c, e)
                if keep.all():
                    assert np.array_equal(_bits(ga["est"][e]), _bits(want["est"])), (c, e)
        prev = ga
    assert int(env.depth_camera.counter.item()) == 7 and (~np.isnan(prev["map"])).sum() > 50
    # force off phase: c = 7 is no multiple of 2 or 3, and the call is a full tick
    cells[:, 1] -= 2
    walk(env, cells, 0.37)
    env.depth_camera.tick(force=True)
    a.tick(force=True); b.tick()
    ga, gb = maps_of(a), maps_of(b)
    same(ga, gb, msg="forced")
    assert np.array_equal(ga["origin"], cells) and not np.array_equal(_bits(prev["map"]), _bits(ga["map"]))
    a.close(); b.close(); env.close()


# ---------------------------------------------------------------- 5. clears on a hold call
@pytest.mark.parametrize("name,kw,done", [("use_done", dict(use_done=True), (0, 1, 0)), ("mask", dict(clear_mask=(0, 1, 0)), (0, 0, 0)),
                                          ("clear_all", dict(clear_all=True), (0, 0, 0))])
@pytest.mark.parametrize("G", (9, 24))
def test_clears_on_a_hold(G, name, kw, done):
    camera, settings, ticks = setup(G)
    cleared = (1, 1, 1) if name == "clear_all" else (0, 1, 0)
    rig, new = FollowRig(3, camera, every=3, **settings), FollowRig(3, camera, follow=False, **settings)
    p = poses()
    rig.put(state_of(p["base"]), ticks[0][1], observations())
    rig.call(c=0, clear_all=True)
    rig.map.map.copy_(torch.from_numpy(crafted(np.random.default_rng(G), 3, G)))
    before = rig.read()
    rig.put(qpos=p["five"])
    rig.env.buffers["done"].copy_(torch.tensor(done, dtype=torch.float32))
    if "clear_mask" in kw:
        kw = dict(kw, clear_mask=torch.tensor(kw["clear_mask"], dtype=torch.uint8))
    got = rig.call(c=1, **kw)
    for e in range(3):
        if cleared[e]:
            assert np.isnan(got["map"][e]).all() and np.array_equal(got["origin"][e], (BASE_CELLS + MOVES["five"])[e]), (name, e)
            assert (got["est"][e] == 0).all() and (got["known"][e] == 0).all() and (got["obs"][e][38:155] == 0).all()
            assert np.array_equal(_bits(got["obs"][e][:38]), _bits(observations()[e][:38])) and np.array_equal(_bits(got["obs"][e][155:]), _bits(observations()[e][155:]))
        else:
            same(before, got, keys=("map", "origin"), rows=e, msg=(name, e))
            want = fol.hold((got["map"][e], got["origin"][e]), p["five"][e], CFG, obs=observations()[e])
            assert np.array_equal(got["known"][e] != 0, want["known"]) and np.array_equal(_bits(got["est"][e]), _bits(want["est"]))
    # done without use_done clears nothing
    if name == "use_done":
        again = rig.call(c=2, use_done=False)
        same(got, again)
    # the next fresh call gives a cleared env what a handle that starts from nothing gives
    rig.env.buffers["done"].zero_()
    rig.put(qpos=p["one"], data=ticks[1][1])
    new.put(state_of(p["one"]), ticks[1][1], observations())
    ga, gb = rig.call(c=3), new.call(clear_all=True)
    for e in range(3):
        if cleared[e]:
            same(ga, gb, rows=e, msg=(name, e))
    assert np.array_equal(ga["origin"], BASE_CELLS + MOVES["one"])
    rig.close(); new.close()


# ---------------------------------------------------------------- 6. batch independence, determinism, the fill behind a hold
def _fresh_then_hold(n, cols, G=24, K=4):
    """a fresh call and a hold behind it with the base moved by a cell, for a batch whose env i has the rows of env cols[i] -> the hold's outputs,
    the fill's, the poses"""
    camera, settings, ticks = setup(G)
    rig = FollowRig(n, camera, every=3, fill=K, **settings)
    p = poses()
    rig.put(state_of(p["base"][cols]), ticks[0][1][cols], observations()[cols])
    rig.call(c=0, clear_all=True)
    rig.map.map[:, ::2, 1::3] = 0.125                                         # something known near every base, whatever the image gave
    rig.put(qpos=p["one"][cols])
    got = rig.call(c=1)
    got["filled_est"], got["filled_dist"], got["filled_obs"] = (getattr(rig.map, k).cpu().numpy().copy() for k in ("filled_est", "filled_dist", "filled_obs"))
    rig.close()
    return got, p["one"][cols]


def test_batch_independence_determinism_and_the_fill():
    keys = OUT + ("filled_est", "filled_dist", "filled_obs")
    three, q = _fresh_then_hold(3, [0, 1, 2])
    again, _ = _fresh_then_hold(3, [0, 1, 2])
    big, _ = _fresh_then_hold(65, [0] + [1] * 63 + [2])
    same(three, again, keys=keys)
    for e, pos in ((0, 0), (2, 64)):
        alone, _ = _fresh_then_hold(1, [e])
        for k in keys:
            assert np.array_equal(_bits(three[k][e]), _bits(alone[k][0])), (k, e)
            assert np.array_equal(_bits(three[k][e]), _bits(big[k][pos])), (k, e)
    for pos in range(1, 64):
        for k in keys:
            assert np.array_equal(_bits(three[k][1]), _bits(big[k][pos])), (k, pos)
    filled = 0
    for e in range(3):                                                        # the fill behind a hold: the held window at the current pose
        f = fref.fill(three["map"][e], three["origin"][e], 4)
        sc = fref.sample(f["map"], f["dist"], three["origin"][e], q[e], CFG)
        assert sc["margin"].min() >= MARGIN
        assert np.array_equal(three["filled_dist"][e], sc["dist"]) and same_floats(three["filled_est"][e], sc["est"]), e
        assert np.array_equal(_bits(three["filled_obs"][e][38:155]), _bits(three["filled_est"][e]))
        filled += int(((sc["dist"] > 0) & (sc["dist"] < 255)).sum())
        assert np.array_equal(three["filled_dist"][e] == 0, three["known"][e] != 0)
    assert filled > 0 and three["known"].sum() > 30


# ---------------------------------------------------------------- 7. one captured step
def test_a_captured_step():
    """sensor tick, follow, fill captured once on one stream - a chain, no parallel branches - and replayed six times behind a base that walks:
    equal to six eager steps of a twin env, bit for bit; with every = 3 the replays are fresh, hold, hold, fresh, hold, hold"""
    mk = lambda: make_env(3, 11, variant=[0, 2, 7], depth=dict(width=16, height=12, every=3),
                          elevation=dict(grid=24, res=RES, alpha=0.5, fill=4, follow_sensor=True))
    a, b = mk(), mk()
    keys = OUT + ("filled_est", "filled_dist", "filled_obs")

    def step(env):
        env.depth_camera.tick()
        env.elevation_map.tick(use_done=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(a)
    torch.cuda.current_stream().wait_stream(s)
    step(b)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(a)
    torch.cuda.synchronize()
    for env in (a, b):
        env.depth_camera.counter.fill_(3)                                     # both start on a fresh call, whatever the warm-up counted
    cells = np.floor(a.buffers["state"][0:2].cpu().numpy().T.astype(float) / RES)
    changed = []
    for t in range(6):
        cells[:, 0] += 1
        walk(a, cells, 0.37); walk(b, cells, 0.37)
        before = a.elevation_map.map.clone()
        g.replay(); step(b)
        torch.cuda.synchronize()
        for k in keys:
            assert np.array_equal(_bits(getattr(a.elevation_map, k)), _bits(getattr(b.elevation_map, k))), (k, t)
        assert np.array_equal(_bits(a.depth), _bits(b.depth)) and int(a.depth_camera.counter.item()) == int(b.depth_camera.counter.item()) == 4 + t
        changed.append(not torch.equal(torch.nan_to_num(before), torch.nan_to_num(a.elevation_map.map)))
    assert changed == [True, False, False, True, False, False]
    a.close(); b.close()


# ---------------------------------------------------------------- 8. refusals
def test_refusals_and_guard_bands():
    G, n = 24, 3
    L = elevation.lib()
    msg = lambda: L.pgtt_elevation_last_error().decode()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    camera, _ = recorded(16, 12)
    cam = {k: camera[k] for k in ("width", "height", "fovy", "near", "far", "mount_pos", "mount_quat")}
    cfg = elevation.config_struct(**cam, grid=G, res=RES, obs_dim=171, scan_row0=38)
    h = C.c_void_p()
    elevation.check(L.pgtt_elevation_create(C.byref(cfg), 0, n, C.byref(h)))
    dev = torch.device("cuda:0")
    counter = torch.ones(1, dtype=torch.int64, device=dev)
    outs = dict(map=Guarded(n, G, G, front=20), origin=Guarded(n, 2, dtype=torch.int32, fill=-77777), est=Guarded(n, 117),
                known=Guarded(n, 117, dtype=torch.uint8, fill=201, front=21, back=17), obs_out=Guarded(n, 171, front=17))
    t = dict(state=torch.from_numpy(state_of(poses()["base"])).to(dev), depth=torch.full((n, camera["height"], camera["width"]), 1.0, device=dev),
             obs=torch.from_numpy(observations()).to(dev))
    b = elevation.PgttElevationBuffers()
    for k, v in t.items():
        setattr(b, k, v.data_ptr())
    for k, g in outs.items():
        setattr(b, k, g.ptr())
    # nothing bound; the rate alone; the buffers alone
    assert L.pgtt_elevation_follow(h, None, 1, 0, 0, stream()) == E_STATE and "bind" in msg()
    assert L.pgtt_elevation_bind_rate(h, None, 3) == E_ARG and "counter" in msg()
    for every in (0, -1):
        assert L.pgtt_elevation_bind_rate(h, counter.data_ptr(), every) == E_ARG and "every" in msg()
    assert L.pgtt_elevation_bind_rate(None, counter.data_ptr(), 3) == E_ARG and L.pgtt_elevation_follow(None, None, 1, 0, 0, stream()) == E_ARG
    assert L.pgtt_elevation_bind(h, C.byref(b)) == 0
    assert L.pgtt_elevation_follow(h, None, 1, 0, 0, stream()) == E_STATE and "pgtt_elevation_bind_rate" in msg()   # no refused bind_rate bound anything
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs.values())
    # the rate persists across a later bind of the buffers; bound before the buffers it would have done too
    assert L.pgtt_elevation_bind_rate(h, counter.data_ptr(), 3) == 0
    assert L.pgtt_elevation_bind(h, C.byref(b)) == 0
    assert L.pgtt_elevation_follow(h, None, 1, 0, 0, stream()) == 0                                          # c = 0: fresh
    counter.fill_(2)
    assert L.pgtt_elevation_follow(h, None, 0, 0, 0, stream()) == 0                                          # c = 1: a hold
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in outs.values()) and outs["est"].written() and outs["obs_out"].written()
    assert np.array_equal(outs["origin"].view.cpu().numpy(), BASE_CELLS)
    assert L.pgtt_elevation(h, None, 0, 0, stream()) == 0                                                    # the plain entry is what it was
    torch.cuda.synchronize()
    L.pgtt_elevation_destroy(h)
    # the Python object: without the flag the refusals stand, with it the torso-only one does
    rig = FollowRig(1, camera, every=1, grid=G)
    rig.env.depth_camera.config.every = 2
    with pytest.raises(ValueError, match="period 1"):
        elevation.ElevationMap(rig.env)
    elevation.ElevationMap(rig.env, follow_sensor=True).close()
    rig.env.depth_camera.config.mount_body = 3
    with pytest.raises(ValueError, match="torso"):
        elevation.ElevationMap(rig.env, follow_sensor=True)
    rig.close()


# ---------------------------------------------------------------- 9. the env
def _walk_envs(envs, steps, seed=6):
    rng = np.random.default_rng(seed)
    n = envs[0].num_envs
    for t in range(steps):
        act = torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda()
        outs = [env.step(act) for env in envs]
        torch.cuda.synchronize()
        yield t, outs


# The window of G = 24 reaches 0.48 m from the base; the default camera's lowest ray meets level ground 0.5 m ahead of the base and the default self
# box drops what is nearer than 0.45 m, so that map holds a few cells of a riser at most and may not change at a fresh call on which the base stays in
# its cell: there the case asserts what a fresh call always does (the origin is the base's cell) and that a hold changes nothing; the LiDAR, which sees
# the ground all round, and the camera with G = 64 are held to the whole pattern.
@pytest.mark.parametrize("source,G", (("depth", 24), ("depth", 64), ("lidar", 24)))
def test_env_integration(source, G):
    strict = (source, G) != ("depth", 24)
    if source == "depth":
        sensor = dict(depth=dict(width=16, height=12, every=3))
        emap = dict(grid=G, fill=4, follow_sensor=True)
    else:
        sensor = dict(lidar=dict(every=3))
        emap = dict(grid=G, fill=4, follow_sensor=True, source="lidar", alpha=0.5)
    a, b = make_env(8, 5, autoreset=True, elevation=emap, **sensor), make_env(8, 5, autoreset=True, **sensor)
    em = a.elevation_map
    sens = a.depth_camera if source == "depth" else a.lidar_scanner
    assert em.follow_sensor and em.sensor_every == 3 and em.sensor_counter is sens.counter and b.elevation_map is None
    assert int(sens.counter.item()) == 1                                      # reset() ticked it with force, and the map behind it
    prev = maps_of(em)
    print(f"{source} G={G}: cells known after reset {int((~np.isnan(prev['map'])).sum())}")
    assert not strict or (~np.isnan(prev["map"])).sum() > 20
    moved = []
    for t, ((oa, ra, da, _), (ob, rb, db, _)) in _walk_envs([a, b], 7):
        pairs = [(oa["state"], ob["state"]), (oa["privileged_state"], ob["privileged_state"]), (ra, rb), (da, db), (a.buffers["state"], b.buffers["state"])]
        pairs.append((a.depth, b.depth) if source == "depth" else (a.lidar_points, b.lidar_points))
        for i, (x, y) in enumerate(pairs):
            assert np.array_equal(_bits(x), _bits(y)), (t, i)
        now = maps_of(em)
        eo, so = _bits(a.elevation_obs), _bits(oa["state"])
        assert np.array_equal(eo[:, :38], so[:, :38]) and np.array_equal(eo[:, 155:], so[:, 155:]) and np.array_equal(eo[:, 38:155], _bits(em.est))
        assert np.isfinite(now["est"]).all() and (not strict or now["known"].sum() > 0)       # scan rows on every step
        fo = _bits(a.elevation_filled_obs)
        assert np.array_equal(fo[:, 38:155], _bits(em.filled_est)) and np.array_equal(fo[:, :38], so[:, :38])
        done = da.cpu().numpy() != 0
        quiet = ~done                                                         # a finished episode clears its map on any step
        moved.append(not np.array_equal(_bits(prev["map"][quiet]), _bits(now["map"][quiet])) or not np.array_equal(prev["origin"][quiet], now["origin"][quiet]))
        for e in np.flatnonzero(done):
            if (int(sens.counter.item()) - 1) % 3 != 0:
                assert np.isnan(now["map"][e]).all() and (now["known"][e] == 0).all()
        S = a.buffers["state"][:7].cpu().numpy().astype(float)
        c = int(sens.counter.item()) - 1                                      # what the sensor's call of this step found
        if c % 3 == 0:                                                        # a fresh call leaves the origin at the base's cell
            sure = ref.border_margin(S[:2].T, RES32) >= 1e-5
            assert np.array_equal(now["origin"][sure], ref.cell(S[:2].T, RES32)[sure]), t
        else:
            assert not moved[-1], t
        for e in range(8):                                                    # the scan is the held (or fresh) map's at this step's pose
            want = fol.hold((now["map"][e], now["origin"][e]), S[:, e], dict(CFG, scan_dist_x=a.config["scan_dist_x"], scan_dist_y=a.config["scan_dist_y"]))
            keep = want["scan"]["margin"] >= MARGIN
            assert np.array_equal(now["known"][e][keep] != 0, want["known"][keep]), (t, e)
            if keep.all():
                assert np.array_equal(_bits(now["est"][e]), _bits(want["est"])), (t, e)
        prev = now
    # the sensor's counter read 1 after reset: the steps find c = 1 .. 7, and the camera's own are c = 3 and 6 - the third and the sixth step
    print(f"{source} G={G}: the map moved at steps {moved}")
    assert not strict or moved == [False, False, True, False, False, True, False], moved
    a.close(); b.close()


def test_follow_sensor_with_every_1_changes_nothing():
    emap = dict(grid=24, fill=4)
    a = make_env(8, 5, autoreset=True, depth=dict(width=16, height=12), elevation=dict(emap, follow_sensor=True))
    b = make_env(8, 5, autoreset=True, depth=dict(width=16, height=12), elevation=emap)
    keys = OUT + ("filled_est", "filled_dist", "filled_obs")
    assert a.elevation_map.follow_sensor and not b.elevation_map.follow_sensor
    for k in keys:
        assert np.array_equal(_bits(getattr(a.elevation_map, k)), _bits(getattr(b.elevation_map, k))), k
    for t, _ in _walk_envs([a, b], 4):
        for k in keys:
            assert np.array_equal(_bits(getattr(a.elevation_map, k)), _bits(getattr(b.elevation_map, k))), (k, t)
    a.reset(5, mask=torch.tensor([1, 0, 0, 1, 0, 0, 0, 0], dtype=torch.uint8)); b.reset(5, mask=torch.tensor([1, 0, 0, 1, 0, 0, 0, 0], dtype=torch.uint8))
    torch.cuda.synchronize()
    for k in keys:
        assert np.array_equal(_bits(getattr(a.elevation_map, k)), _bits(getattr(b.elevation_map, k))), k
    assert (~torch.isnan(a.elevation_map.map)).sum() > 20
    a.close(); b.close()
