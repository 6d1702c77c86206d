"""pgtt_elevation_fill on the GPU against the numpy statement of tests/elevation_fill_reference.py.

The device's inputs are tensors the test writes: `map` and `origin` are crafted on the host and `ElevationMap.fill()` launches the fill alone, so
there is no rounding between the reference and the device in the dense outputs - they are compared bit for bit, every cell.  The scan outputs depend
on which cell a scan point falls into, computed in fp32 on the device: the coordinate is a three-term sum of magnitude <= 20 m followed by one
division, so its error is a few ulp(20) ~ 1e-5 m, and the poses are chosen by rejection so that every scan point is at least 1e-4 m from a cell
border (about 8 x that); nothing is left out, and the test asserts the margin itself.  `est` is then one fp32 subtraction of two of the map's values:
compared bit for bit, where inf - inf is a NaN on both sides (its sign is the platform's)."""
import ctypes as C
import math
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_fill_reference as fref  # noqa: E402
import elevation_reference as ref  # noqa: E402
from test_gpu_elevation import RES, Rig, _bits, make_env, recorded  # noqa: E402
from test_gpu_learn_kernels import Guarded  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, elevation  # noqa: E402

pytestmark = pytest.mark.gpu

CAMERA = dict(width=16, height=12, fovy=58.0, near=0.1, far=3.0, mount_pos=(0.3, 0.0, 0.05), mount_quat=(1.0, 0.0, 0.0, 0.0))
RES32 = float(np.float32(RES))
CFG = dict(res=RES, scan_dist_x=0.1, scan_dist_y=0.1)
MARGIN = 1e-4
SHARES = ("none", "one", 0.05, 0.5, "all")
TICK_OUT = ("map", "origin", "est", "known", "obs")
FILLED = ("filled_est", "filled_dist", "filled_obs", "filled_map", "filled_dist_map")
E_ARG, E_STATE = -1, -2


def pose(rng, G):
    """a base within 20 m of the world's origin at any yaw, a little rolled and pitched, whose 117 scan points all lie at least MARGIN from a cell
    border and whose cell is no multiple of G on either axis -> (qpos [7] of fp32 values, origin [2])"""
    while True:
        yaw = rng.uniform(-math.pi, math.pi)
        q = np.array([math.cos(yaw / 2), 0.03 * rng.normal(), 0.03 * rng.normal(), math.sin(yaw / 2)])
        qpos = np.concatenate([rng.uniform(-20, 20, 2), [0.4], q]).astype(np.float32).astype(float)
        origin = ref.cell(qpos[:2], RES32)
        if (origin % G == 0).any() or ((origin - G // 2) % G == 0).any():
            continue
        if ref.border_margin(ref.scan_points(qpos), RES32).min() >= MARGIN:
            return qpos, origin


def crafted_map(rng, G, share, specials):
    m = np.full((G, G), np.nan, np.float32)
    if share == "none":
        return m
    if share == "one":
        m[rng.integers(G), rng.integers(G)] = np.float32(rng.normal())
        return m
    keep = np.ones((G, G), bool) if share == "all" else rng.random((G, G)) < share
    m[keep] = rng.normal(size=int(keep.sum())).astype(np.float32)
    if specials:                                                     # -0, +0, -inf, +inf among the known cells
        i, j = np.nonzero(keep)
        pick = rng.choice(len(i), min(4, len(i)), replace=False)
        m[i[pick], j[pick]] = np.array([-0.0, 0.0, -np.inf, np.inf], np.float32)[:len(pick)]
    return m


@lru_cache(maxsize=None)
def inputs(G):
    """ten envs: the five known shares, each at two poses - the first with +-0 and +-inf among its values, the second with finite values alone"""
    rng = np.random.default_rng(100 + G)
    maps, origins, qposs = [], [], []
    for share in SHARES:
        for specials in (True, False):
            q, o = pose(rng, G)
            maps.append(crafted_map(rng, G, share, specials)); origins.append(o); qposs.append(q)
    obs = rng.normal(size=(len(maps), 171)).astype(np.float32)
    return np.stack(maps), np.stack(origins), np.stack(qposs), obs


def run_fill(G, K, maps, origins, qpos, obs, dense=True):
    """the fill alone on crafted inputs -> the five outputs; what the tick owns is found as it was left"""
    n = len(maps)
    rig = Rig(n, CAMERA, grid=G, res=RES, fill=K, dense=dense)
    em = rig.map
    S = np.zeros((abi.NSTATE, n), np.float32)
    S[:7] = np.asarray(qpos, np.float32).T
    rig.env.buffers["state"].copy_(torch.from_numpy(S))
    rig.env.buffers["obs_state"].copy_(torch.from_numpy(np.ascontiguousarray(obs)))
    em.map.copy_(torch.from_numpy(np.ascontiguousarray(maps)))
    em.origin.copy_(torch.from_numpy(np.asarray(origins, np.int32)))
    em.est.fill_(-3.0); em.known.fill_(7); em.obs.fill_(-5.0)
    assert em.fill() is em.filled_obs
    torch.cuda.synchronize()
    assert np.array_equal(_bits(em.map), _bits(np.ascontiguousarray(maps))) and np.array_equal(em.origin.cpu().numpy(), origins)
    assert bool((em.est == -3.0).all()) and bool((em.known == 7).all()) and bool((em.obs == -5.0).all())
    out = {k: getattr(em, k).cpu().numpy().copy() for k in FILLED if dense or not k.endswith("map")}
    rig.close()
    return out


@lru_cache(maxsize=None)
def device(G, K):
    return run_fill(G, K, *inputs(G))


@lru_cache(maxsize=None)
def reference(G, K):
    maps, origins, qpos, obs = inputs(G)
    fills = [fref.fill(m, o, K) for m, o in zip(maps, origins)]
    scans = [fref.sample(f["map"], f["dist"], o, q, CFG) for f, o, q in zip(fills, origins, qpos)]
    return fills, scans


def same_floats(got, want):
    """bit for bit, a NaN at the same places"""
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g.view(np.int32)[~np.isnan(w)], w.view(np.int32)[~np.isnan(w)])


SIZES = [(G, K) for G in (8, 9, 24, 64, 96) for K in (1, 3, G - 1)]


# ---------------------------------------------------------------- 1. the dense outputs
@pytest.mark.parametrize("G,K", SIZES)
def test_dense_bit_for_bit(G, K):
    maps, origins, _, _ = inputs(G)
    assert (origins < 0).any() and (origins % G != 0).all()
    got, (fills, _) = device(G, K), reference(G, K)
    filled = 0
    for e, f in enumerate(fills):
        assert np.array_equal(got["filled_dist_map"][e], f["dist"]), (G, K, e)
        assert same_floats(got["filled_map"][e], f["map"]), (G, K, e)
        assert np.array_equal(np.isnan(f["map"]), f["dist"] == 255)
        filled += int(((f["dist"] > 0) & (f["dist"] < 255)).sum())
    assert filled > 0 and (fills[0]["dist"] == 255).all() and (fills[-1]["dist"] == 0).all()
    if G >= 24:                                                      # the special values took part: a -0 or an infinity was copied into a hole
        sp = [np.float32(v).view(np.int32) for v in (-0.0, -np.inf)]
        assert any(np.isin(got["filled_map"][e][(fills[e]["dist"] > 0) & (fills[e]["dist"] < 255)].view(np.int32), sp).any() for e in (4, 6))


# ---------------------------------------------------------------- 2. the seam
@pytest.mark.parametrize("G", (8, 9, 24))
def test_the_seam_on_the_device(G):
    origin = np.array([G // 2 + 3 - 5 * G, 2 - G])
    W = np.full((G, G), np.nan, np.float32)
    W[0, :] = np.arange(G, dtype=np.float32)
    m = fref.to_slots(W, origin)
    qpos = np.array([[0.0, 0.0, 0.4, 1.0, 0.0, 0.0, 0.0]])
    obs = np.zeros((1, 171), np.float32)
    for K in (G - 1, G - 2):
        got = run_fill(G, K, m[None], origin[None], qpos, obs)
        want = fref.fill(m, origin, K)
        D = fref.to_window(got["filled_dist_map"][0], origin)
        assert np.array_equal(D, want["D"]) and same_floats(got["filled_map"][0], want["map"])
        assert (D[G - 1] == (G - 1 if K == G - 1 else 255)).all() and (D[G - 1] != 1).all() and (D[1] == 1).all()


# ---------------------------------------------------------------- 3. the scan outputs
@pytest.mark.parametrize("G,K", SIZES)
def test_scan_outputs(G, K):
    maps, origins, qpos, obs = inputs(G)
    got, (_, scans) = device(G, K), reference(G, K)
    known = 0
    for e, sc in enumerate(scans):
        assert sc["margin"].min() >= MARGIN                          # no point is left out
        assert np.array_equal(got["filled_dist"][e], sc["dist"]), (G, K, e)
        assert same_floats(got["filled_est"][e], sc["est"]), (G, K, e)
        o, src = _bits(got["filled_obs"][e]), _bits(obs[e])
        assert np.array_equal(o[:38], src[:38]) and np.array_equal(o[155:], src[155:]) and np.array_equal(o[38:155], _bits(got["filled_est"][e]))
        known += int((sc["dist"] != 255).sum())
        if e % 2 == 1:
            assert np.isfinite(sc["est"]).all() and (sc["est"] >= 0).all()
    assert known > 0 and (scans[0]["dist"] == 255).all() and (got["filled_est"][0] == 0).all()
    if G >= 24:
        full = scans[-1]                                             # the fully known map: the scan inside the window is measured, and est has a spread
        assert (full["dist"] == 0).sum() > 20 and full["est"].max() > 0 and (full["est"] == 0).any()


# ---------------------------------------------------------------- 4. the tick is untouched
def test_the_tick_is_untouched():
    camera, ticks = recorded(16, 12)
    settings = dict(grid=24, res=RES, alpha=0.5, self_half=(0.12, 0.1, 0.45))
    camera = dict(camera, mount_pos=(camera["mount_pos"][0] - 0.5, 0.0, camera["mount_pos"][2]))       # the near field lands in the small window
    a, b = Rig(3, camera, fill=8, dense=True, **settings), Rig(3, camera, **settings)
    for t, (S, img, obs) in enumerate(ticks):
        for r in (a, b):
            r.put(S, img, obs)
        ga, gb = a.tick(clear_all=t == 0), b.tick(clear_all=t == 0)
        for k in TICK_OUT:
            assert np.array_equal(_bits(ga[k]), _bits(gb[k])), (k, t)
        # and the fill ran behind the tick, on the map it left
        for e in range(3):
            want = fref.fill(ga["map"][e], ga["origin"][e], 8)
            assert np.array_equal(a.map.filled_dist_map[e].cpu().numpy(), want["dist"]) and same_floats(a.map.filled_map[e].cpu().numpy(), want["map"])
    fd = a.map.filled_dist.cpu().numpy()
    assert (~np.isnan(ga["map"])).sum() > 50 and ((fd > 0) & (fd < 255)).any() and (fd[ga["known"] != 0] == 0).all()
    assert not hasattr(b.map, "filled_est") and not hasattr(b.map, "filled_map")
    a.close(); b.close()


# ---------------------------------------------------------------- 5. batch independence, determinism
def test_batch_independence_and_determinism():
    G, K = 24, 3
    maps, origins, qpos, obs = inputs(G)
    rows = [4, 6, 9]                                                  # a 5 % map with special values, a 50 % one, the full one
    take = lambda cols: (maps[cols], origins[cols], qpos[cols], obs[cols])
    three, again = run_fill(G, K, *take(rows)), run_fill(G, K, *take(rows))
    big = run_fill(G, K, *take([rows[0]] + [rows[1]] * 63 + [rows[2]]))
    whole = device(G, K)
    for k in FILLED:
        assert np.array_equal(_bits(three[k]), _bits(again[k])), k
        assert np.array_equal(_bits(three[k]), _bits(whole[k][rows])), k
        for i, pos in ((0, 0), (2, 64)):
            alone = run_fill(G, K, *take([rows[i]]))
            assert np.array_equal(_bits(three[k][i]), _bits(alone[k][0])), (k, i)
            assert np.array_equal(_bits(three[k][i]), _bits(big[k][pos])), (k, i)


# ---------------------------------------------------------------- 6. arguments
def test_arguments_and_guard_bands():
    G, K, n = 24, 3, 3                                               # whole 16-byte runs of the map, outputs at odd offsets: the mixed paths
    maps, origins, qpos, obs = (x[[4, 6, 9]] for x in inputs(G))
    L = elevation.lib()
    msg = lambda: L.pgtt_elevation_last_error().decode()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    outs = dict(est=Guarded(n, 117), dist=Guarded(n, 117, dtype=torch.uint8, fill=201, front=21, back=17), obs_out=Guarded(n, 171, front=17),
                map_out=Guarded(n, G, G), dist_out=Guarded(n, G, G, dtype=torch.uint8, fill=201, front=29))

    def struct(**drop):
        o = elevation.PgttElevationFill()
        for k, t in outs.items():
            setattr(o, k, None if k in drop else t.ptr())
        return o
    # a handle with nothing bound
    cfg = elevation.config_struct(**CAMERA, grid=G, res=RES, obs_dim=171, scan_row0=38)
    h = C.c_void_p()
    elevation.check(L.pgtt_elevation_create(C.byref(cfg), 0, n, C.byref(h)))
    assert L.pgtt_elevation_fill(h, stream()) == E_STATE and "bind" in msg()
    assert L.pgtt_elevation_bind_fill(h, None, K) == E_ARG and msg()
    for name in ("est", "dist"):
        assert L.pgtt_elevation_bind_fill(h, C.byref(struct(**{name: 1})), K) == E_ARG and msg(), name
    for passes in (0, -1, 96):
        assert L.pgtt_elevation_bind_fill(h, C.byref(struct()), passes) == E_ARG and "passes" in msg(), passes
    assert L.pgtt_elevation_fill(h, stream()) == E_STATE and msg()            # none of the refused binds bound anything
    for passes in (1, 95, K):
        assert L.pgtt_elevation_bind_fill(h, C.byref(struct()), passes) == 0
    assert L.pgtt_elevation_fill(h, stream()) == E_STATE and "bind" in msg()  # the outputs are bound, the buffers are not
    # the buffers, without obs: refused while the fill's obs_out is bound
    dev = torch.device("cuda:0")
    S = np.zeros((abi.NSTATE, n), np.float32)
    S[:7] = qpos.astype(np.float32).T
    t = dict(state=torch.from_numpy(S).to(dev), depth=torch.zeros(n, CAMERA["height"], CAMERA["width"], device=dev), obs=torch.from_numpy(obs).to(dev),
             map=torch.from_numpy(maps).to(dev), origin=torch.from_numpy(origins.astype(np.int32)).to(dev), est=torch.zeros(n, 117, device=dev),
             known=torch.zeros(n, 117, dtype=torch.uint8, device=dev))

    def buffers(with_obs):
        b = elevation.PgttElevationBuffers()
        for k, v in t.items():
            setattr(b, k, v.data_ptr() if with_obs or k != "obs" else None)
        return b
    assert L.pgtt_elevation_bind(h, C.byref(buffers(False))) == 0
    assert L.pgtt_elevation_fill(h, stream()) == E_ARG and "obs" in msg()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs.values())
    assert L.pgtt_elevation_bind_fill(h, C.byref(struct(obs_out=1, map_out=1, dist_out=1)), K) == 0      # the optional ones may be NULL
    assert L.pgtt_elevation_fill(h, stream()) == 0
    torch.cuda.synchronize()
    assert outs["est"].written() and outs["dist"].written() and all(outs[k].untouched() for k in ("obs_out", "map_out", "dist_out"))
    first = outs["est"].view.clone()
    # the binding persists across a later bind of the buffers; now everything is bound
    assert L.pgtt_elevation_bind_fill(h, C.byref(struct()), K) == 0
    assert L.pgtt_elevation_bind(h, C.byref(buffers(True))) == 0
    assert L.pgtt_elevation_fill(h, stream()) == 0
    torch.cuda.synchronize()
    for k, g in outs.items():
        assert g.guards_intact(), k
    assert torch.equal(first.view(torch.int32), outs["est"].view.view(torch.int32))
    for e in range(n):
        f = fref.fill(maps[e], origins[e], K)
        sc = fref.sample(f["map"], f["dist"], origins[e], qpos[e], CFG)
        assert np.array_equal(outs["dist_out"].view[e].cpu().numpy(), f["dist"]) and same_floats(outs["map_out"].view[e].cpu().numpy(), f["map"])
        assert np.array_equal(outs["dist"].view[e].cpu().numpy(), sc["dist"]) and same_floats(outs["est"].view[e].cpu().numpy(), sc["est"])
        o = _bits(outs["obs_out"].view[e])
        assert np.array_equal(o[:38], _bits(obs[e])[:38]) and np.array_equal(o[155:], _bits(obs[e])[155:]) and np.array_equal(o[38:155], _bits(outs["est"].view[e]))
    assert np.array_equal(_bits(t["map"]), _bits(maps))
    L.pgtt_elevation_destroy(h)
    # the Python object
    rig = Rig(1, CAMERA, grid=G)
    with pytest.raises(elevation.ElevationError, match="fill=0"):
        rig.map.fill()
    assert rig.map.passes == 0 and not any(hasattr(rig.map, k) for k in FILLED)
    rig.close()
    rig = Rig(1, CAMERA, grid=G, fill=True)
    assert rig.map.passes == 16 and rig.map.filled_dist.shape == (1, 117) and not hasattr(rig.map, "filled_map")
    rig.close()


# ---------------------------------------------------------------- 7. graph capture
def test_graph_capture():
    """a tick and its fill captured on a stream and replayed three times equal three eager calls bit for bit; the two launches are a chain"""
    camera, ticks = recorded(64, 48)
    settings = dict(grid=64, res=RES, alpha=0.5, self_half=(0.45, 0.25, 0.45), fill=8, dense=True)
    S, img, obs = ticks[0]
    a, b = Rig(3, camera, **settings), Rig(3, camera, **settings)
    for r in (a, b):
        r.put(S, img, obs)
        r.map.map[:, ::3, :].fill_(0.25)                                          # alpha = 0.5 moves every touched known cell at every tick; holes remain
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
    for t in range(3):
        before = b.map.filled_map.clone()
        g.replay(); b.map.tick()
        torch.cuda.synchronize()
        for k in TICK_OUT + FILLED:
            assert np.array_equal(_bits(getattr(a.map, k)), _bits(getattr(b.map, k))), (k, t)
        assert not torch.equal(torch.nan_to_num(before), torch.nan_to_num(b.map.filled_map))
    d = b.map.filled_dist_map
    assert bool(((d > 0) & (d < 255)).any())
    a.close(); b.close()


# ---------------------------------------------------------------- 8. the env
def _check_env_fill(env, tally):
    """the env's fill against the reference on the device's own map, origin and state"""
    em = env.elevation_map
    torch.cuda.synchronize()
    maps, origins, S = em.map.cpu().numpy(), em.origin.cpu().numpy(), env.buffers["state"].cpu().numpy()
    obs, fo, fe, fd = (_bits(x) for x in (env.buffers["obs_state"], env.elevation_filled_obs, em.filled_est, env.elevation_dist))
    assert fd is not None and np.array_equal(fo[:, :38], obs[:, :38]) and np.array_equal(fo[:, 155:], obs[:, 155:]) and np.array_equal(fo[:, 38:155], fe)
    cfg = dict(res=em.res, scan_dist_x=env.config["scan_dist_x"], scan_dist_y=env.config["scan_dist_y"])
    for e in range(env.num_envs):
        f = fref.fill(maps[e], origins[e], em.passes)
        if em.dense:
            assert np.array_equal(em.filled_dist_map[e].cpu().numpy(), f["dist"]) and same_floats(em.filled_map[e].cpu().numpy(), f["map"]), e
        sc = fref.sample(f["map"], f["dist"], origins[e], S[:7, e].astype(float), cfg)
        keep = sc["margin"] >= MARGIN
        tally["points"] += ref.NSCAN; tally["out"] += int((~keep).sum())
        assert np.array_equal(fd[e][keep], sc["dist"][keep]), e
        if keep.all():
            tally["strict"] += 1
            assert same_floats(em.filled_est[e].cpu().numpy(), sc["est"]), e
        tally["filled"] += int(((sc["dist"] > 0) & (sc["dist"] < 255)).sum())


@pytest.mark.parametrize("source", ("depth", "lidar"))
def test_env_integration(source):
    if source == "depth":
        sensor, with_fill, without = dict(depth={}), dict(fill=8, dense=True), True
    else:
        sensor, with_fill, without = dict(lidar={}), dict(source="lidar", fill=8), dict(source="lidar")
    a, b = make_env(8, 5, autoreset=True, elevation=with_fill, **sensor), make_env(8, 5, autoreset=True, elevation=without, **sensor)
    assert b.elevation_filled_obs is None and b.elevation_dist is None
    assert a.elevation_filled_obs.shape == (8, 171) and a.elevation_dist.shape == (8, 117) and a.elevation_dist.dtype == torch.uint8
    tally = dict(points=0, out=0, strict=0, filled=0)

    def same():
        torch.cuda.synchronize()
        pairs = [(a.buffers["obs_state"], b.buffers["obs_state"]), (a.buffers["state"], b.buffers["state"]), (a.elevation_obs, b.elevation_obs),
                 (a.elevation_known, b.elevation_known), (a.elevation_map.map, b.elevation_map.map), (a.elevation_map.origin, b.elevation_map.origin)]
        if source == "depth":
            pairs.append((a.depth, b.depth))
        for i, (x, y) in enumerate(pairs):
            assert np.array_equal(_bits(x), _bits(y)), i
    same()
    _check_env_fill(a, tally)
    rng = np.random.default_rng(6)
    for t in range(3):
        act = torch.from_numpy(np.tanh(rng.normal(size=(8, 12)) * 0.6).astype(np.float32)).cuda()
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        for x, y in ((oa["state"], ob["state"]), (oa["privileged_state"], ob["privileged_state"]), (ra, rb), (da, db)):
            assert np.array_equal(_bits(x), _bits(y)), t
        same()
        _check_env_fill(a, tally)
    # one episode ended by hand: the masked envs' maps are cleared, and their fills start from the new episode's first view
    mask = torch.tensor([1, 0, 0, 1, 0, 0, 0, 0], dtype=torch.uint8)
    a.reset(5, mask=mask); b.reset(5, mask=mask)
    same()
    _check_env_fill(a, tally)
    assert tally["out"] <= 0.05 * tally["points"] and tally["strict"] >= 1 and tally["filled"] > 0, tally
    assert bool((a.elevation_dist[a.elevation_known != 0] == 0).all())
    a.close(); b.close()
    assert a.elevation_filled_obs is None and a.elevation_dist is None
