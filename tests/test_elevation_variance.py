"""The variance-weighted elevation map without a GPU: facts that hold tests/elevation_variance_reference.py (the fp64 statement of the variance
tick of include/pgtt_elevation.h that tests/test_gpu_elevation_variance.py compares the kernel with) on its own, and the host side: the refusals
of pgtt_elevation_check_var, the struct's size, and the refusals of Joystick and ElevationMap that come before anything touches a device."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_reference as dref  # noqa: E402
import elevation_reference as ref  # noqa: E402
import elevation_variance_reference as vref  # noqa: E402

from phase_guided_terrain_traversal_amd import configs, elevation  # noqa: E402

CAM = dict(fovy=58.0, near=0.1, far=3.0, mount_pos=(0.0, 0.0, 0.0), mount_quat=dref.pitch_quat(30.0).astype(np.float32).astype(float), res=0.04, alpha=1.0,
           self_half=(0.0, 0.0, 0.0))
DOWN = dict(CAM, mount_quat=dref.pitch_quat(90.0).astype(np.float32).astype(float))          # a camera that looks straight down
PTS = dict(res=0.04, self_half=(0.0, 0.0, 0.0))                                             # the points source needs no camera
W, H = 64, 48
G = 64


def image(qpos, cfg, boxes=(), w=W, h=H, dtype=np.float32):
    """the noise-free image of the plane z = 0 and `boxes` from the camera of `cfg` on a base at `qpos` (depth_reference's ray caster)"""
    cam = ref.camera_pose(qpos, cfg["mount_pos"], cfg["mount_quat"])
    return dref.depth_image(cam, cfg["fovy"], w, h, cfg["near"], cfg["far"], boxes)["depth"].astype(dtype)


def test_settings_match_the_module():
    assert vref.DEFAULTS == elevation.VARIANCE_DEFAULTS and vref.MAX_BAND == elevation.MAX_BAND
    assert elevation.variance_settings(None) is None and elevation.variance_settings(False) is None
    assert elevation.variance_settings(True) == elevation.VARIANCE_DEFAULTS and elevation.variance_settings(dict(band=0.1))["band"] == 0.1


def test_one_pixel_per_cell_is_the_maximum_map():
    """with one pixel per cell and process = 0, the first tick's map is elevation_reference's (alpha = 1), exactly: m is zmax bit for bit"""
    qpos = np.array([0.013, -0.021, 0.3, 0.99, 0.02, -0.03, 0.1])
    img = image(qpos, CAM, w=32, h=24)
    first = ref.tick(ref.new_state(G), qpos, img, CAM, clear=True)
    rel = first["cell"] - (first["origin"] - G // 2)
    use = first["kept"] & ((rel >= 0) & (rel < G)).all(1)
    seen, flat = set(), img.reshape(-1).copy()
    for p in np.flatnonzero(use):                                                  # every pixel after a cell's first reads `far`: one pixel per cell
        c = tuple(first["cell"][p])
        if c in seen:
            flat[p] = CAM["far"]
        seen.add(c)
    img = flat.reshape(img.shape)
    want = ref.tick(ref.new_state(G), qpos, img, CAM, clear=True)
    got = vref.tick(vref.new_state(G), qpos, img, CAM, vref.settings(dict(process=0.0)), clear=True)
    assert want["touched"].sum() > 100 and (got["n"][want["touched"]] == 1).all() and (got["S"] == 0).all()
    assert np.array_equal(got["map"], want["map"], equal_nan=True) and np.array_equal(got["est"], want["est"])
    assert np.array_equal(np.isnan(got["var"]), np.isnan(got["map"])) and (got["branch"][want["touched"]] == 1).all()


def test_a_fixed_pose_ticked_k_times():
    """the same noise-free image K times from one pose: h does not move, v = r / K"""
    qpos = np.array([0.013, -0.021, 0.3, 1.0, 0.0, 0.0, 0.0])
    img = image(qpos, CAM, [dict(c=np.array([1.0, 0.0, 0.1]), A=np.eye(3), h=np.array([0.3, 0.4, 0.1]))])
    var = vref.settings(dict(process=0.0))
    state, K = vref.new_state(G), 7
    for k in range(1, K + 1):
        out = vref.tick(state, qpos, img, CAM, var, clear=k == 1)
        if k == 1:
            first = out
        t = first["touched"]
        assert np.array_equal(out["touched"], t) and np.array_equal(out["map"][t], first["map"][t])
        assert np.abs(out["var"][t] * k / first["r"][t] - 1).max() <= 1e-12
        assert (out["branch"][t] == (1 if k == 1 else 2)).all()
        state = (out["map"], out["var"], out["origin"])
    assert t.sum() > 200 and (first["var"][t] == np.minimum(first["r"][t], 1.0)).all()
    sc = out["scan"]
    assert out["known"].any() and not out["known"].all()
    assert (out["est_var"][~out["known"]] == 1.0).all() and (out["est_var"][out["known"]] < 1e-3).all()


def test_flat_ground_under_range_noise():
    """flat ground, relative Gaussian range noise of 2 %, one pose, 30 ticks, fixed seed: the variance map's RMSE is below that of the maximum map with
    alpha = 1 and with alpha = 0.5 (the maximum of a cell's noisy pixels is biased upwards and alpha does not average it away), and the variance falls at
    every tick in the cells whose measurement passed the gate at every tick - nine in ten of the cells touched at every tick at least"""
    qpos = np.array([0.013, -0.021, 0.3, 1.0, 0.0, 0.0, 0.0])
    clean = image(qpos, CAM, dtype=np.float64)
    rng = np.random.default_rng(3)
    sigma, T = 0.02, 30
    var = vref.settings(dict(sigma0=0.002, sigma_rel=sigma, process=0.0))
    sv, s1, s5 = vref.new_state(G), ref.new_state(G), ref.new_state(G)
    always, passed, falling, last_v = None, None, None, None
    for t in range(T):
        img = np.where(clean < CAM["far"], clean * (1 + sigma * rng.standard_normal(clean.shape)), clean).astype(np.float32)
        ov = vref.tick(sv, qpos, img, CAM, var, clear=t == 0)
        o1 = ref.tick(s1, qpos, img, CAM, clear=t == 0)
        o5 = ref.tick(s5, qpos, img, dict(CAM, alpha=0.5), clear=t == 0)
        sv, s1, s5 = (ov["map"], ov["var"], ov["origin"]), (o1["map"], o1["origin"]), (o5["map"], o5["origin"])
        if t == 0:
            always, passed, falling = ov["touched"].copy(), np.ones((G, G), bool), np.ones((G, G), bool)
        else:
            always &= ov["touched"]
            passed &= ov["branch"] == 2
            with np.errstate(invalid="ignore"):
                falling &= ov["var"] < last_v
        last_v = ov["var"].copy()
    assert always.sum() > 100
    rmse = lambda m: float(np.sqrt(np.mean(m[always] ** 2)))                       # the truth is z = 0
    rv, r1, r5 = rmse(ov["map"]), rmse(o1["map"]), rmse(o5["map"])
    print(f"flat ground, sigma {sigma}: RMSE variance {rv:.4f}, maximum alpha=1 {r1:.4f}, alpha=0.5 {r5:.4f} m over {always.sum()} cells; "
          f"{(always & passed).sum()} of them passed the gate at every tick")
    assert rv < r1 and rv < r5
    assert falling[always & passed].all() and (always & passed).sum() >= 0.9 * always.sum()


def _one_point(z):
    return np.array([[0.1, 0.1, z]], np.float32)


def test_the_gate():
    """a higher outlier replaces the cell; a lower one is ignored while process = 0, and with process > 0 it is accepted at the first tick at which
    (m - h)^2 <= gate^2 (v + r): the tick the growth of v by `process` per tick implies"""
    qpos = np.array([0.02, 0.02, 0.3, 1.0, 0.0, 0.0, 0.0])
    Gs = 8
    c = tuple(ref.cell(np.array([0.1, 0.1]), 0.04) % Gs)
    var = vref.settings(dict(process=0.0))
    a = vref.tick(vref.new_state(Gs), qpos, _one_point(0.0), PTS, var, clear=True, points=True)
    assert a["branch"][c] == 1 and a["map"][c] == 0.0 and a["touched"].sum() == 1
    st = (a["map"], a["var"], a["origin"])
    up = vref.tick(st, qpos, _one_point(0.5), PTS, var, points=True)
    assert up["branch"][c] == 3 and up["map"][c] == 0.5 and up["var"][c] == up["r"][c]
    for _ in range(20):
        lo = vref.tick(st, qpos, _one_point(-0.1), PTS, var, points=True)
        assert lo["branch"][c] == 4 and lo["map"][c] == 0.0 and lo["var"][c] == a["var"][c]
        st = (lo["map"], lo["var"], lo["origin"])
    # process > 0: v grows by `process` per tick (the predict comes before the test) until the gate opens
    process, gate = 1e-4, 3.0
    var = vref.settings(dict(process=process, gate=gate))
    v0, r = a["var"][c], lo["r"][c]
    p32 = float(np.float32(process))
    want = int(np.ceil(((0.1 ** 2) / gate ** 2 - r - v0) / p32))
    assert 5 < want < 20
    st = (a["map"], a["var"], a["origin"])
    for t in range(1, want + 1):
        lo = vref.tick(st, qpos, _one_point(-0.1), PTS, var, points=True)
        assert lo["branch"][c] == (2 if t == want else 4), (t, want)
        st = (lo["map"], lo["var"], lo["origin"])
    assert -0.1 < lo["map"][c] < 0.0 and lo["var"][c] < r


def _edge_scene():
    """a camera 1 m above the ground looking straight down over the edge x = 0.02 of a box whose top is at z = 0.2: the riser is seen edge-on, so the
    cells [0, 0.04) x ... straddle the edge with pixels of the top and of the ground"""
    box = dict(c=np.array([-0.48, 0.0, 0.1]), A=np.eye(3), h=np.array([0.5, 1.0, 0.1]))
    qpos = np.array([0.02, 0.02, 1.0, 1.0, 0.0, 0.0, 0.0])
    return qpos, image(qpos, DOWN, [box], w=96, h=72)


def test_the_band():
    """a cell that straddles a box edge holds the upper face's height to within the image's fp32 error; with a band that covers the riser it holds
    the mixture of the two faces (the band is 0.25 m over a riser of 0.2 m: on the riser's own height the image's rounding would decide)"""
    qpos, img = _edge_scene()
    thin = vref.tick(vref.new_state(G), qpos, img, DOWN, vref.settings(), clear=True)
    wide = vref.tick(vref.new_state(G), qpos, img, DOWN, vref.settings(dict(band=0.25)), clear=True)
    wc = ref.world_cells(thin["origin"], G)
    straddle = thin["touched"] & (wc[..., 0] == 0) & (thin["excluded"] > 0)
    assert straddle.sum() >= 5 and (thin["n"][straddle] >= 1).all()
    assert np.abs(thin["map"][straddle] - 0.2).max() <= 2e-6
    assert (wide["excluded"][straddle] == 0).all() and (wide["n"][straddle] == thin["n"][straddle] + thin["excluded"][straddle]).all()
    share = thin["n"][straddle] / wide["n"][straddle]                               # the top's share of the cell's pixels
    assert np.abs(wide["map"][straddle] - 0.2 * share).max() <= 2e-6 + 2.0 ** -18
    assert ((wide["map"][straddle] > 0.01) & (wide["map"][straddle] < 0.19)).all()
    # away from the edge both hold the face they see
    top, ground = thin["touched"] & (wc[..., 0] < -1), thin["touched"] & (wc[..., 0] > 1)
    assert top.sum() > 50 and ground.sum() > 50 and np.abs(wide["map"][top] - 0.2).max() <= 2e-6 and np.abs(wide["map"][ground]).max() <= 2e-6


def _cloud(rng, P=600):
    pts = np.empty((P, 3), np.float32)
    pts[:, :2] = rng.uniform(-0.5, 0.5, (P, 2))
    pts[:, 2] = 0.02 * rng.standard_normal(P)
    pts[::17] = np.nan
    return pts


def test_permuted_points_give_identical_outputs():
    rng = np.random.default_rng(8)
    qpos = np.array([0.02, 0.02, 0.3, 0.98, 0.02, -0.03, 0.2])
    Gs, var = 24, vref.settings(dict(process=1e-4))
    sa = sb = vref.new_state(Gs)
    for t in range(3):
        pts = _cloud(rng)
        a = vref.tick(sa, qpos, pts, PTS, var, clear=t == 0, points=True)
        b = vref.tick(sb, qpos, pts[rng.permutation(len(pts))], PTS, var, clear=t == 0, points=True)
        for k in ("map", "var", "est", "est_var", "known", "n", "S", "branch"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, t)
        sa, sb = (a["map"], a["var"], a["origin"]), (b["map"], b["var"], b["origin"])
    assert (a["n"] >= 2).sum() > 50 and (a["excluded"] > 0).sum() > 20 and set(np.unique(a["branch"])) >= {0, 2}


def test_max_count_caps_the_variance_reduction():
    rng = np.random.default_rng(9)
    qpos = np.array([0.02, 0.02, 0.3, 1.0, 0.0, 0.0, 0.0])
    pts = _cloud(rng, 3000)
    pts[:, 2] = 0.0                                                                 # every point of a cell is in the band: n is the cell's count
    outs = {mc: vref.tick(vref.new_state(24), qpos, pts, PTS, vref.settings(dict(max_count=mc)), clear=True, points=True) for mc in (1, 4, 1000)}
    t = outs[1]["touched"]
    n = outs[1]["n"][t]
    assert (n >= 5).sum() > 50 and (n < 4).sum() >= 1
    base = outs[1]["var"][t]                                                        # r of one pixel
    assert np.allclose(outs[4]["var"][t], base / np.minimum(n, 4), rtol=1e-12) and np.allclose(outs[1000]["var"][t], base / n, rtol=1e-12)
    assert np.array_equal(outs[1]["map"], outs[4]["map"], equal_nan=True)


# ---------------------------------------------------------------- the host side
def test_joystick_and_map_refusals():
    """before anything touches a device"""
    from phase_guided_terrain_traversal_amd.env import Joystick
    with pytest.raises(ValueError, match="not built yet"):
        Joystick("stairs", configs.training_config(), num_envs=4, depth=dict(every=2), elevation=dict(variance=True, follow_sensor=True))
    with pytest.raises(ValueError, match="True or a dict"):
        Joystick("stairs", configs.training_config(), num_envs=4, depth={}, elevation=dict(variance=3))
    with pytest.raises(ValueError, match="needs depth"):
        Joystick("stairs", configs.training_config(), num_envs=4, elevation=dict(variance=True))
    env = types.SimpleNamespace()
    with pytest.raises(ValueError, match="not built yet"):
        elevation.ElevationMap(env, variance=True, follow_sensor=True)
    with pytest.raises(ValueError, match="grid <= 64"):
        elevation.ElevationMap(env, grid=96, variance=True)
    with pytest.raises(ValueError, match="unknown setting"):
        elevation.ElevationMap(env, variance=dict(sigma=0.01))


def test_struct_layout_without_the_library():
    assert C.sizeof(elevation.PgttElevationVar) == 48
    v = elevation.variance_struct(**elevation.VARIANCE_DEFAULTS)
    assert v.max_count == 4 and v.var is None and abs(v.band - 0.03) < 1e-8


needs_lib = pytest.mark.skipif(not os.path.exists(elevation.LIB_PATH), reason="libpgtt_elevation.so not built (run __graft_entry__.build())")


@needs_lib
def test_check_var_refuses():
    L = elevation.lib()
    good = elevation.VARIANCE_DEFAULTS
    assert L.pgtt_elevation_check_var(C.byref(elevation.variance_struct(**good))) == 0
    for kw in (dict(sigma0=0.0), dict(sigma_rel=0.0), dict(process=0.0), dict(band=0.0), dict(band=0.5), dict(max_count=1), dict(gate=0.1)):
        assert L.pgtt_elevation_check_var(C.byref(elevation.variance_struct(**dict(good, **kw)))) == 0, kw
    nan, inf = float("nan"), float("inf")
    bad = {"sigma0_negative": dict(sigma0=-0.001), "sigma_rel_negative": dict(sigma_rel=-0.01), "both_sigmas_zero": dict(sigma0=0.0, sigma_rel=0.0),
           "process_negative": dict(process=-1e-6), "gate_0": dict(gate=0.0), "gate_negative": dict(gate=-3.0), "band_negative": dict(band=-0.01),
           "band_above_max": dict(band=0.51), "max_count_0": dict(max_count=0), "var_max_0": dict(var_max=0.0), "var_max_negative": dict(var_max=-1.0),
           "sigma0_nan": dict(sigma0=nan), "process_nan": dict(process=nan), "gate_inf": dict(gate=inf), "band_nan": dict(band=nan),
           "var_max_inf": dict(var_max=inf), "sigma_rel_inf": dict(sigma_rel=inf)}
    for name, kw in bad.items():
        assert L.pgtt_elevation_check_var(C.byref(elevation.variance_struct(**dict(good, **kw)))) == -1, name
        assert L.pgtt_elevation_last_error(), name
    assert L.pgtt_elevation_check_var(None) == -1


@needs_lib
def test_sizeof_var_and_exports():
    L = elevation.lib()
    assert L.pgtt_elevation_sizeof_var() == C.sizeof(elevation.PgttElevationVar)
    for name in ("pgtt_elevation_check_var", "pgtt_elevation_bind_var", "pgtt_elevation_var", "pgtt_elevation_var_points", "pgtt_elevation_sizeof_var"):
        assert name in elevation.EXPORTS and hasattr(L, name)
    # NULL arguments are refused before anything is launched
    assert L.pgtt_elevation_bind_var(None, C.byref(elevation.variance_struct())) == -1
    assert L.pgtt_elevation_var(None, None, 0, 0, None) == -1 and L.pgtt_elevation_var_points(None, None, 0, 0, None) == -1
