"""The depth-fused elevation map without a GPU: facts that hold tests/elevation_reference.py (the fp64 statement of include/pgtt_elevation.h that
the GPU tests compare the kernel with) on its own, and the host side of libpgtt_elevation.so - the config's refusals, the struct sizes, the source
hash (its file list: tests/test_abi.py), and the refusals of Joystick(elevation=...) that come before anything touches a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_reference as dref  # noqa: E402
import elevation_reference as ref  # noqa: E402

from phase_guided_terrain_traversal_amd import configs, elevation, srchash  # noqa: E402

CAM = dict(fovy=58.0, near=0.1, far=3.0, mount_pos=(0.0, 0.0, 0.0), mount_quat=dref.pitch_quat(30.0).astype(np.float32).astype(float), res=0.04, alpha=1.0, self_half=(0.0, 0.0, 0.0))
W, H = 64, 48                                  # CAM's numbers are what a device would see (fp32 values): the image and the map use ONE camera


def image(qpos, cfg, boxes=(), dtype=np.float32):
    """the noise-free image of the plane z = 0 and `boxes` from the camera of `cfg` on a base at `qpos` (depth_reference's ray caster)"""
    cam = ref.camera_pose(qpos, cfg["mount_pos"], cfg["mount_quat"])
    return dref.depth_image(cam, cfg["fovy"], W, H, cfg["near"], cfg["far"], boxes)["depth"].astype(dtype)


def by_world_cell(out, G):
    """{(ix, iy): height} of the non-NaN cells"""
    wc = ref.world_cells(out["origin"], G)
    keep = ~np.isnan(out["map"])
    return {tuple(c): h for c, h in zip(wc[keep], out["map"][keep])}


def test_flat_ground():
    """a level base 0.3 m above the plane z = 0, the camera pitched 30 degrees down: every touched cell holds 0, none lies behind the camera"""
    G = 64
    qpos = np.array([0.013, -0.021, 0.3, 1.0, 0.0, 0.0, 0.0])
    out = ref.tick(ref.new_state(G), qpos, image(qpos, CAM, dtype=np.float64), CAM)
    assert out["touched"].sum() > 100 and np.array_equal(out["touched"], ~np.isnan(out["map"]))
    assert np.abs(out["map"][out["touched"]]).max() <= 1e-9
    wc = ref.world_cells(out["origin"], G)[out["touched"]]
    assert ((wc[:, 0] + 1) * CAM["res"] > qpos[0]).all()                       # the cell's far edge is ahead of the camera
    assert tuple(out["origin"]) == (0, -1)


def box_top_scene():
    box = dict(c=np.array([1.0, 0.0, 0.1]), A=np.eye(3), h=np.array([0.3, 0.4, 0.1]))      # top at z = 0.2 over [0.7, 1.3] x [-0.4, 0.4]
    return [box]


def test_window_shift():
    """cells entirely inside the visible top of a box hold 0.2; a shift of the base by k cells leaves the map unchanged when indexed by world cell;
    a shift by G cells or more leaves only the new tick's cells"""
    G, res = 64, CAM["res"]
    boxes = box_top_scene()
    q0 = np.array([0.0, 0.0, 0.45, 1.0, 0.0, 0.0, 0.0])
    a = ref.tick(ref.new_state(G), q0, image(q0, CAM, boxes), CAM)
    cells = by_world_cell(a, G)
    inner = [(ix, iy) for (ix, iy) in cells if 0.7 <= ix * res and (ix + 1) * res <= 1.3 and -0.4 <= iy * res and (iy + 1) * res <= 0.4]
    assert len(inner) > 50 and all(abs(cells[c] - 0.2) <= 1e-6 for c in inner)          # 1e-6: the image is fp32
    # a second tick k cells further with an image that adds nothing (all far): the same world cells, minus those that left the window
    for k in (1, 5, 31):
        q1 = q0 + np.array([k * res, 0, 0, 0, 0, 0, 0])
        b = ref.tick((a["map"], a["origin"]), q1, np.full((H, W), 3.0, np.float32), CAM)
        assert tuple(b["origin"]) == (k, 0) and not b["touched"].any()
        lo = b["origin"][0] - G // 2
        want = {c: h for c, h in cells.items() if lo <= c[0] < lo + G}
        assert by_world_cell(b, G) == want and len(want) > 0
    # a jump of G cells and of G + 7: nothing of the old map survives, whatever the slots alias to
    for k in (G, G + 7, -3 * G):
        q1 = q0 + np.array([k * res, 0, 0, 0, 0, 0, 0])
        img = image(q1, CAM, boxes)
        b = ref.tick((a["map"], a["origin"]), q1, img, CAM)
        fresh = ref.tick(ref.new_state(G), q1, img, CAM, clear=True)
        assert np.array_equal(np.isnan(b["map"]), np.isnan(fresh["map"])) and np.array_equal(b["map"][b["touched"]], fresh["map"][fresh["touched"]])
        assert np.array_equal(b["touched"], ~np.isnan(b["map"]))


def test_negative_coordinates():
    """bases at x = -0.01 and x = +0.01 put the same world point into the same world cell (floor, not truncation)"""
    G = 24
    got = []
    for bx in (-0.01, 0.01):
        qpos = np.array([bx, -0.3, 0.3, 1.0, 0.0, 0.0, 0.0])
        out = ref.tick(ref.new_state(G), qpos, image(qpos, CAM), CAM)
        assert out["origin"][0] == (-1 if bx < 0 else 0) and out["origin"][1] == -8
        got.append(out)
    assert tuple(ref.cell(np.array([-0.01, 0.01]), 0.04)) == (-1, 0)
    # the world point (0.3, -0.3) - and every other - lands in the same world cell from both bases
    a, b = by_world_cell(got[0], G), by_world_cell(got[1], G)
    c = tuple(ref.cell(np.array([0.3, -0.3]), float(np.float32(0.04))))
    assert c in a and c in b and c == (7, -8)
    common = set(a) & set(b)
    assert len(common) > 20 and all(abs(a[k] - b[k]) <= 1e-6 for k in common)
    # slots: floor-mod
    wc = ref.world_cells(got[0]["origin"], G)
    s = np.arange(G)
    assert np.array_equal(wc[:, 0, 0] % G, s) and np.array_equal(wc[0, :, 1] % G, s) and wc[..., 0].min() == -1 - G // 2


def test_scan_offset_invariance():
    G = 64
    qpos = np.array([0.2, 0.1, 0.45, 0.98, 0.02, -0.03, 0.2])
    a = ref.tick(ref.new_state(G), qpos, image(qpos, CAM, box_top_scene()), CAM)
    s0 = ref.sample(a["map"], a["origin"], qpos, CAM)
    s1 = ref.sample(a["map"] + 7.5, a["origin"], qpos, CAM)
    assert s0["known"].any() and not s0["known"].all() and np.array_equal(s0["known"], s1["known"])
    assert np.abs(s0["est"] - s1["est"]).max() <= 1e-12 and s0["est"].min() == 0.0 and s0["est"].max() > 0.15
    # unknown points take the minimum of the known ones: est is 0 there
    assert (s0["est"][~s0["known"]] == 0).all() and (s0["z"][~s0["known"]] == s0["z"][s0["known"]].min()).all()
    empty = ref.sample(ref.new_state(G)[0], a["origin"], qpos, CAM)
    assert not empty["known"].any() and (empty["est"] == 0).all()
    # the grid is the observe kernel's: point 0 is 0.6 m ahead and 0.4 m to the left of the base, the centre point is the base
    xy = ref.scan_points(np.array([1.0, 2.0, 0.3, 1.0, 0.0, 0.0, 0.0]))
    assert np.allclose(xy[0], (1.6, 2.4)) and np.allclose(xy[58], (1.0, 2.0)) and np.allclose(xy[116], (0.4, 1.6))
    # obs_out
    obs = np.arange(171.0)
    o = ref.tick(ref.new_state(G), qpos, image(qpos, CAM), CAM, obs=obs)["obs_out"]
    assert np.array_equal(o[:38], obs[:38]) and np.array_equal(o[155:], obs[155:]) and o.shape == (171,)


def test_self_filter():
    """points inside the box around the base are dropped; self_half = 0 keeps them"""
    G = 64
    qpos = np.array([0.0, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0])
    img = image(qpos, CAM)
    keep = ref.tick(ref.new_state(G), qpos, img, CAM)
    cut = ref.tick(ref.new_state(G), qpos, img, dict(CAM, self_half=(0.45, 0.25, 0.45)))
    assert keep["kept"].sum() == keep["valid"].sum() and np.isinf(keep["self_margin"]).all()
    inside = (np.abs(keep["point"][:, 0]) <= 0.45) & (np.abs(keep["point"][:, 1]) <= 0.25) & (np.abs(keep["point"][:, 2] - 0.3) <= 0.45)
    assert (inside & keep["valid"]).sum() > 10
    assert np.array_equal(cut["kept"], keep["valid"] & ~inside)
    dropped = {tuple(c) for c in keep["cell"][keep["valid"] & inside]} - {tuple(c) for c in keep["cell"][cut["kept"]]}
    assert dropped and all(c not in by_world_cell(cut, G) for c in dropped) and all(c in by_world_cell(keep, G) for c in dropped)
    assert (cut["self_margin"][keep["valid"]] >= 0).all() and np.isfinite(cut["self_margin"]).all()


def test_alpha_fuses():
    G = 24
    qpos = np.array([0.0, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0])
    img = image(qpos, CAM)
    cfg = dict(CAM, alpha=0.5)
    old = np.full((G, G), 1.0)
    out = ref.tick((old, ref.cell(qpos[:2], 0.04)), qpos, img, cfg)
    assert np.allclose(out["map"][out["touched"]], 0.5, atol=1e-9) and (out["map"][~out["touched"]] == 1.0).all()


# ---------------------------------------------------------------- the host side of the library
def test_joystick_refusals():
    """before anything touches a device"""
    from phase_guided_terrain_traversal_amd.env import Joystick
    with pytest.raises(ValueError, match="needs depth"):
        Joystick("stairs", configs.training_config(), num_envs=4, elevation=True)
    with pytest.raises(ValueError, match="every=1"):
        Joystick("stairs", configs.training_config(), num_envs=4, depth=dict(every=2), elevation=dict(grid=24))
    with pytest.raises(ValueError, match="torso"):
        Joystick("stairs", configs.training_config(), num_envs=4, depth=dict(mount_body=1), elevation=True)


def test_struct_layout_without_the_library():
    assert C.sizeof(elevation.PgttElevationConfig) == 92 and C.sizeof(elevation.PgttElevationBuffers) == 72
    assert elevation.settings(True) == elevation.DEFAULTS and elevation.settings(dict(grid=24))["grid"] == 24
    assert set(elevation.DEFAULTS) == {"grid", "res", "alpha", "self_half"}


needs_lib = pytest.mark.skipif(not os.path.exists(elevation.LIB_PATH), reason="libpgtt_elevation.so not built (run __graft_entry__.build())")
GOOD = dict(width=64, height=48, fovy=58.0, near=0.1, far=3.0, mount_pos=(0.3, 0.0, 0.05), mount_quat=(0.97, 0.0, 0.26, 0.0), grid=64, res=0.04, alpha=1.0,
            self_half=(0.45, 0.25, 0.45), obs_dim=171, scan_row0=38)


@needs_lib
def test_check_refuses():
    L = elevation.lib()
    assert L.pgtt_elevation_check(C.byref(elevation.config_struct(**GOOD))) == 0
    for g in (8, 9, 96):
        assert L.pgtt_elevation_check(C.byref(elevation.config_struct(**dict(GOOD, grid=g)))) == 0, g
    assert L.pgtt_elevation_check(C.byref(elevation.config_struct(**dict(GOOD, obs_dim=162, scan_row0=30)))) == 0
    bad = {"grid_7": dict(grid=7), "grid_97": dict(grid=97), "res_0": dict(res=0.0), "res_negative": dict(res=-0.04), "res_nan": dict(res=float("nan")),
           "alpha_0": dict(alpha=0.0), "alpha_1.5": dict(alpha=1.5), "near_ge_far": dict(near=3.0, far=3.0), "near_gt_far": dict(near=4.0),
           "scan_rows_past_obs": dict(scan_row0=55), "obs_shorter_than_the_scan_rows": dict(obs_dim=154), "mount_body": dict(mount_body=1),
           "zero_quat": dict(mount_quat=(0, 0, 0, 0)), "fovy": dict(fovy=180.0), "width": dict(width=257), "self_half": dict(self_half=(0.1, -0.1, 0.1))}
    for name, kw in bad.items():
        assert L.pgtt_elevation_check(C.byref(elevation.config_struct(**dict(GOOD, **kw)))) == -1, name
        assert L.pgtt_elevation_last_error(), name
    assert L.pgtt_elevation_check(None) == -1


@needs_lib
def test_sizeof_exports_and_build_info():
    L = elevation.lib()
    assert L.pgtt_elevation_sizeof_config() == C.sizeof(elevation.PgttElevationConfig)
    assert L.pgtt_elevation_sizeof_buffers() == C.sizeof(elevation.PgttElevationBuffers)
    info = elevation.build_info()
    assert info["src"] == srchash.side_sha256("elevation") and info["flavor"] == "product"
    for name in elevation.EXPORTS:
        getattr(L, name)

