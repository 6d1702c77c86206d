"""The point-fed elevation map without a GPU: tests/elevation_points_reference.py (the fp64 statement of pgtt_elevation_points that the GPU tests
compare the kernel with) against tests/elevation_reference.py fed the same geometry, and on its own: a NaN point is skipped, the self filter,
clear and recentre behave as they do for the image."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_points_reference as pref  # noqa: E402
import elevation_reference as ref  # noqa: E402
from test_elevation import CAM, box_top_scene, by_world_cell, image  # noqa: E402

KEYS = ("map", "origin", "est", "known", "touched")


def same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


def cloud(out):
    """the reference's own unprojected, valid pixels as a point cloud: NaN rows where a pixel had no return"""
    return np.where(out["valid"][:, None], out["point"], np.nan)


def test_equals_the_image_reference_on_its_own_points():
    """three ticks of a moving base, with and without the self filter, alpha = 1 and 0.5: the same maps, origins, scans and touched cells, bit
    for bit in fp64"""
    G = 64
    boxes = box_top_scene()
    poses = [np.array([0.2, 0.1, 0.45, 0.98, 0.02, -0.03, 0.2]), np.array([0.41, 0.1, 0.45, 0.98, 0.02, -0.03, 0.25]), np.array([-0.3, 0.9, 0.4, 1.0, 0.0, 0.0, 0.0])]
    for cfg in (CAM, dict(CAM, self_half=(0.45, 0.25, 0.45)), dict(CAM, alpha=0.5)):
        a, b = ref.new_state(G), pref.new_state(G)
        obs = np.arange(171.0)
        for t, q in enumerate(poses):
            wa = ref.tick(a, q, image(q, cfg, boxes), cfg, clear=t == 0, obs=obs)
            wb = pref.tick(b, q, cloud(wa), cfg, clear=t == 0, obs=obs)
            same(wa, wb)
            assert np.array_equal(wa["obs_out"], wb["obs_out"]) and np.array_equal(wa["kept"], wb["kept"]) and wa["touched"].sum() > 50
            assert np.array_equal(wa["margin"][wa["valid"]], wb["margin"][wb["valid"]])
            assert np.array_equal(wa["self_margin"][wa["valid"]], wb["self_margin"][wb["valid"]])
            assert ref.doubtful_cells(wa, cfg["res"], 2e-5) == pref.doubtful_cells(wb, cfg["res"], 2e-5)
            a, b = (wa["map"], wa["origin"]), (wb["map"], wb["origin"])


def test_nan_and_non_finite_points_are_skipped():
    G = 24
    q = np.array([0.0, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0])
    pts = np.array([[0.1, 0.1, 0.25], [np.nan, 0.1, 9.0], [0.1, np.nan, 9.0], [0.1, 0.1, np.nan], [np.inf, 0.1, 9.0], [0.1, 0.1, -np.inf], [0.1, 0.1, np.inf],
                    [np.nan, np.nan, np.nan], [-0.21, 0.3, 0.5], [0.1, 0.1, 0.2]])
    out = pref.tick(pref.new_state(G), q, pts, CAM)
    assert list(out["valid"]) == [True] + [False] * 7 + [True, True]
    assert by_world_cell(out, G) == {(2, 2): 0.25, (-6, 7): 0.5}                     # the maximum of the cell's two points; nothing of the bad rows
    empty = pref.tick(pref.new_state(G), q, np.full((16, 3), np.nan), CAM)
    assert not empty["touched"].any() and np.isnan(empty["map"]).all() and not empty["known"].any() and (empty["est"] == 0).all()
    far_away = pref.tick(pref.new_state(G), q, np.array([[5.0, 0.0, 1.0], [0.0, -0.49, 1.0], [0.0, 0.47, 1.0]]), CAM)
    assert by_world_cell(far_away, G) == {(0, 11): 1.0}                              # the window is [-12, 12) cells: y = -0.49 is cell -13


def test_self_filter_on_points():
    G = 24
    q = np.array([0.0, 0.0, 0.3, np.cos(0.4), 0.0, 0.0, np.sin(0.4)])               # yawed by 0.8 rad: the box turns with the base
    c, s = np.cos(0.8), np.sin(0.8)
    inside, outside = np.array([0.4 * c, 0.4 * s, 0.3]), np.array([-0.4 * s, 0.4 * c, 0.3])      # 0.4 m ahead (|x| <= 0.45), 0.4 m to the left (|y| > 0.25)
    cfg = dict(CAM, self_half=(0.45, 0.25, 0.45))
    out = pref.tick(pref.new_state(G), q, np.stack([inside, outside]), cfg)
    assert list(out["kept"]) == [False, True] and out["touched"].sum() == 1
    assert np.allclose(out["self_margin"], [0.05, 0.15])
    assert pref.tick(pref.new_state(G), q, np.stack([inside, outside]), CAM)["touched"].sum() == 2


def test_clear_and_recentre():
    G, res = 24, CAM["res"]
    q0 = np.array([0.01, 0.01, 0.3, 1.0, 0.0, 0.0, 0.0])
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.uniform(-0.45, 0.45, (200, 2)), rng.uniform(0, 0.3, (200, 1))], 1)
    a = pref.tick(pref.new_state(G), q0, pts, CAM)
    cells = by_world_cell(a, G)
    assert len(cells) > 100
    nothing = np.full((4, 3), np.nan)
    for k in (1, 5, 11):                                                         # the same world cells, minus those that left the window
        q1 = q0 + np.array([k * res, 0, 0, 0, 0, 0, 0])
        b = pref.tick((a["map"], a["origin"]), q1, nothing, CAM)
        lo = b["origin"][0] - G // 2
        assert tuple(b["origin"]) == (k, 0) and by_world_cell(b, G) == {c: h for c, h in cells.items() if lo <= c[0] < lo + G}
    for k in (G, G + 7, -3 * G):                                                 # a jump of G cells or more: nothing survives
        q1 = q0 + np.array([k * res, 0, 0, 0, 0, 0, 0])
        assert not by_world_cell(pref.tick((a["map"], a["origin"]), q1, nothing, CAM), G)
    cleared = pref.tick((a["map"], a["origin"]), q0, pts[:10], CAM, clear=True)
    assert np.array_equal(cleared["touched"], ~np.isnan(cleared["map"])) and cleared["touched"].sum() <= 10
    kept = pref.tick((a["map"], a["origin"]), q0, pts[:10], CAM)
    assert by_world_cell(kept, G).keys() == cells.keys()
    # alpha fuses as for the image
    old = np.full((G, G), 1.0)
    out = pref.tick((old, ref.cell(q0[:2], res)), q0, pts * np.array([1, 1, 0]), dict(CAM, alpha=0.5))
    assert np.allclose(out["map"][out["touched"]], 0.5, atol=1e-9) and (out["map"][~out["touched"]] == 1.0).all()
