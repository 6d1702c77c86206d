"""The fp64 reference of the map call (tests/render_map_reference.py) held to facts it does not compute itself - an analytic single column, one
terrain box cast by test_gpu_render's caster, the elevation reference's slot mapping - and the host side of Renderer.render_map: the ctypes
mirror and the refusals that come before any library call.  No GPU."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_reference as eref  # noqa: E402
import render_map_reference as R  # noqa: E402
import test_gpu_render as tgr  # noqa: E402

from phase_guided_terrain_traversal_amd import render  # noqa: E402

def _scene(hwin, origin=(0, 0), res=0.1, floor_z=-0.1, lift=0.0, twin=None, tint=(0.0, 1.0), boxes=None):
    hwin = np.asarray(hwin, np.float32)
    G = hwin.shape[0]
    return dict(grid=G, res=res, lo=R.window_lo(origin, G), hwin=hwin, twin=twin, floor_z=floor_z, lift=lift, tint_lo=tint[0], tint_hi=tint[1],
                geoms=[], markers=(), boxes=boxes, shadows=False)


def _ray(o, to):
    d = np.asarray(to, float) - np.asarray(o, float)
    return np.asarray(o, float), (d / np.linalg.norm(d))[None]


def test_single_column_analytic_distance_and_face():
    """the column [0, 0.125]^2 x [-0.125, 0.25] (G = 1, origin 0; every number a binary fraction): from above, from each side and from
    below the floor"""
    sc = _scene([[0.25]], res=0.125, floor_z=-0.125)
    c = 0.0625
    for o, to, t_true, n_true in (
            ((c, c, 1.25), (c, c, 0.0), 1.0, (0, 0, 1)),                              # straight down on the top
            ((0.02, 0.07, 0.9), (0.02, 0.07, 0.0), 0.65, (0, 0, 1)),
            ((-0.5, c, 0.1), (0.5, c, 0.1), 0.5, (-1, 0, 0)),                         # the four walls, level rays
            ((0.625, c, 0.1), (-0.5, c, 0.1), 0.5, (1, 0, 0)),
            ((c, -0.4, 0.1), (c, 0.5, 0.1), 0.4, (0, -1, 0)),
            ((c, 0.725, 0.1), (c, -0.5, 0.1), 0.6, (0, 1, 0)),
            ((c, c, -0.625), (c, c, 0.0), 0.5, (0, 0, -1))):                          # from below the floor, looking up: the bottom face
        oo, d = _ray(o, to)
        r = R.cast_map(oo, d, sc)
        assert r["id"][0] == R.SEG_CELL and abs(r["t"][0] - t_true) < 1e-12, (o, r["t"])
        assert np.allclose(r["n"][0], n_true), (o, r["n"])
    # a slanted ray onto the top: t = (z0 - top) / |d.z|, landing inside the cell
    oo, d = _ray((0.3, 0.25, 0.8), (c, c, 0.25))
    r = R.cast_map(oo, d, sc)
    assert abs(r["t"][0] - 0.55 / abs(d[0, 2])) < 1e-12 and np.allclose(r["n"][0], (0, 0, 1))
    # beside the column: sky
    oo, d = _ray((0.25, 0.05, 1.0), (0.25, 0.05, 0.0))
    r = R.cast_map(oo, d, sc)
    assert r["id"][0] == render.SEG_SKY and np.isinf(r["t"][0])


def test_flat_map_is_one_terrain_box():
    """all cells at one height: away from nothing but exact cell borders the columns are ONE box of the window's extent, cast by the existing
    fp64 caster (floor_z = 0, so the caster's plane lies under the box and is never nearer)"""
    G, res, origin, h = 12, 0.05, (-7, 5), float(np.float32(0.23))
    sc = _scene(np.full((G, G), h), origin=origin, res=res, floor_z=0.0)
    lo = sc["lo"]
    r32 = float(np.float32(res))
    c = np.array([(lo[0] + G / 2) * r32, (lo[1] + G / 2) * r32, h / 2])
    box = dict(c=c, A=np.eye(3), h=np.array([G * r32 / 2, G * r32 / 2, h / 2]))
    hits = tops = walls = 0
    for az, el in ((30.0, -40.0), (200.0, -15.0), (117.0, -75.0)):
        cam = render.Camera("fixed", target=(c[0] + 0.013, c[1] + 0.007, h), distance=0.8, azimuth=az, elevation=el, fovy=70.0)
        o, d = render.camera_rays(cam, 41, 31)
        d = d.reshape(-1, 3)
        a = R.cast_map(o, d, sc)
        b = tgr.cast(o, d, [box], [], shadows=False)
        on_box = b["id"] == render.SEG_BOX
        assert np.array_equal(a["id"] >= R.SEG_CELL, on_box)
        assert np.abs(a["t"][on_box] / b["t"][on_box] - 1).max() < 1e-12
        nb = tgr._hit_box(o, d, box["c"], box["A"], box["h"])[1]
        nb = np.where((np.sum(nb * d, -1) > 0)[:, None], -nb, nb)
        assert np.array_equal(a["n"][on_box], nb[on_box])
        hits += on_box.sum()
        tops, walls = tops + (np.abs(a["n"][on_box][:, 2]) == 1).sum(), walls + (a["n"][on_box][:, 2] == 0).sum()
    assert hits > 500 and tops > 100 and walls > 100


@pytest.mark.parametrize("G,origin", [(8, (3, -2)), (9, (-40, -40)), (24, (-13, 7)), (5, (-1, 0)), (96, (-130, 70)), (7, (-3, 11))])
def test_slot_mapping_is_the_elevation_reference_s(G, origin):
    wc = eref.world_cells(origin, G)                                   # the world cell each SLOT holds
    lo = R.window_lo(origin, G)
    win = np.arange(G * G, dtype=np.float32).reshape(G, G)            # window cell (a, b) holds a G + b
    slots = R.to_slots(win, origin)
    a, b = wc[..., 0] - lo[0], wc[..., 1] - lo[1]
    assert ((0 <= a) & (a < G) & (0 <= b) & (b < G)).all()
    assert np.array_equal(slots, (a * G + b).astype(np.float32))
    assert np.array_equal(R.to_window(slots, origin), win)
    # an origin outside +-2^30 is taken as +-2^30
    assert np.array_equal(R.window_lo((2 ** 31 - 1, -2 ** 31), G), np.array([2 ** 30, -2 ** 30]) - G // 2)


def test_floor_nan_and_lift():
    h = np.array([[0.2, np.nan], [-0.3, 0.1]], np.float32)
    sc = _scene(h, res=0.1, floor_z=-0.1)
    down = lambda x, y: _ray((x, y, 1.0), (x, y, -5.0))                 # noqa: E731
    lo = sc["lo"] * 0.1
    centre = lambda a, b: (lo[0] + (a + 0.5) * float(np.float32(0.1)), lo[1] + (b + 0.5) * float(np.float32(0.1)))   # noqa: E731
    seen = {(a, b): R.cast_map(*down(*centre(a, b)), sc) for a in range(2) for b in range(2)}
    assert seen[0, 0]["id"][0] == R.SEG_CELL + 0 and seen[1, 1]["id"][0] == R.SEG_CELL + 3
    assert seen[0, 1]["id"][0] == render.SEG_SKY                       # NaN draws nothing
    assert seen[1, 0]["id"][0] == render.SEG_SKY                       # h <= floor_z draws nothing
    # lift: h + lift <= floor_z still nothing, above it a column; a top hit moves by exactly lift / |d.z|
    assert R.cast_map(*down(*centre(1, 0)), dict(sc, lift=0.2))["id"][0] == render.SEG_SKY
    assert R.cast_map(*down(*centre(1, 0)), dict(sc, lift=0.25))["id"][0] == R.SEG_CELL + 2
    o, d = _ray((centre(0, 0)[0] + 0.3, centre(0, 0)[1] - 0.2, 0.9), (*centre(0, 0), 0.2))
    t0, t1 = R.cast_map(o, d, sc)["t"][0], R.cast_map(o, d, dict(sc, lift=0.03125))["t"][0]
    assert abs((t0 - t1) - 0.03125 / abs(d[0, 2])) < 1e-12


def test_a_ray_that_starts_inside_a_column_does_not_see_it():
    h = np.array([[0.5, 0.1], [0.1, 0.9]], np.float32)
    sc = _scene(h, res=0.1, floor_z=-0.1)
    lo = sc["lo"] * float(np.float32(0.1))
    inside = np.array([lo[0] + 0.05, lo[1] + 0.05, 0.3])               # inside column (0, 0)
    for to in ((inside[0], inside[1], 5.0), (inside[0] - 1, inside[1], 0.3), (inside[0], inside[1], -5.0)):
        r = R.cast_map(*_ray(inside, to), sc)
        assert r["id"][0] == render.SEG_SKY, to
    # toward the tall neighbour (1, 1): that one it sees, by its wall
    r = R.cast_map(*_ray(inside, (lo[0] + 0.15, lo[1] + 0.151, 0.3)), sc)
    assert r["id"][0] == R.SEG_CELL + 3 and r["n"][0, 2] == 0


def test_tint_albedo():
    lo, hi = 0.25, 0.75
    assert np.allclose(R.cell_albedo(np.array([lo]), lo, hi)[0], R.COLD) and np.allclose(R.cell_albedo(np.array([hi]), lo, hi)[0], R.HOT)
    assert np.allclose(R.cell_albedo(np.array([-3.0]), lo, hi)[0], R.COLD) and np.allclose(R.cell_albedo(np.array([9.0]), lo, hi)[0], R.HOT)
    assert np.allclose(R.cell_albedo(np.array([0.5]), lo, hi)[0], (R.COLD + R.HOT) / 2)
    assert np.allclose(R.cell_albedo(np.array([np.nan]), lo, hi)[0], R.NOVALUE)
    # the three colours and the terrain boxes' can be told apart: 0.3 in some channel, as the header promises
    cols = [R.COLD, R.HOT, R.NOVALUE, tgr.BOX_RGB]
    for i in range(4):
        for j in range(i):
            assert np.abs(cols[i] - cols[j]).max() >= 0.3 - 1e-12, (i, j)
    # through the caster: the tint layer, not the height, colours the cell, and without a layer the height does
    h = np.array([[0.2]], np.float32)
    o, d = _ray((0.05, 0.05, 1.0), (0.05, 0.05, 0.0))
    shade = tgr.AMBIENT + tgr.DIFFUSE * tgr.LIGHT[2]
    for twin, s in ((None, 0.2), (np.array([[0.9]], np.float32), 0.9), (np.array([[np.nan]], np.float32), np.nan)):
        r = R.cast_map(o, d, _scene(h, twin=twin, tint=(0.0, 1.0)))
        want = R.NOVALUE if np.isnan(s) else R.COLD + (R.HOT - R.COLD) * float(np.float32(s))
        assert np.allclose(r["alb"][0], want) and np.array_equal(r["rgb"][0], np.rint(255 * want * shade))
    header = open(os.path.join(tgr.ROOT, "include", "pgtt_render.h")).read()
    for name, col in (("COLD", R.COLD), ("HOT", R.HOT), ("NOVALUE", R.NOVALUE)):
        for ch, x in zip("RGB", col):
            assert f"#define PGTT_RENDER_MAP_{name}_{ch} {x:.2f}f" in header, (name, ch)
    assert np.allclose(render.MAP_COLD, R.COLD) and np.allclose(render.MAP_HOT, R.HOT) and np.allclose(render.MAP_NOVALUE, R.NOVALUE)


def test_the_prescribed_cases_stay_inside_the_ambiguity_cap():
    """the reference alone, columns only, on a prescribed case: under 1 % ambiguous at delta = 3e-4, tops, walls and sky in frame"""
    sc = dict(R.case("g8"), geoms=[])
    ref, amb = R.reference_map_image(sc["cam"], sc["W"], sc["H"], None, None, sc)
    assert amb.mean() <= 0.01
    cells = ref["id"] >= R.SEG_CELL
    assert (cells & (np.abs(ref["n"][:, 2]) == 1)).any() and (cells & (ref["n"][:, 2] == 0)).any() and (ref["id"] == render.SEG_SKY).any()
    assert ((ref["vis"] == 0) & cells).any()                          # columns shadow columns


# ---------------------------------------------------------------- the host side of Renderer.render_map
def test_ctypes_mirror_of_the_map_struct():
    names = [n for n, _ in render.PgttRenderMap._fields_]
    assert names == ["map", "origin", "tint", "grid", "res", "floor_z", "lift", "tint_lo", "tint_hi", "flags"]
    ptr = C.sizeof(C.c_void_p)
    by_hand = 3 * ptr + 4 + 5 * 4 + 4                                  # three pointers, grid, five floats, flags ...
    by_hand += -by_hand % ptr                                          # ... and the tail up to the pointers' alignment
    assert C.sizeof(render.PgttRenderMap) == by_hand == 56
    assert render.PgttRenderMap.grid.offset == 3 * ptr and render.PgttRenderMap.flags.offset == 3 * ptr + 24
    assert render.SEG_CELL == 10000 and render.MAP_TERRAIN == 1 and render.MAP_MAX_GRID == 96
    header = open(os.path.join(tgr.ROOT, "include", "pgtt_render.h")).read()
    assert "#define PGTT_SEG_CELL 10000" in header and "#define PGTT_RENDER_MAP_MAX_GRID 96" in header
    assert "pgtt_render_map" in render.EXPORTS and "pgtt_render_sizeof_map" in render.EXPORTS
    if os.path.exists(render.LIB_PATH):
        L = C.CDLL(render.LIB_PATH)
        assert L.pgtt_render_sizeof_map() == C.sizeof(render.PgttRenderMap)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"render_map reached the library ({name}) with arguments it should have refused")


def _host_renderer(n=3):
    r = object.__new__(render.Renderer)
    r.env = types.SimpleNamespace(device=torch.device("cpu"), num_envs=n, buffers={})
    r.width, r.height, r.shadows, r._lib, r._h, r._ws = 8, 6, True, _NoLibrary(), None, {}
    return r


def test_render_map_refuses_bad_layers_before_any_library_call():
    n, G = 3, 8
    r = _host_renderer(n)
    good = dict(map=torch.zeros(n, G, G), origin=torch.zeros(n, 2, dtype=torch.int32), grid=G, res=0.04)
    bad = {
        "map shape": dict(good, map=torch.zeros(n, G, G + 1)), "map dtype": dict(good, map=torch.zeros(n, G, G, dtype=torch.float64)),
        "map envs": dict(good, map=torch.zeros(n - 1, G, G)), "origin shape": dict(good, origin=torch.zeros(n, 3, dtype=torch.int32)),
        "origin dtype": dict(good, origin=torch.zeros(n, 2, dtype=torch.int64)), "grid 0": dict(good, grid=0),
        "grid above the cap": dict(good, grid=97, map=torch.zeros(n, 97, 97)), "not contiguous": dict(good, map=torch.zeros(n, G, 2 * G)[:, :, ::2]),
        "not a tensor": dict(good, map=np.zeros((n, G, G), np.float32)), "on another device": dict(good, origin=torch.zeros(n, 2, dtype=torch.int32, device="meta")),
    }
    for name, m in bad.items():
        with pytest.raises(ValueError, match="render_map"):
            r.render_map([0], m)
    with pytest.raises(ValueError, match="lacks"):
        r.render_map([0], dict(map=good["map"], origin=good["origin"]))
    for tint in (torch.zeros(n, G, G + 1), torch.zeros(n, G, G, dtype=torch.float16), "var", "dist", "colour"):
        with pytest.raises(ValueError, match="render_map"):
            r.render_map([0], good, tint=tint)
    # a map object without the layer that is asked for
    plain = types.SimpleNamespace(map=good["map"], origin=good["origin"], grid=G, res=0.04, variance=None, dense=False, passes=0)
    for tint in ("var", "dist"):
        with pytest.raises(ValueError, match="needs a map made with"):
            r.render_map([0], plain, tint=tint)
