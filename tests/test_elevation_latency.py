"""Sensor latency (include/pgtt_elevation.h, "Sensor latency: capture-stamped fusion") without a GPU: facts that hold the numpy statement of
tests/elevation_latency_reference.py on its own, the host side of the library (settings, ranges, struct size, refusals), and the inputs
tests/test_gpu_elevation_latency.py holds the device to - the moving case's poses, images and fp64 answers and the seed and ids of its draws are made
and checked here, where no GPU is needed, and imported from here."""
import ctypes as C
import math
import os
import re
import sys
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_reference as dref  # noqa: E402
import elevation_latency_reference as lref  # noqa: E402
import elevation_points_reference as pref  # noqa: E402
import elevation_reference as ref  # noqa: E402
from test_elevation import CAM, box_top_scene, image  # noqa: E402
from test_elevation_follow import BASE_CELLS, MARGIN, MOVES, RES, RES32  # noqa: E402

from phase_guided_terrain_traversal_amd import configs, elevation  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2e-5                                      # test_gpu_elevation.py's bar and doubt radius
# the draws the GPU test makes: 64 envs from a global id that is not 0, latencies in [0, 4]
SEED, ID_OFFSET, DRAW_N, DRAW_TICKS = 20261021, 1000, 64, (0, 4)
# the moving case: three envs (test_elevation_follow's cells; env 2 at negative x and y) walk through these whole-cell moves, one per call, with a new
# place inside the cell and a new yaw near the env's heading at every call; a box stands 0.7 m ahead of each base's first cell
MOVE_SEQ = ("same", "one", "five", "five", "one", "same", "one")
HEADINGS = (0.3, 2.0, -2.5)
MOVING_LAT = (1, 3)
MOVING_GRIDS = (8, 9, 24, 64)
W16, H12 = 16, 12
KEYS = ("map", "origin", "est", "known", "touched")


def same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=np.asarray(a[k]).dtype.kind == "f"), k


# ---------------------------------------------------------------- 1. latency 0 is the reference of the plain tick
POSES = [np.array([0.2, 0.1, 0.45, 0.98, 0.02, -0.03, 0.2]), np.array([0.41, 0.1, 0.45, 0.98, 0.02, -0.03, 0.25]), np.array([-0.3, 0.9, 0.4, 1.0, 0.0, 0.0, 0.0])]


def test_latency_0_is_the_image_reference():
    """test_elevation_points' three ticks of a moving base, with and without the self filter, alpha = 1 and 0.5: every field, bit for bit in fp64"""
    G, boxes, obs = 64, box_top_scene(), np.arange(171.0)
    for cfg in (CAM, dict(CAM, self_half=(0.45, 0.25, 0.45)), dict(CAM, alpha=0.5)):
        a, d = ref.new_state(G), lref.Delayed(G, 0, 0)
        for t, q in enumerate(POSES):
            img = image(q, cfg, boxes)
            wa = ref.tick(a, q, img, cfg, clear=t == 0, obs=obs)
            wd = d.call(t, q, img, cfg, clear=t == 0, obs=obs)
            same(wa, wd, KEYS + ("obs_out", "valid", "point", "cell", "margin", "kept", "self_margin"))
            assert wd["fused"] and wd["lat"] == 0 and wd["slot"] == wd["frame_slot"] == 0 and wa["touched"].sum() > 50
            a = (wa["map"], wa["origin"])


def test_latency_0_is_the_points_reference():
    G, boxes, obs = 64, box_top_scene(), np.arange(171.0)
    for cfg in (CAM, dict(CAM, self_half=(0.45, 0.25, 0.45)), dict(CAM, alpha=0.5)):
        b, d = pref.new_state(G), lref.Delayed(G, 0, 0, points=True)
        for t, q in enumerate(POSES):
            seen = ref.tick(ref.new_state(G), q, image(q, cfg, boxes), dict(cfg, self_half=(0, 0, 0)))
            pts = np.where(seen["valid"][:, None], seen["point"], np.nan)
            wb = pref.tick(b, q, pts, cfg, clear=t == 0, obs=obs)
            wd = d.call(t, q, pts, cfg, clear=t == 0, obs=obs)
            same(wb, wd, KEYS + ("obs_out", "valid", "cell", "kept", "self_margin"))
            assert wd["fused"] and wb["touched"].sum() > 50
            b = (wb["map"], wb["origin"])


# ---------------------------------------------------------------- 2. a static pose: the plain reference, L calls late
@pytest.mark.parametrize("L", (1, 3))
def test_a_static_pose_gives_the_plain_tick_L_calls_late(L):
    G, q, cfg = 64, POSES[0], dict(CAM, alpha=0.5, self_half=(0.45, 0.25, 0.45))
    scenes = [box_top_scene(), [], box_top_scene(), [dict(c=np.array([0.9, 0.2, 0.15]), A=np.eye(3), h=np.array([0.2, 0.2, 0.15]))], [], box_top_scene()]
    imgs = [image(q, cfg, s) for s in scenes]
    plain, a = [], ref.new_state(G)
    for t, img in enumerate(imgs):
        plain.append(ref.tick(a, q, img, cfg, clear=t == 0))
        a = (plain[-1]["map"], plain[-1]["origin"])
    d = lref.Delayed(G, L, L)
    for t, img in enumerate(imgs):
        w = d.call(t, q, img, cfg, clear=t == 0)
        assert w["lat"] == L and w["age"] == min(t + 1, L + 1) and w["fused"] == (t >= L)
        if t < L:
            assert np.isnan(w["map"]).all() and not w["known"].any() and (w["est"] == 0).all() and not w["touched"].any()
            assert np.array_equal(w["origin"], plain[0]["origin"])
        else:
            same(w, plain[t - L])
    assert not np.array_equal(np.nan_to_num(plain[0]["map"]), np.nan_to_num(plain[1]["map"]))     # the images differ: "late" is not "any"


# ---------------------------------------------------------------- 3. the draws
def test_the_draws_cover_their_range():
    """for the seed and the ids the GPU test uses: inside [lo, hi], every value occurs, another counter gives other draws, and the wrap of the counter's
    low word is the Philox word's"""
    lo, hi = DRAW_TICKS
    ids = ID_OFFSET + np.arange(DRAW_N)
    a = lref.draw(SEED, ids, 0, lo, hi)
    assert a.min() >= lo and a.max() <= hi and set(a) == set(range(lo, hi + 1))
    assert not np.array_equal(a, lref.draw(SEED, ids, 1, lo, hi)) and not np.array_equal(a, lref.draw(SEED + 1, ids, 0, lo, hi))
    assert np.array_equal(lref.draw(SEED, ids, 2 ** 32 + 5, lo, hi), lref.draw(SEED, ids, 5, lo, hi))
    assert np.array_equal(lref.draw(SEED, ids[37:42], 0, lo, hi), a[37:42])                         # a function of the global id, not of the batch
    assert (lref.draw(SEED, ids, 3, 2, 2) == 2).all()
    w0 = dref.philox4x32_10((SEED & 0xFFFFFFFF, SEED >> 32), np.array([[ID_OFFSET, 0, lref.RS_LATENCY, 0]], np.uint32))[0, 0]
    assert a[0] == lo + (int(w0) * 5 >> 32) and lref.RS_LATENCY == elevation.RS_LATENCY == 35
    # the ring of the GPU test: D = 3 slots across the wrap of 2^32
    c0 = 2 ** 32 - 2
    assert [(c0 + t) % 3 for t in range(8)] == [2, 0, 1, 2, 0, 1, 2, 0] and [(c0 + t - 2) % 3 for t in range(3)] == [0, 1, 2]


# ---------------------------------------------------------------- 4. the moving case
def pose_at(rng, cells, heading):
    """test_elevation_follow.pose_in with the yaw near `heading`: a base inside world cell `cells`, a little rolled and pitched, whose 117 scan points all
    lie at least MARGIN from a cell border -> qpos [7] of fp32 values"""
    while True:
        yaw = heading + rng.uniform(-0.25, 0.25)
        q = np.array([math.cos(yaw / 2), 0.03 * rng.normal(), 0.03 * rng.normal(), math.sin(yaw / 2)])
        xy = (np.asarray(cells) + rng.uniform(0.2, 0.8, 2)) * RES32
        qpos = np.concatenate([xy, [0.4], q]).astype(np.float32).astype(float)
        if (ref.cell(qpos[:2], RES32) == cells).all() and ref.border_margin(ref.scan_points(qpos), RES32).min() >= MARGIN:
            return qpos


@lru_cache(maxsize=None)
def moving_poses():
    """[T, 3, 7]: the pose of every env at every call"""
    rng = np.random.default_rng(2026)
    return np.stack([np.stack([pose_at(rng, c, HEADINGS[e]) for e, c in enumerate(BASE_CELLS + MOVES[name])]) for name in MOVE_SEQ])


def moving_setup(G):
    """the camera and the map's settings of the moving case: the camera of test_elevation's CAM, 16 x 12; for the small windows it sits further back
    so that its near field lands in them (test_gpu_elevation.case_setup's reason).  The self filter is on from G = 24 on -> (camera, settings)"""
    back, half = {8: (0.7, (0.0, 0.0, 0.0)), 9: (0.7, (0.0, 0.0, 0.0)), 24: (0.3, (0.12, 0.1, 0.45)), 64: (0.0, (0.45, 0.25, 0.45))}[G]
    camera = dict(width=W16, height=H12, fovy=58.0, near=0.1, far=3.0, mount_pos=(-back, 0.0, 0.0),
                  mount_quat=tuple(float(x) for x in dref.pitch_quat(30.0).astype(np.float32)))
    return camera, dict(grid=G, res=RES, alpha=0.5, self_half=half)


def moving_cfg(G):
    camera, settings = moving_setup(G)
    return dict(fovy=camera["fovy"], near=camera["near"], far=camera["far"], mount_pos=camera["mount_pos"], mount_quat=camera["mount_quat"],
                res=settings["res"], alpha=settings["alpha"], self_half=settings["self_half"])


@lru_cache(maxsize=None)
def moving_images(G):
    """[T, 3, 12, 16] fp32: what the camera of moving_setup(G) sees from every pose - the plane z = 0 and the env's box"""
    cfg, out = moving_cfg(G), []
    for qs in moving_poses():
        row = []
        for e, q in enumerate(qs):
            ahead = (BASE_CELLS[e] + 0.5) * RES32 + 0.7 * np.array([math.cos(HEADINGS[e]), math.sin(HEADINGS[e])])
            box = dict(c=np.array([ahead[0], ahead[1], 0.1]), A=np.eye(3), h=np.array([0.15, 0.2, 0.1]))
            cam = ref.camera_pose(q, cfg["mount_pos"], cfg["mount_quat"])
            row.append(dref.depth_image(cam, cfg["fovy"], W16, H12, cfg["near"], cfg["far"], [box])["depth"].astype(np.float32))
        out.append(np.stack(row))
    return np.stack(out)


@lru_cache(maxsize=None)
def moving_observations():
    return np.random.default_rng(78).normal(size=(3, 171)).astype(np.float32)


@lru_cache(maxsize=None)
def moving_reference(G, L):
    """the fp64 answers of the moving case, computed once and shared with the GPU test -> (wants[t][e], doubtful[t][e], shares): every want is
    Delayed.call's dictionary, doubtful the world cells left out from that tick on (test_gpu_elevation.run_sequence's rule: a cell stays in doubt
    while it can hold something of the doubtful tick), shares = (cells left out / touched, scan points left out / scan points, touched)"""
    cfg, poses, imgs, obs = moving_cfg(G), moving_poses(), moving_images(G), moving_observations()
    envs = [lref.Delayed(G, L, L) for _ in range(3)]
    doubt = [set() for _ in range(3)]
    wants, doubts = [], []
    touched = touched_out = scan = scan_out = 0
    for t in range(len(MOVE_SEQ)):
        wants.append([]); doubts.append([])
        for e in range(3):
            w = envs[e].call(t, poses[t, e], imgs[t, e], cfg, clear=t == 0, obs=obs[e].astype(float))
            w["obs_in"] = obs[e]
            wc = ref.world_cells(w["origin"], G)
            doubt[e] &= {tuple(c) for c in wc.reshape(-1, 2)}
            doubt[e] |= ref.doubtful_cells(w, cfg["res"], EPS)
            out = np.array([[tuple(wc[i, j]) in doubt[e] for j in range(G)] for i in range(G)])
            touched += int(w["touched"].sum()); touched_out += int((w["touched"] & out).sum())
            left = (w["scan"]["margin"] < EPS) | np.array([tuple(c) in doubt[e] for c in w["scan"]["cell"]])
            scan += ref.NSCAN; scan_out += int(left.sum())
            wants[-1].append(w); doubts[-1].append(frozenset(doubt[e]))
    return wants, doubts, (touched_out / max(touched, 1), scan_out / scan, touched)


def test_the_moving_poses_keep_their_margin():
    p = moving_poses()
    assert p.shape == (len(MOVE_SEQ), 3, 7)
    for t, name in enumerate(MOVE_SEQ):
        for e in range(3):
            assert np.array_equal(p[t, e], p[t, e].astype(np.float32).astype(float))
            assert np.array_equal(ref.cell(p[t, e, :2], RES32), (BASE_CELLS + MOVES[name])[e]), (t, e)
            assert ref.border_margin(ref.scan_points(p[t, e]), RES32).min() >= MARGIN, (t, e)
    yaws = np.array([[ref.yaw_of(q) for q in row] for row in p])
    assert (np.abs(np.diff(yaws, axis=0)) > 1e-3).all() and (p[0, 2, :2] < 0).all()


@pytest.mark.parametrize("L", MOVING_LAT)
@pytest.mark.parametrize("G", MOVING_GRIDS)
def test_the_moving_case_for_the_reference_alone(G, L):
    """the doubt rule's two shares stay under the caps of 5 % on the moving case's own inputs, the case is not vacuous, and it holds what it is
    for: a capture pose that puts a pixel into another cell than the current pose would, and one that puts the self-filter box elsewhere.
    Shares (cells, scan points) and touched cells, L = 1 / L = 3: printed below, a few tenths of a per cent."""
    wants, _, (cells, scan, touched) = moving_reference(G, L)
    print(f"G={G} L={L}: touched {touched}, cells left out {100 * cells:.2f} %, scan points left out {100 * scan:.2f} %")
    assert cells <= 0.05 and scan <= 0.05 and touched >= 20
    cfg, poses, imgs = moving_cfg(G), moving_poses(), moving_images(G)
    other_cell = other_box = known = 0
    for t, row in enumerate(wants):
        for e, w in enumerate(row):
            assert w["fused"] == (t >= L) and w["lat"] == L
            assert np.array_equal(w["origin"], (BASE_CELLS + MOVES[MOVE_SEQ[t]])[e])              # the window follows the CURRENT pose
            known += int(w["known"].sum())
            if not w["fused"]:
                assert not w["touched"].any()
                continue
            # the same frame under the current pose
            now = lref.stamped_tick(ref.new_state(G), poses[t, e], poses[t, e], imgs[t - L, e], cfg, clear=True)
            v = w["valid"]
            other_cell += int((w["cell"][v] != now["cell"][v]).any(1).sum())
            # the frame's points (under the capture pose) against the box of the CURRENT base: what a kernel that shared one base would drop
            qn = poses[t, e, 3:7] / np.linalg.norm(poses[t, e, 3:7])
            in_box_now = (np.abs((w["point"] - poses[t, e, :3]) @ dref.qmat(qn)) <= np.asarray(cfg["self_half"], float)).all(1)
            other_box += int((w["kept"] != (v & ~in_box_now)).sum())
    assert other_cell > 0 and known > 0
    if G >= 24:
        assert any(cfg["self_half"]) and other_box > 0
    else:
        assert not any(cfg["self_half"])


# ---------------------------------------------------------------- 5. clears and the ring, in the reference
def test_a_clear_redraws_and_forgets_the_old_frames():
    G, lo, hi = 24, 1, 3
    q = np.array([0.0, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0])
    d = lref.Delayed(G, lo, hi, seed=SEED, gid=ID_OFFSET + 1, points=True)
    old = np.array([[0.1, 0.1, 5.0], [0.2, -0.1, 5.0]])
    new = np.array([[0.1, 0.1, 0.25], [0.2, -0.1, 0.5]])
    for c in range(5):
        w = d.call(c, q, old, CAM, clear=c == 0)
    assert w["lat"] == lref.draw(SEED, [ID_OFFSET + 1], 0, lo, hi)[0] and (w["map"] == 5.0).sum() == 2 and w["age"] == hi + 1
    seen = []
    for c in range(5, 11):
        w = d.call(c, q, new, CAM, clear=c == 5)
        assert w["lat"] == lref.draw(SEED, [ID_OFFSET + 1], 5, lo, hi)[0] and w["age"] == min(c - 4, hi + 1)
        assert w["fused"] == (c - 5 >= w["lat"]) and not (w["map"] == 5.0).any()
        seen.append(int((~np.isnan(w["map"])).sum()))
    assert seen[0] == 0 and seen[-1] == 2


# ---------------------------------------------------------------- the host side
def test_the_settings_parser():
    ls = elevation.latency_settings
    assert ls(None) is None and ls(False) is None
    assert ls(0) == dict(ticks=(0, 0), seed=0) and ls(3) == dict(ticks=(3, 3), seed=0)
    assert ls((1, 4)) == dict(ticks=(1, 4), seed=0) and ls([0, 2]) == dict(ticks=(0, 2), seed=0)
    assert ls({}) == dict(ticks=(0, 0), seed=0) == dict(ticks=tuple(elevation.LATENCY_DEFAULTS["ticks"]), seed=elevation.LATENCY_DEFAULTS["seed"])
    assert ls(dict(ticks=2)) == dict(ticks=(2, 2), seed=0) and ls(dict(ticks=(0, 4), seed=7)) == dict(ticks=(0, 4), seed=7)
    for bad in (True, 1.5, "2", (1,), (1, 2, 3), (1, 2.0), dict(tick=2), dict(ticks="2"), dict(ticks=(0, 1), seed=1.5), dict(ticks=True)):
        with pytest.raises(ValueError, match="latency"):
            ls(bad)
    assert "latency" not in elevation.DEFAULTS and elevation.MAX_LATENCY == lref.MAX_LATENCY == 8
    s = elevation.latency_struct(ticks=(1, 4), seed=2 ** 64 + 5, env_id_offset=9)
    assert (s.lat_lo, s.lat_hi, s.D, s.seed, s.env_id_offset) == (1, 4, 5, 5, 9) and elevation.latency_struct(ticks=(0, 2), D=7).D == 7


def test_the_struct_and_the_declarations():
    assert C.sizeof(elevation.PgttElevationLatency) == 80
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "pgtt_elevation.h")).read())
    for decl in ("int pgtt_elevation_check_latency(const PgttElevationLatency* l);",
                 "int pgtt_elevation_bind_latency(pgtt_elevation_handle h, const PgttElevationLatency* l);",
                 "int pgtt_elevation_delayed(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream);",
                 "int pgtt_elevation_sizeof_latency(void);", "#define PGTT_RS_LATENCY 35", "#define PGTT_ELEVATION_MAX_LATENCY 8",
                 "Sensor latency: capture-stamped fusion"):
        assert decl in text, decl
    for name in ("pgtt_elevation_check_latency", "pgtt_elevation_bind_latency", "pgtt_elevation_delayed", "pgtt_elevation_sizeof_latency"):
        assert name in elevation.EXPORTS, name


needs_lib = pytest.mark.skipif(not os.path.exists(elevation.LIB_PATH), reason="libpgtt_elevation.so not built (run __graft_entry__.build())")


@needs_lib
def test_check_latency_range_table():
    L = elevation.lib()
    assert L.pgtt_elevation_sizeof_latency() == C.sizeof(elevation.PgttElevationLatency)
    ok = lambda **kw: L.pgtt_elevation_check_latency(C.byref(elevation.latency_struct(**kw)))
    for ticks, D in (((0, 0), None), ((0, 0), 9), ((8, 8), None), ((0, 8), 9), ((2, 4), 5), ((2, 4), 9), ((3, 3), 4)):
        assert ok(ticks=ticks, D=D) == 0, (ticks, D)
    for ticks, D in (((-1, 0), 1), ((3, 2), 4), ((0, 9), 9), ((9, 9), None), ((0, 4), 4), ((0, 8), 10), ((0, 0), 0), ((0, 0), 10), ((2, 4), -1)):
        assert ok(ticks=ticks, D=D) == -1, (ticks, D)
        assert b"pgtt_elevation_check_latency" in L.pgtt_elevation_last_error()
    assert L.pgtt_elevation_check_latency(None) == -1
    assert L.pgtt_elevation_bind_latency(None, C.byref(elevation.latency_struct())) == -1 and L.pgtt_elevation_delayed(None, None, 0, 0, None) == -1


def test_the_refusals():
    """before anything touches a device or the env: the variance tick, visibility and follow_sensor behind a latency are not built"""
    from phase_guided_terrain_traversal_amd.env import Joystick
    for other in (dict(variance=True), dict(visibility=True), dict(follow_sensor=True), dict(variance=dict(gate=2.0))):
        with pytest.raises(ValueError, match="not built"):
            elevation.ElevationMap(None, latency=2, **other)
        with pytest.raises(ValueError, match="not built"):
            Joystick("stairs", configs.training_config(), num_envs=4, depth=dict(), elevation=dict(grid=24, latency=(0, 2), **other))
    with pytest.raises(ValueError, match="latency"):
        elevation.ElevationMap(None, latency="2")
    with pytest.raises(ValueError, match="needs depth"):
        Joystick("stairs", configs.training_config(), num_envs=4, elevation=dict(latency=2))


def test_evaluate_flag():
    """--sensor_latency LO[,HI]: refused without --elevation, outside its range and with what is not built, before anything touches a device"""
    sys.path.insert(0, ROOT)
    import evaluate
    ap = evaluate.make_parser()
    assert ap.parse_args([]).sensor_latency is None
    kw = evaluate.sensor_kwargs(ap.parse_args(["--elevation", "--sensor_latency", "2"]))
    assert kw["elevation"] == dict(latency=(2, 2)) and "every" not in kw["depth"]
    kw = evaluate.sensor_kwargs(ap.parse_args(["--elevation", "24", "--elevation_source", "lidar", "--sensor_latency", "0,4", "--odometry_drift", "--elevation_fill"]))
    assert kw["elevation"]["latency"] == (0, 4) and kw["elevation"]["source"] == "lidar" and kw["elevation"]["odometry"] is True and kw["elevation"]["fill"] is True
    assert evaluate.sensor_kwargs(ap.parse_args(["--elevation"]))["elevation"] is True                     # without the flag: what it was
    for bad, why in ((["--sensor_latency", "2"], "give --elevation too"), (["--elevation", "--sensor_latency", "9"], "HI <= 8"),
                     (["--elevation", "--sensor_latency", "3,2"], "LO <= HI"), (["--elevation", "--sensor_latency", "1.5"], "whole numbers"),
                     (["--elevation", "--sensor_latency", "1,2,3"], "LO or LO,HI"), (["--elevation", "--sensor_latency", "2", "--sensor_every", "3"], "not built"),
                     (["--elevation", "--sensor_latency", "2", "--elevation_variance"], "not built"),
                     (["--elevation", "--sensor_latency", "2", "--elevation_visibility"], "not built")):
        with pytest.raises(SystemExit, match=why):
            evaluate.sensor_kwargs(ap.parse_args(bad))
