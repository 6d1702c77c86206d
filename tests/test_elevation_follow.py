"""Following a slower sensor (include/pgtt_elevation.h), without a GPU: the numpy statement of tests/elevation_follow_reference.py on maps whose
answer is known by hand, the schedule, the two declarations, and the poses tests/test_gpu_elevation_follow.py holds the device to (exported from
here, so that their margin is asserted where no GPU is needed)."""
import math
import os
import re
import sys
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_follow_reference as fol  # noqa: E402
import elevation_reference as ref  # noqa: E402
from test_elevation import CAM, image  # noqa: E402

from phase_guided_terrain_traversal_amd import elevation  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.04
RES32 = float(np.float32(RES))
MARGIN = 1e-4                                   # test_gpu_elevation_fill.py's: about 8 x the fp32 error of a scan point's coordinate within 20 m
FAR_CELLS = 97                                  # a move of more than G cells for every G <= 96
# the cells of the three bases (env 2 at negative x and y; none a multiple of a tested G, nor is its window's first cell), and the whole-cell moves
# of the hold calls, per env
BASE_CELLS = np.array([[33, 57], [203, -115], [-33, -19]])
MOVES = {"same": np.zeros((3, 2), int), "one": np.array([[1, 0], [0, -1], [-1, 1]]), "five": np.array([[5, -3], [-5, 2], [-4, -5]]),
         "far": np.array([[FAR_CELLS, 0], [0, -FAR_CELLS], [-FAR_CELLS, FAR_CELLS]])}


def pose_in(rng, cells):
    """a base somewhere inside world cell `cells` at any yaw, a little rolled and pitched, whose 117 scan points all lie at least MARGIN from a cell
    border: chosen by rejection -> qpos [7] of fp32 values"""
    while True:
        yaw = rng.uniform(-math.pi, math.pi)
        q = np.array([math.cos(yaw / 2), 0.03 * rng.normal(), 0.03 * rng.normal(), math.sin(yaw / 2)])
        xy = (np.asarray(cells) + rng.uniform(0.2, 0.8, 2)) * RES32
        qpos = np.concatenate([xy, [0.4], q]).astype(np.float32).astype(float)
        if (ref.cell(qpos[:2], RES32) == cells).all() and ref.border_margin(ref.scan_points(qpos), RES32).min() >= MARGIN:
            return qpos


@lru_cache(maxsize=None)
def poses():
    """{"base": [3, 7], "same" | "one" | "five" | "far": [3, 7]}: the pose of the fresh call and those of the holds behind it - the base moved by
    whole cells (and inside the cell), with another yaw each ("same": another place and yaw inside the same cell)"""
    rng = np.random.default_rng(2024)
    out = {"base": np.stack([pose_in(rng, c) for c in BASE_CELLS])}
    for name, mv in MOVES.items():
        out[name] = np.stack([pose_in(rng, c) for c in BASE_CELLS + mv])
    return out


def test_the_exported_poses_keep_their_margin():
    p = poses()
    assert set(p) == {"base"} | set(MOVES)
    for name, qs in p.items():
        cells = BASE_CELLS + (MOVES[name] if name in MOVES else 0)
        for e, q in enumerate(qs):
            assert np.array_equal(q, q.astype(np.float32).astype(float))
            assert np.array_equal(ref.cell(q[:2], RES32), cells[e]), (name, e)
            assert ref.border_margin(ref.scan_points(q), RES32).min() >= MARGIN, (name, e)
    assert (p["base"][2][:2] < 0).all()
    yaws = np.array([[ref.yaw_of(q) for q in p[k]] for k in ("base", "same", "one", "five")])
    assert (np.abs(np.diff(yaws, axis=0)) > 1e-3).all()                      # the yaw changes with every move
    for G in (8, 9, 24, 64):                                                 # the toroidal seam is inside every window
        assert (BASE_CELLS % G != 0).all() and ((BASE_CELLS - G // 2) % G != 0).all(), G


def ticked(G=64):
    """one tick of the flat ground under a level base -> (tick's dict, qpos)"""
    qpos = np.array([0.013, -0.021, 0.3, 1.0, 0.0, 0.0, 0.0])
    return ref.tick(ref.new_state(G), qpos, image(qpos, CAM, dtype=np.float64), CAM), qpos


def test_a_hold_leaves_the_map_and_the_origin_alone():
    out, qpos = ticked()
    m32 = out["map"].astype(np.float32)
    moved = qpos.copy()
    moved[:2] += (0.21, -0.13)
    h = fol.hold((m32, out["origin"]), moved, CAM)
    assert np.array_equal(h["map"].view(np.int32), m32.view(np.int32)) and np.array_equal(h["origin"], out["origin"])
    assert not np.array_equal(ref.cell(moved[:2], RES32), out["origin"])     # though the base has left the origin's cell
    assert h["known"].sum() > 10


def test_a_hold_behind_a_tick_at_the_same_pose_returns_the_ticks_scan():
    out, qpos = ticked()
    obs = np.random.default_rng(0).normal(size=171).astype(np.float32)
    h = fol.hold((out["map"], out["origin"]), qpos, CAM, obs=obs)
    assert out["known"].sum() > 10 and np.array_equal(h["known"], out["known"])
    assert np.allclose(h["est"], out["est"], rtol=0, atol=1e-6)              # the tick's est is an fp64 difference, the hold's an fp32 one
    assert np.array_equal(h["obs_out"][:38], obs[:38]) and np.array_equal(h["obs_out"][155:], obs[155:]) and np.array_equal(h["obs_out"][38:155], h["est"])


def step_map(G=64):
    """a window centred on world cell (0, 0) that knows every cell: 0.2 where the world cell's ix >= 10, else 0 -> (map in slot layout, origin)"""
    origin = np.zeros(2, np.int64)
    wc = ref.world_cells(origin, G)
    return np.where(wc[..., 0] >= 10, np.float32(0.2), np.float32(0.0)).astype(np.float32), origin


def test_a_moved_base_reads_the_heights_it_should():
    """the step edge at x = 0.4 m, the scan rows 0.1 m apart along x: a base at x = 0.02 has its rows r = 0, 1, 2 (x = 0.62, 0.52, 0.42) on the step;
    moved by one cell (x = 0.06) still those three; moved by five (x = 0.22) the rows r = 0 .. 4"""
    m, origin = step_map()
    cfg = dict(res=RES)
    for cells, rows_up in ((0, 3), (1, 3), (5, 5)):
        qpos = np.array([(cells + 0.5) * RES32, 0.5 * RES32, 0.3, 1.0, 0.0, 0.0, 0.0])
        h = fol.hold((m, origin), qpos, cfg)
        assert h["known"].all()
        r = np.arange(117) // 9
        x = qpos[0] + (6 - r) * 0.1
        assert np.array_equal(np.floor(x / RES32) >= 10, r < rows_up)           # the docstring's arithmetic
        want = np.where(r < rows_up, np.float32(0.2), np.float32(0.0)).astype(np.float32)
        assert np.array_equal(h["est"].view(np.int32), want.view(np.int32)), cells
        assert np.array_equal(h["origin"], origin) and np.array_equal(h["map"], m)
    # a window that is all step: the minimum is the step's own height and est is 0
    h = fol.hold((np.where(np.isnan(m), m, np.float32(0.2)), origin), qpos, cfg)
    assert h["known"].all() and (h["est"] == 0).all()


def test_a_move_of_G_cells_knows_nothing():
    """the scan reaches 0.6 m, 15 cells, from the base and the window G / 2 cells from its origin: a base G + 16 cells away has no scan point in
    the window, and FAR_CELLS are that far for every G <= 96"""
    for G in (8, 24, 64):
        m = np.full((G, G), 0.25, np.float32)
        origin = np.array([3, -5])
        for mv in ((G + 16, 0), (0, -(G + 16)), (FAR_CELLS, FAR_CELLS)):
            qpos = np.array([(origin[0] + mv[0] + 0.5) * RES32, (origin[1] + mv[1] + 0.5) * RES32, 0.3, 1.0, 0.0, 0.0, 0.0])
            h = fol.hold((m, origin), qpos, dict(res=RES))
            assert not h["known"].any() and (h["est"] == 0).all() and h["est"].dtype == np.float32
            assert np.array_equal(h["map"], m) and np.array_equal(h["origin"], origin)
    # an origin no tick ever wrote is read as the clamp: nothing is known, and it is not rewritten
    h = fol.hold((m, np.array([2 ** 31 - 1, -2 ** 31])), qpos, dict(res=RES))
    assert not h["known"].any() and np.array_equal(h["origin"], [2 ** 31 - 1, -2 ** 31])


def test_a_cleared_hold():
    out, qpos = ticked()
    moved = qpos.copy()
    moved[:2] = (-1.234, 0.777)
    obs = np.arange(171, dtype=np.float32)
    h = fol.hold((out["map"], out["origin"]), moved, CAM, clear=True, obs=obs)
    assert np.isnan(h["map"]).all() and np.array_equal(h["origin"], [-31, 19]) and np.array_equal(h["origin"], ref.cell(moved[:2], RES32))
    assert not h["known"].any() and (h["est"] == 0).all() and (h["obs_out"][38:155] == 0).all() and np.array_equal(h["obs_out"][:38], obs[:38])
    assert not np.isnan(out["map"]).all()                                     # the caller's state is not modified


def test_the_schedule():
    """every = 3, seven calls behind a sensor that started at counter 0: fresh at c = 0, 3, 6; force overrides it; a counter that no sensor call has
    advanced (c = -1) is not fresh"""
    assert [fol.fresh(c + 1, 3) for c in range(7)] == [True, False, False, True, False, False, True]
    assert [fol.fresh(c + 1, 2) for c in range(7)] == [True, False, True, False, True, False, True]
    assert all(fol.fresh(c + 1, 1) for c in range(7)) and all(fol.fresh(c + 1, 3, force=True) for c in range(7))
    assert not fol.fresh(0, 3) and not fol.fresh(0, 1) and fol.fresh(0, 3, force=True)
    G = 64
    state, maps = ref.new_state(G), []
    qpos = np.array([0.013, -0.021, 0.3, 1.0, 0.0, 0.0, 0.0])
    for c in range(7):
        qpos = qpos + np.array([0.05, 0.0, 0, 0, 0, 0, 0])                   # the base walks on; the image is the last fresh call's pose's own
        if fol.fresh(c + 1, 3):
            img = image(qpos, CAM, dtype=np.float64)
        out = fol.follow(state, qpos, img, dict(CAM, alpha=0.5), c + 1, 3)
        assert out["fresh"] == (c % 3 == 0)
        state = (out["map"], out["origin"])
        maps.append(np.nan_to_num(np.asarray(out["map"], float), nan=-7.0))
    changed = [not np.array_equal(maps[c], maps[c - 1]) for c in range(1, 7)]
    assert changed == [False, False, True, False, False, True]
    forced = fol.follow(state, qpos, img, dict(CAM, alpha=0.5), 8, 3, force=True)
    assert forced["fresh"] and not np.array_equal(np.nan_to_num(forced["map"], nan=-7.0), maps[-1])


def test_the_declarations():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "pgtt_elevation.h")).read())
    assert "int pgtt_elevation_bind_rate(pgtt_elevation_handle h, const int64_t* counter, int every);" in text
    assert ("int pgtt_elevation_follow(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, int force, void* stream);"
            in text)
    assert "Following a slower sensor" in text
    assert "pgtt_elevation_bind_rate" in elevation.EXPORTS and "pgtt_elevation_follow" in elevation.EXPORTS
    assert "follow_sensor" not in elevation.DEFAULTS
    if os.path.exists(elevation.LIB_PATH):
        L = elevation.lib()
        assert L.pgtt_elevation_bind_rate and L.pgtt_elevation_follow


def test_evaluate_flag():
    """--sensor_every M: 1 unless given, refused without --elevation and below 1 before anything touches a device"""
    import pytest
    sys.path.insert(0, ROOT)
    import evaluate
    ap = evaluate.make_parser()
    assert ap.parse_args([]).sensor_every == 1 and ap.parse_args(["--elevation", "--sensor_every", "3"]).sensor_every == 3
    base = ["--policy", "policy177", "--terrain_file", "level4"]
    with pytest.raises(SystemExit, match="give --elevation too"):
        evaluate.run_evaluation(ap.parse_args(base + ["--sensor_every", "3"]), num_eval_envs=4, verbose=False)
    with pytest.raises(SystemExit, match="period"):
        evaluate.run_evaluation(ap.parse_args(base + ["--elevation", "--sensor_every", "0"]), num_eval_envs=4, verbose=False)


def test_the_refusals_stand_without_the_flag():
    """before anything touches a device: follow_sensor lifts the two `every=1` refusals and no other"""
    import pytest
    from phase_guided_terrain_traversal_amd import configs
    from phase_guided_terrain_traversal_amd.env import Joystick
    cfg = configs.training_config()
    for emap in (dict(grid=24), dict(grid=24, follow_sensor=False)):
        with pytest.raises(ValueError, match="every=1"):
            Joystick("stairs", cfg, num_envs=4, depth=dict(every=2), elevation=emap)
        with pytest.raises(ValueError, match="every=1"):
            Joystick("stairs", cfg, num_envs=4, lidar=dict(every=2), elevation=dict(emap, source="lidar"))
    with pytest.raises(ValueError, match="torso"):
        Joystick("stairs", cfg, num_envs=4, depth=dict(every=2, mount_body=1), elevation=dict(follow_sensor=True))
    with pytest.raises(ValueError, match="needs lidar"):
        Joystick("stairs", cfg, num_envs=4, depth=dict(every=2), elevation=dict(follow_sensor=True, source="lidar"))
