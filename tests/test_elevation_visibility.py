"""The visibility clean-up of the elevation map without a GPU: facts that hold tests/elevation_visibility_reference.py (the fp64 statement of the
block "Visibility clean-up" of include/pgtt_elevation.h that the GPU tests compare the kernel with) on its own; the host side of the new entries -
the ranges of pgtt_elevation_check_visibility, the struct's size, the header's declarations, EXPORTS, the refusals of ElevationMap that come before
anything touches a device; and the cap check: on depth_reference images of the GPU test's cases the reference alone leaves at most 5 % of the cells
with a bound undecided, for the bound and for the verdict.  What the GPU test shares with this file (the cases, their cameras, the preparation of
the map) lives here."""
import ctypes as C
import os
import re
import sys
import types
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_reference as dref  # noqa: E402
import elevation_reference as ref  # noqa: E402
import elevation_visibility_reference as vref  # noqa: E402

from phase_guided_terrain_traversal_amd import depth as depth_mod, elevation  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL4 = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy")
EPS = 2e-5                                     # tests/test_gpu_elevation.py's (test_eps_is_the_elevation_tests)
RES = 0.04
VARIANTS = [0, 2, 7]                           # tests/test_gpu_elevation.py's
CAP = 0.05
VIS = dict(margin=0.05, end_guard=0.06, sigmas=0.0)
CAM = dict(fovy=58.0, near=0.1, far=3.0, mount_pos=(0.0, 0.0, 0.0), mount_quat=dref.pitch_quat(30.0).astype(np.float32).astype(float), res=RES, alpha=1.0,
           self_half=(0.0, 0.0, 0.0))
W, H = 64, 48
# the GPU test's cases: (width, height, G, stride)
CASES = [(w, h, g, s) for (w, h) in ((16, 12), (48, 32)) for g in (8, 9, 24, 64) for s in (1, 3)]


def case_setup(camera, G):
    """the camera and the map's settings of a case.  A window of 8 or 9 cells is 0.32 m or 0.36 m around the base and one of 24 cells 0.96 m, which a
    camera that looks ahead from the head hardly sees, and a ray is sampled over 2 G cells only: those cases tell the map that the camera sits
    0.25 m and 0.5 m behind the base, so that its rays cross the window and its near field lands in it (the map does not care how the image was
    made).  G < 24 runs without the self filter, G = 24 with a small box, G = 64 with the default one."""
    settings = dict(grid=G, res=RES, alpha=1.0, self_half=(0.45, 0.25, 0.45))
    if G <= 24:
        camera = dict(camera, mount_pos=(-0.25 if G < 24 else camera["mount_pos"][0] - 0.5, 0.0, camera["mount_pos"][2]))
        settings["self_half"] = (0.0, 0.0, 0.0) if G < 24 else (0.12, 0.1, 0.45)
    return camera, settings


def ref_cfg(camera, settings):
    return dict(fovy=camera["fovy"], near=camera["near"], far=camera["far"], mount_pos=camera["mount_pos"], mount_quat=camera["mount_quat"], res=settings["res"],
                alpha=settings["alpha"], self_half=settings["self_half"])


def prepare(hmap, seed):
    """what the GPU test does to a ticked map on the host: a seeded tenth of the known cells raised by 0.3 m, heights written into a tenth of the
    unknown ones -> the new map as fp32 values, [G, G]"""
    rng = np.random.default_rng(seed)
    m = np.array(hmap, np.float32)
    known = np.flatnonzero(~np.isnan(m.reshape(-1)))
    unknown = np.flatnonzero(np.isnan(m.reshape(-1)))
    up = rng.choice(known, (len(known) + 9) // 10, replace=False) if len(known) else known
    new = rng.choice(unknown, (len(unknown) + 9) // 10, replace=False) if len(unknown) else unknown
    m.reshape(-1)[up] += np.float32(0.3)
    m.reshape(-1)[new] = rng.uniform(-0.1, 0.5, len(new)).astype(np.float32)
    return m


def image(qpos, cfg, boxes=(), dtype=np.float32, w=W, h=H):
    """the noise-free image of the plane z = 0 and `boxes` from the camera of `cfg` on a base at `qpos` (depth_reference's ray caster)"""
    cam = ref.camera_pose(qpos, cfg["mount_pos"], cfg["mount_quat"])
    return dref.depth_image(cam, cfg["fovy"], w, h, cfg["near"], cfg["far"], boxes)["depth"].astype(dtype)


def slot_of(x, y, G):
    c = ref.cell(np.array([x, y]), RES)
    return int(c[0] % G), int(c[1] % G)


Q0 = np.array([0.013, -0.021, 0.3, 1.0, 0.0, 0.0, 0.0])


# ---------------------------------------------------------------- the reference on its own
def test_eps_is_the_elevation_tests():
    text = open(os.path.join(ROOT, "tests", "test_gpu_elevation.py")).read()
    assert re.search(r"^EPS = 2e-5$", text, re.M) and EPS == 2e-5 == vref.BAR


@pytest.mark.parametrize("margin", [1e-4, 0.01, 0.05])
def test_a_plane_seen_from_above_clears_nothing(margin):
    G = 64
    img = image(Q0, CAM)
    out = ref.tick(ref.new_state(G), Q0, img, CAM)
    v = vref.visibility((out["map"], out["origin"]), Q0, CAM, dict(VIS, margin=margin, stride=1), depth=img)
    assert out["touched"].sum() > 100 and v["has_bound"].sum() > 100 and v["samples"] > 1000
    assert v["cleared"] == 0 and not v["clear_any"].any()
    assert np.nanmin(v["bound_any"]) > -1e-6                                   # no ray passes below the ground it ends on


def test_a_phantom_in_view_is_cleared_and_one_behind_an_occluder_is_not():
    G = 64
    wall = [dict(c=np.array([0.95, 0.0, 0.2]), A=np.eye(3), h=np.array([0.05, 1.5, 0.2]))]      # x in [0.9, 1.0], up to z = 0.4, above the sensor
    for boxes, behind in (((), False), (wall, True)):
        img = image(Q0, CAM, boxes)
        out = ref.tick(ref.new_state(G), Q0, img, CAM)
        m = out["map"].copy()
        near, far = slot_of(0.5, 0.0, G), slot_of(1.2, 0.0, G)
        m[near], m[far] = 0.3, 0.3
        v = vref.visibility((m, out["origin"]), Q0, CAM, dict(VIS, stride=1), depth=img)
        assert v["clear_sure"][near] and v["verdict_decided"][near] and np.isnan(v["map"][near])
        if behind:                                                              # no ray passes the wall: the cell behind it has no bound at all
            assert not v["has_bound"][far] and not v["clear_any"][far] and v["map"][far] == 0.3
        else:
            assert v["clear_sure"][far]
        kept = ~v["clear_any"]
        assert np.array_equal(v["map"][kept], m[kept], equal_nan=True)


def test_end_guard_protects_the_hit_cell():
    """rays that end low on a wall's face sample the wall's own cell below its top when they are sampled up to their end, and forget it; an end
    guard of a cell and a half keeps every sample out of the cell that was hit"""
    G = 64
    wall = [dict(c=np.array([0.95, 0.0, 0.1]), A=np.eye(3), h=np.array([0.05, 1.5, 0.1]))]      # top at 0.2: the camera sees the face and the top
    img = image(Q0, CAM, wall)
    out = ref.tick(ref.new_state(G), Q0, img, CAM)
    wc = ref.world_cells(out["origin"], G)
    hit = out["touched"] & (out["map"] > 0.15) & (wc[..., 0] == ref.cell(0.9 + 1e-3, RES))     # the cells that hold the face
    assert hit.sum() > 10
    state = (out["map"], out["origin"])
    guarded = vref.visibility(state, Q0, CAM, dict(VIS, stride=1), depth=img)
    bare = vref.visibility(state, Q0, CAM, dict(VIS, end_guard=0.0, stride=1), depth=img)
    assert not guarded["clear_any"][hit].any()
    assert bare["clear_sure"][hit].sum() > 5


def test_permuting_the_points_changes_nothing_and_stride_selects_the_stated_rays():
    G = 64
    box = [dict(c=np.array([1.0, 0.2, 0.1]), A=np.eye(3), h=np.array([0.2, 0.3, 0.1]))]
    img = image(Q0, CAM, box)
    out = ref.tick(ref.new_state(G), Q0, img, CAM)
    state = (prepare(out["map"], 3), out["origin"])
    pts = out["point"][out["valid"]]
    vis = dict(VIS, stride=1, sensor_pos=CAM["mount_pos"])
    a = vref.visibility(state, Q0, CAM, vis, points=pts)
    b = vref.visibility(state, Q0, CAM, vis, points=pts[np.random.default_rng(1).permutation(len(pts))])
    c = vref.visibility(state, Q0, CAM, vis, depth=img)
    for k in ("bound_sure", "bound_any", "clear_sure", "map"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(a[k], c[k], equal_nan=True), k                    # the valid pixels' points from the camera's place: the same rays
    assert a["cleared"] > 0
    # stride 3 = stride 1 on an image whose other pixels read far
    masked = np.full_like(img, CAM["far"])
    masked[::3, ::3] = img[::3, ::3]
    s3 = vref.visibility(state, Q0, CAM, dict(VIS, stride=3), depth=img)
    s1 = vref.visibility(state, Q0, CAM, dict(VIS, stride=1), depth=masked)
    for k in ("bound_sure", "bound_any", "clear_sure"):
        assert np.array_equal(s3[k], s1[k], equal_nan=True), k
    assert 0 < s3["samples"] < c["samples"] / 4
    assert list(vref.selected_pixels(4, 5, 3)) == [0, 3, 15, 18]
    # every third point
    p3 = vref.visibility(state, Q0, CAM, dict(vis, stride=3), points=pts)
    p1 = vref.visibility(state, Q0, CAM, vis, points=pts[::3])
    assert np.array_equal(p3["bound_any"], p1["bound_any"], equal_nan=True)


def test_an_env_that_will_be_cleared_is_skipped():
    G = 24
    img = image(Q0, CAM)
    m = np.full((G, G), 0.7)
    v = vref.visibility((m, np.zeros(2, np.int64)), Q0, CAM, dict(VIS, stride=1), depth=img, skip=True)
    assert v["cleared"] == 0 and np.isnan(v["bound_any"]).all() and (v["map"] == 0.7).all()
    w = vref.visibility((m, np.zeros(2, np.int64)), Q0, CAM, dict(VIS, stride=1), depth=img)
    assert w["cleared"] > 0


def test_no_samples_without_a_horizontal_run():
    """a camera that looks straight down from above the window's centre: Lh is 0 at the image's centre and below the first sample around it"""
    G = 24
    down = dict(CAM, mount_quat=dref.pitch_quat(90.0).astype(np.float32).astype(float))
    img = image(Q0, down, w=3, h=3)
    v = vref.visibility((np.full((G, G), 0.2), ref.cell(Q0[:2], RES)), Q0, down, dict(VIS, end_guard=0.0, stride=1), depth=img)
    assert np.isfinite(v["bound_any"][v["has_bound"]]).all()
    one = vref.visibility((np.full((G, G), 0.2), ref.cell(Q0[:2], RES)), Q0, down, dict(VIS, end_guard=0.0, stride=1), depth=img[1:2, 1:2])
    assert one["samples"] == 0 and not one["has_bound"].any()


# ---------------------------------------------------------------- the host side
def test_struct_defaults_and_settings():
    assert C.sizeof(elevation.PgttElevationVisibility) == 48
    assert elevation.visibility_settings(None) is None and elevation.visibility_settings(False) is None
    s = elevation.visibility_settings(True, res=0.04)
    assert s == dict(margin=0.05, end_guard=1.5 * 0.04, stride=elevation.VISIBILITY_DEFAULTS["stride"], sigmas=0.0)
    assert elevation.visibility_settings(dict(stride=4, end_guard=0.1))["end_guard"] == 0.1
    with pytest.raises(ValueError, match="unknown"):
        elevation.visibility_settings(dict(guard=1))
    with pytest.raises(ValueError, match="True or a dict"):
        elevation.visibility_settings(3)
    v = elevation.visibility_struct(**s, sensor_pos=(0.1, 0.2, 0.3))
    assert v.stride == s["stride"] and v.cleared is None and v.bound_out is None and abs(v.sensor_pos[2] - 0.3) < 1e-7


needs_lib = pytest.mark.skipif(not os.path.exists(elevation.LIB_PATH), reason="libpgtt_elevation.so not built (run __graft_entry__.build())")


@needs_lib
def test_check_visibility_ranges():
    L = elevation.lib()
    good = dict(margin=0.05, end_guard=0.06, stride=2, sigmas=0.0)
    chk = lambda **kw: L.pgtt_elevation_check_visibility(C.byref(elevation.visibility_struct(**dict(good, **kw))))
    assert chk() == 0
    for kw in (dict(margin=1e-6), dict(end_guard=0.0), dict(stride=1), dict(stride=1000), dict(sigmas=3.0), dict(sensor_pos=(-1.0, 2.0, 0.5))):
        assert chk(**kw) == 0, kw
    nan, inf = float("nan"), float("inf")
    for kw in (dict(margin=0.0), dict(margin=-0.05), dict(margin=nan), dict(margin=inf), dict(end_guard=-0.01), dict(end_guard=nan), dict(end_guard=inf),
               dict(stride=0), dict(stride=-2), dict(sigmas=-1.0), dict(sigmas=nan), dict(sigmas=inf), dict(sensor_pos=(nan, 0, 0)), dict(sensor_pos=(0, inf, 0))):
        assert chk(**kw) == -1, kw
        assert L.pgtt_elevation_last_error(), kw
    assert L.pgtt_elevation_check_visibility(None) == -1


@needs_lib
def test_sizeof_exports_and_null_arguments():
    L = elevation.lib()
    assert L.pgtt_elevation_sizeof_visibility() == C.sizeof(elevation.PgttElevationVisibility)
    names = ("pgtt_elevation_check_visibility", "pgtt_elevation_bind_visibility", "pgtt_elevation_visibility", "pgtt_elevation_sizeof_visibility")
    for name in names:
        assert name in elevation.EXPORTS and hasattr(L, name)
    assert L.pgtt_elevation_bind_visibility(None, C.byref(elevation.visibility_struct())) == -1
    assert L.pgtt_elevation_visibility(None, None, 0, 0, None) == -1


def test_the_header_declares_the_block():
    text = open(os.path.join(ROOT, "include", "pgtt_elevation.h")).read()
    for decl in ("int pgtt_elevation_check_visibility(const PgttElevationVisibility*", "int pgtt_elevation_bind_visibility(pgtt_elevation_handle",
                 "int pgtt_elevation_visibility(pgtt_elevation_handle", "int pgtt_elevation_sizeof_visibility(void);"):
        assert decl in text, decl
    body = re.search(r"typedef struct PgttElevationVisibility \{(.*?)\} PgttElevationVisibility;", text, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[\d\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in elevation.PgttElevationVisibility._fields_]
    assert "Visibility clean-up." in text and "floor(x_k * (1 / res))" in text


def _stub_env(lidar_body=None, every=1):
    cc = depth_mod.config_struct(16, 12, 58.0, 0.1, 3.0, 0, (0, 0, 0), (1, 0, 0, 0), every=every)
    env = types.SimpleNamespace(depth_camera=types.SimpleNamespace(config=cc), observation_size={"state": 171}, config=dict(scan_dist_x=0.1, scan_dist_y=0.1),
                                method="pgtt")
    if lidar_body is not None:
        env.lidar_scanner = types.SimpleNamespace(points=object(), config=types.SimpleNamespace(every=1, mount_body=lidar_body, mount_pos=(0.29, 0.0, -0.04)))
    return env


def test_elevation_map_refusals():
    with pytest.raises(ValueError, match="follow_sensor"):
        elevation.ElevationMap(_stub_env(every=3), follow_sensor=True, visibility=True)
    with pytest.raises(ValueError, match="LiDAR on the torso"):
        elevation.ElevationMap(_stub_env(lidar_body=2), source="lidar", visibility=True)
    with pytest.raises(ValueError, match="dense_bound"):
        elevation.ElevationMap(_stub_env(), dense_bound=True)
    with pytest.raises(ValueError, match="unknown"):
        elevation.ElevationMap(_stub_env(), visibility=dict(range=2))


def test_evaluate_parses_the_flag():
    import evaluate
    assert evaluate.elevation_visibility(None) is None and evaluate.elevation_visibility("") is True
    assert evaluate.elevation_visibility("0.08,0.1,4") == dict(margin=0.08, end_guard=0.1, stride=4)
    with pytest.raises(SystemExit):
        evaluate.elevation_visibility("0.08,0.1,x")
    args = evaluate.make_parser().parse_args(["--policy", "policy177", "--elevation", "--elevation_visibility", "0.07"])
    assert evaluate.sensor_kwargs(args)["elevation"] == dict(visibility=dict(margin=0.07))
    with pytest.raises(SystemExit):
        evaluate.sensor_kwargs(evaluate.make_parser().parse_args(["--policy", "policy177", "--elevation_visibility"]))


# ---------------------------------------------------------------- the cap check, before any GPU run
CAMERA = dict(fovy=58.0, near=0.1, far=3.0, mount_pos=(0.30, 0.0, 0.05), mount_quat=tuple(dref.pitch_quat(30.0).astype(np.float32).astype(float)))
# three bases near the start of level4, with a little roll, pitch and yaw: what six random actions leave of the reset pose
BASES = [np.array([0.0137, 0.0249, 0.31, 0.9990, 0.012, -0.021, 0.035]), np.array([0.0537, -0.0351, 0.30, 0.9952, -0.015, 0.018, -0.095]),
         np.array([-1.3063, -0.6951, 0.32, 0.9870, 0.010, 0.025, 0.158])]


@lru_cache(maxsize=None)
def cap_case(width, height, G):
    """the three envs' (qpos, image, ticked and prepared map, origin, cfg) of a case, with the base chosen by rejection - moved by up to a cell
    until the reference alone, at stride 1 and 3, leaves no more than the cap undecided"""
    terrain = np.load(LEVEL4)
    camera, settings = case_setup(dict(CAMERA, width=width, height=height), G)
    cfg = ref_cfg(camera, settings)
    rng = np.random.default_rng(17)
    out, tries = [], 0
    for e, v in enumerate(VARIANTS):
        boxes = dref.terrain_boxes(terrain[v])
        boxes = [b for b in boxes if np.abs(b["c"][:2] - BASES[e][:2]).max() < 5.0]             # the boxes a 3 m camera can see
        while True:
            tries += 1
            q = BASES[e].copy()
            q[0:2] = (q[0:2] + rng.uniform(-RES, RES, 2)).astype(np.float32)
            q = q.astype(np.float32).astype(float)
            img = image(q, cfg, boxes, w=width, h=height)
            t = ref.tick(ref.new_state(G), q, img, cfg, clear=True)
            m = prepare(t["map"], 100 + e)
            worst = 0.0
            for stride in (1, 3):
                sb, sv, _ = vref.shares(vref.visibility((m, t["origin"]), q, cfg, dict(VIS, stride=stride), depth=img, eps=EPS))
                worst = max(worst, sb, sv)
            if worst <= CAP or tries > 40:
                out.append((q, img, m, t["origin"], cfg))
                break
    return out, tries


@pytest.mark.parametrize("width,height,G,stride", CASES)
def test_cap_on_the_reference_alone(width, height, G, stride):
    envs, tries = cap_case(width, height, G)
    nb = nv = n = cleared = 0
    for q, img, m, origin, cfg in envs:
        v = vref.visibility((m, origin), q, cfg, dict(VIS, stride=stride), depth=img, eps=EPS)
        sb, sv, k = vref.shares(v)
        nb += round(sb * k); nv += round(sv * k); n += k; cleared += v["cleared"]
        assert sb <= CAP and sv <= CAP, (sb, sv, k)
    print(f"{width}x{height} G={G} stride={stride}: {tries} poses tried, {n} cells with a bound, undecided bound {nb} ({100 * nb / max(n, 1):.2f} %), "
          f"undecided verdict {nv} ({100 * nv / max(n, 1):.2f} %), cleared {cleared}")
    assert n >= 20 and cleared >= 1, "the case would be vacuous"


# ---------------------------------------------------------------- the jump of the estimate: the GPU test's scenario, chosen here
JUMP = np.float32(3 * RES)                     # an odometry x error of three cells, set by hand between two ticks
JUMP_SIZE = (48, 32)


def jump_scenario():
    """three treads of 0.1 m ahead of a level base, seen by the default camera: -> (qpos fp32 values [7], image [32, 48] fp32, cfg, G)"""
    stairs = [dict(c=np.array([0.70 + 0.3 * k + 1.0, 0.0, 0.05 * (k + 1)]), A=np.eye(3), h=np.array([1.0, 1.5, 0.05 * (k + 1)])) for k in range(3)]
    G = 64
    settings = dict(grid=G, res=RES, alpha=1.0, self_half=(0.45, 0.25, 0.45))
    cfg = ref_cfg(dict(CAMERA), settings)
    q = Q0.astype(np.float32).astype(float)
    return q, image(q, cfg, stairs, w=JUMP_SIZE[0], h=JUMP_SIZE[1]), cfg, G


def test_the_jump_scenario_clears_a_decided_cell():
    """the map of the true pose, then the clean-up under a pose three cells ahead: the old risers stand in rays that now end on the tread behind
    them.  At least one cell is cleared by a decided verdict, and on flat ground ahead of the first riser nothing is"""
    q, img, cfg, G = jump_scenario()
    t = ref.tick(ref.new_state(G), q, img, cfg, clear=True)
    est = q.copy()
    est[0] = float(np.float32(q[0]) + JUMP)
    v = vref.visibility((t["map"], t["origin"]), est, cfg, dict(VIS, stride=1), depth=img, eps=EPS)
    decided = v["clear_sure"] & v["verdict_decided"]
    print(f"jump scenario: {int(decided.sum())} cells cleared by a decided verdict, {int((~v['verdict_decided'] & v['has_bound']).sum())} undecided of {int(v['has_bound'].sum())}")
    assert decided.sum() >= 1
    same = vref.visibility((t["map"], t["origin"]), q, cfg, dict(VIS, stride=1), depth=img, eps=EPS)
    assert same["cleared"] <= decided.sum() // 2                                 # the exact pose contradicts far less
