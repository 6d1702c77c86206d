"""The three ray casters (libpgtt_lidar.so, libpgtt_depth.so, libpgtt_render.so) at the edges of their primitives, on the crafted scenes of
tests/raycast_edge_cases.py against its fp64 primitives: capsules seen along their axis (angles from 0 to 0.3 rad, from either end, at 0 to 1.1
radii from the axis), spheres that hold the origin, lie behind it or sit 2.9 m away, camera rays with exact zero components on an aligned box, a
ray origin inside a box, and primitives at the margin of the depth camera's cone cull and of both sensors' reach.  The bars are those of
test_gpu_lidar.py, test_gpu_depth.py and test_gpu_render.py: a hit within 1e-4 relative, a miss exactly `far` (the renderer: inf and SEG_SKY).
No case is skipped: tests/test_raycast_edge_cases.py shows on the CPU that each is unambiguous by the reference alone.
The LiDAR does not get one handle per capsule family with a few hundred rays: a ray from a fixed origin meets a given capsule at one angle and offset
only, so every case needs a capsule of its own, and a handle takes 32 geoms.  The same 400 cases go through 16 handles of one 42-ray pattern
(32 general directions, the six coordinate axes, four rays next to +x for the reach cases), each capsule on a ray of its own."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_edge_cases as rc  # noqa: E402
from test_gpu_depth import _env, _set_qpos  # noqa: E402
from test_raycast_edge_cases import scenes  # noqa: E402

from phase_guided_terrain_traversal_amd import depth, lidar, render  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-4
FAR32 = np.float32(rc.FAR)
CAMERA = render.Camera("fixed", target=(1.0, 0.0, 4.0), distance=1.0, azimuth=0.0, elevation=0.0, fovy=rc.FOVY)       # at ORIGIN, looking along +x


@pytest.fixture(scope="module")
def env():
    """one env of flat_terrain, the base at ORIGIN with the identity quaternion: 4 m above the floor"""
    e, _ = _env("flat_terrain", 1)
    q = np.zeros(19, np.float32)
    q[0:3], q[3] = rc.ORIGIN, 1.0
    _set_qpos(e, 0, q)
    yield e
    e.close()


# ---------------------------------------------------------------- one scene through one library -> what it wrote for every ray
def cast_lidar(env, sc):
    lid = lidar.LidarScanner(env, near=rc.NEAR, far=rc.FAR, pattern=rc.lidar_pattern(), geoms=sc["geoms"], points=False)
    lid.set_terrain(sc.get("terrain"))
    got = lid.tick(force=True)[0].cpu().numpy()
    lid.close()
    return got


def cast_depth(env, sc):
    cam = depth.DepthCamera(env, rc.W, rc.H, rc.FOVY, rc.NEAR, rc.FAR, geoms=sc["geoms"])
    cam.set_terrain(sc.get("terrain"))
    got = cam.tick(force=True)[0].cpu().numpy().reshape(-1)
    cam.close()
    return got


def cast_render(env, sc):
    r = render.Renderer(env, rc.W, rc.H, geoms=sc["geoms"])
    r.set_terrain(sc.get("terrain"))
    out = r.render([0], camera=CAMERA, depth=True, segmentation=True)
    got = out["depth"][0].cpu().numpy().reshape(-1), out["segmentation"][0].cpu().numpy().reshape(-1)
    r.close()
    return got


def errors(sensor, env, sc):
    """-> (relative error of each checked ray that the reference sees inside the sensor's reach [n], or nan; wrong [n]: a hit beyond the bar, a
    miss that is not exactly `far` (the renderer: not inf, or another segment than the reference's))"""
    chk = np.asarray(sc["check"])
    if sensor == "lidar":
        dirs = rc.lidar_rays()
        e, got = rc.expected(sc, dirs), cast_lidar(env, sc)[chk]
        want = e["t"][chk]
    else:
        dirs = rc.pixel_rays()
        e = rc.expected(sc, dirs)
        want = (e["t"] * dirs[:, 0])[chk]                                  # depth along the optical axis
        if sensor == "depth":
            got = cast_depth(env, sc)[chk]
        else:
            got, seg = (a[chk] for a in cast_render(env, sc))
    if sensor == "render":                                                # no reach: the floor below the horizon is part of the expectation
        hit = e["seg"][chk] != rc.SEG_SKY
        wrong = seg != e["seg"][chk]
        wrong[~hit] |= got[~hit] != np.inf
    else:
        hit = want < rc.FAR
        wrong = np.zeros(len(chk), bool)
        wrong[~hit] = got[~hit] != FAR32
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(hit, np.abs(got.astype(np.float64) / np.where(hit, want, 1.0) - 1), np.nan)
    wrong[hit] |= ~(rel[hit] < BAR)
    return rel, wrong


# ---------------------------------------------------------------- 1. the capsule sweep
@pytest.mark.parametrize("sensor", ["lidar", "depth", "render"])
def test_capsule_sweep(env, sensor):
    """400 capsules per library, each on a ray of its own: hits within 1e-4 relative and of the crafted geom, misses exactly `far` (sky).  The
    capsules along coordinate axes have a = |ba x d|^2 = 0 exactly; those at 0 and 1e-6 rad have an a at rounding-noise level, which may even come
    out negative: the kernels' `a <= 1e-12 baba` rule, decided before the discriminant (pgtt_raycast.hip.h), is what these cases hold."""
    sweep = scenes()["lidar" if sensor == "lidar" else "camera"][0]
    worst, bad, n = {}, [], 0
    for sc in sweep:
        rel, wrong = errors(sensor, env, sc)
        for c, r, w in zip(sc["cases"], rel, wrong):
            n += 1
            for key in (c["fam"], f"angle {c['asked']:g}"):
                lo, nbad = worst.get(key, (0.0, 0))
                worst[key] = (max(lo, 0.0 if np.isnan(r) else float(r)), nbad + int(w))
            if w:
                bad.append(f"{c['fam']} r={c['prim']['r']:.3f} angle={c['theta']:.3e} k={c['k']} end={c['end']} dist={c['dist']} rel={r:.3e}")
    for key, (r, nbad) in worst.items():
        print(f"{sensor} {key}: worst relative error {r:.3e} ({r / BAR:.4f} of the bar), {nbad} wrong")
    assert n == 400
    assert not bad, (len(bad), bad[:12])


# ---------------------------------------------------------------- 2. spheres, boxes, the culls
@pytest.mark.parametrize("sensor", ["lidar", "depth", "render"])
def test_spheres_boxes_and_culls(env, sensor):
    """every scene besides the sweep: for the renderer, which culls nothing and has no reach, the spheres and the boxes"""
    if sensor == "lidar":
        todo = scenes()["lidar"][1]
    else:
        _, shared, cull = scenes()["camera"]
        todo = shared + (cull if sensor == "depth" else [])
    bad = []
    for sc in todo:
        rel, wrong = errors(sensor, env, sc)
        hits = int(np.isfinite(rel).sum())
        top = float(np.nanmax(rel)) if hits else 0.0
        print(f"{sensor} {sc['name']}: {len(rel)} rays, {hits} hits, worst relative error {top:.3e} ({top / BAR:.4f} of the bar), {int(wrong.sum())} wrong")
        bad += [f"{sc['name']}: ray {ray} rel={r:.3e}" for ray, r, w in zip(sc["check"], rel, wrong) if w]
    assert len(todo) == {"lidar": 6, "depth": 9, "render": 4}[sensor]
    assert not bad, (len(bad), bad[:12])
    torch.cuda.synchronize()
