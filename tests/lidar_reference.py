"""fp64 numpy statement of include/pgtt_lidar.h on top of tests/depth_reference.py: the sensor pose from the env's qpos, the world directions of
a pattern, depth_reference.cast, the clamp, the point rule, and the Philox noise on stream 33.  Also the ambiguity mask of a scan, computed from
this reference alone: a ray is ambiguous when turning its direction by +-5e-4 rad about either perpendicular changes which primitive is nearest,
when its two nearest candidates are within 1e-4 relative of each other, or when its hit is within 1e-4 relative of `far`.  No GPU, no test
module imported."""
import numpy as np

import depth_reference as dref

RS_LIDAR = 33                         # include/pgtt_lidar.h
AMB_TURN, AMB_TIE = 5e-4, 1e-4


def spherical_pattern(n_az, n_el, az_deg, el_deg):
    """lidar.spherical_pattern, stated again: ray r = a * n_el + k, azimuths at cell centres, elevations on the closed interval"""
    d = np.zeros((n_az, n_el, 3))
    for a in range(n_az):
        az = np.radians(az_deg[0] + (a + 0.5) * (az_deg[1] - az_deg[0]) / n_az)
        for k in range(n_el):
            el = np.radians(el_deg[0] + k * (el_deg[1] - el_deg[0]) / (n_el - 1) if n_el > 1 else 0.5 * (el_deg[0] + el_deg[1]))
            d[a, k] = [np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)]
    return d.reshape(-1, 3)


def unit_rows(dirs):
    """what pgtt_lidar_create keeps: each row normalised in double, rounded to fp32"""
    d = np.asarray(np.asarray(dirs, np.float32), np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)


def sensor_pose(xpos, xquat, mount_body=0, mount_pos=(0, 0, 0), mount_quat=(1, 0, 0, 0)):
    """sensor pose = body pose * mount pose -> (origin [3], rotation [3, 3]: columns = the sensor's axes in world coordinates)"""
    mq = np.asarray(mount_quat, float) / np.linalg.norm(mount_quat)
    return xpos[mount_body] + dref.qmat(xquat[mount_body]) @ np.asarray(mount_pos, float), dref.qmat(dref.qmul(xquat[mount_body], mq))


def _perpendiculars(d):
    """two unit vectors perpendicular to each row of d and to each other"""
    helper = np.where((np.abs(d[:, 2]) < 0.9)[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    p = np.cross(d, helper)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return p, np.cross(d, p)


def scan(o, R, dirs, near, far, boxes=(), geoms=()):
    """o, R: the sensor pose; dirs [P, 3] unit rows in the sensor frame -> dict(range [P] clamped to [near, far] with far on a miss, id [P],
    points [P, 3] (NaN where the range is not strictly inside (near, far)), dirs [P, 3] world directions, ambiguous [P])"""
    d = np.asarray(dirs, float) @ R.T
    t, ids, second = dref.cast(o, d, boxes, geoms)
    rng = np.clip(np.where(ids >= 0, t, np.inf), near, far)
    amb = (ids >= 0) & np.isfinite(second) & (second <= t * (1 + AMB_TIE))
    amb |= (ids >= 0) & (np.abs(t - far) <= AMB_TIE * far)
    p, q = _perpendiculars(d)
    for axis in (p, q):
        for s in (AMB_TURN, -AMB_TURN):
            dd = d * np.cos(s) + axis * np.sin(s)
            amb |= dref.cast(o, dd, boxes, geoms)[1] != ids
    pts = np.where(((rng > near) & (rng < far))[:, None], o[None] + rng[:, None] * d, np.nan)
    return dict(range=rng, id=ids, points=pts, dirs=d, ambiguous=amb, origin=o)


def env_scan(model, qpos, cfg, dirs, terrain_v=None, geoms=None, params=None, e=0):
    """the scan of one env: cfg = dict(near, far[, mount_body, mount_pos, mount_quat]); dirs: the pattern as given to the library (normalised
    here as it is there); terrain_v: [B, 10] rows of the env's variant or None; geoms: the robot primitive dicts when the robot is in the scene"""
    xpos, xquat = dref.body_poses(model, qpos, params, e)
    o, R = sensor_pose(xpos, xquat, cfg.get("mount_body", 0), cfg.get("mount_pos", (0, 0, 0)), cfg.get("mount_quat", (1, 0, 0, 0)))
    return scan(o, R, unit_rows(dirs), cfg["near"], cfg["far"], dref.terrain_boxes(terrain_v) if terrain_v is not None else (),
                dref.place_geoms(xpos, xquat, geoms) if geoms else ())


def kinds(r, far):
    """the return kinds a scan holds: box, floor, far, geom"""
    out = set()
    inside = r["range"] < far
    if ((r["id"] >= dref.ID_BOX) & (r["id"] < dref.ID_GEOM) & inside).any():
        out.add("box")
    if ((r["id"] == dref.ID_PLANE) & inside).any():
        out.add("floor")
    if ((r["id"] < 0) | ~inside).any():
        out.add("far")
    if ((r["id"] >= dref.ID_GEOM) & inside).any():
        out.add("geom")
    return out


# ---------------------------------------------------------------- the sensor noise: the camera's formulas on stream 33, ray r for pixel p
def noise_uniforms(seed, env_id, counter, nrays):
    """u_k = uniform(seed, env id, (uint32) counter, RS_LIDAR, 4 r + k), k = 0 .. 2 -> [nrays, 3] exact multiples of 2^-24"""
    ctr = np.zeros((nrays, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = env_id & 0xFFFFFFFF, counter & 0xFFFFFFFF, RS_LIDAR, np.arange(nrays)
    w = dref.philox4x32_10((seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), ctr)
    return (w[:, :3] >> 8).astype(np.float64) / 16777216.0


def apply_noise(rng, near, far, sigma, dropout, seed, env_id, counter):
    """rng [R] noise-free clamped ranges -> (noisy ranges, dropped mask, u_0)"""
    u = noise_uniforms(seed, env_id, counter, rng.size)
    dropped = u[:, 0] < np.float64(np.float32(dropout))
    z = np.sqrt(-2 * np.log(1 - u[:, 1])) * np.cos(2 * np.pi * u[:, 2])
    out = np.clip(rng * (1 + np.float64(np.float32(sigma)) * z), near, far)
    return np.where(dropped, far, out), dropped, u[:, 0]
