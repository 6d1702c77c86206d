"""fp64 numpy statement of include/pgtt_elevation.h: the six steps of one pgtt_elevation() call for ONE env - clear, recentre, tick maximum, fuse,
sample, assemble - on the pixel geometry and the camera pose of tests/depth_reference.py.  Next to the results it returns, for every pixel and for
every scan point, the distance of the point from the nearest cell border, and for every pixel how far it is from changing sides of the self-filter
box: what a comparison with an fp32 device needs to know which cells a rounding error could have changed.  No GPU, no test module imported."""
import numpy as np

import depth_reference as dref

NSCAN, SCAN_H, SCAN_W = 117, 13, 9


def as_device(cfg):
    """the config as the device sees it: every real number rounded to fp32 (a clamped pixel reads exactly fp32(near): `near < d` must be decided
    against that value), then carried in fp64"""
    out = dict(cfg)
    for k in ("fovy", "near", "far", "res", "alpha", "scan_dist_x", "scan_dist_y"):
        if k in out:
            out[k] = float(np.float32(out[k]))
    for k in ("mount_pos", "mount_quat", "self_half"):
        if k in out:
            out[k] = np.asarray(out[k], np.float32).astype(float)
    return out


def new_state(G):
    """an empty map: (map [G, G] of NaN, origin [2])"""
    return np.full((G, G), np.nan), np.zeros(2, np.int64)


def camera_pose(qpos, mount_pos, mount_quat):
    """base pose (qpos[0:7], the quaternion normalised) * mount pose -> (pos, fwd, right, up), depth_reference.camera_basis with the torso alone"""
    q = np.asarray(qpos[3:7], float)
    return dref.camera_basis(np.asarray(qpos[0:3], float)[None], (q / np.linalg.norm(q))[None], 0, mount_pos, mount_quat)


def cell(x, res):
    return np.floor(np.asarray(x, float) / res).astype(np.int64)


def border_margin(xy, res):
    """distance (m) of points [..., 2] from the nearest cell border"""
    f = xy / res - np.floor(xy / res)
    return (np.minimum(f, 1 - f) * res).min(-1)


def unproject(qpos, depth, cfg):
    """every pixel's world point [H * W, 3] (depth = distance along the optical axis): cam_pos + d (fwd + u right + v up)"""
    pos, fwd, right, up = camera_pose(qpos, cfg["mount_pos"], cfg["mount_quat"])
    H, W = depth.shape
    d = dref.camera_rays(fwd, right, up, cfg["fovy"], W, H)                   # unit directions; d . fwd = 1 / |fwd + u right + v up|
    return pos[None] + np.asarray(depth, float).reshape(-1, 1) * d / (d @ fwd)[:, None]


def yaw_of(qpos):
    w, x, y, z = np.asarray(qpos[3:7], float) / np.linalg.norm(qpos[3:7])
    return np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


def scan_points(qpos, sdx=0.1, sdy=0.1):
    """[117, 2] world xy of the observe kernel's scan grid, point i = 9 r + c"""
    r, c = np.divmod(np.arange(NSCAN), SCAN_W)
    ox, oy = ((SCAN_H - 1) * 0.5 - r) * sdx, ((SCAN_W - 1) * 0.5 - c) * sdy
    yaw = yaw_of(qpos)
    cy, sy = np.cos(yaw), np.sin(yaw)
    return np.stack([qpos[0] + ox * cy - oy * sy, qpos[1] + ox * sy + oy * cy], 1)


def sample(hmap, origin, qpos, cfg):
    """step 5 -> dict(est [117], known [117] bool, z, xy [117, 2], cell [117, 2], margin [117])"""
    cfg = as_device(cfg)
    G, res = hmap.shape[0], cfg["res"]
    xy = scan_points(qpos, cfg.get("scan_dist_x", 0.1), cfg.get("scan_dist_y", 0.1))
    c = cell(xy, res)
    rel = c - (origin - G // 2)
    inside = ((rel >= 0) & (rel < G)).all(1)
    z = np.where(inside, hmap[c[:, 0] % G, c[:, 1] % G], np.nan)
    known = inside & ~np.isnan(z)
    if known.any():
        zmin = z[known].min()
        z = np.where(known, z, zmin)
    else:
        zmin, z = 0.0, np.zeros(NSCAN)
    return dict(est=z - zmin, known=known, z=z, xy=xy, cell=c, margin=border_margin(xy, res))


def tick(state, qpos, depth, cfg, clear=False, obs=None):
    """one call for one env.  state = (map, origin) as new_state / the last tick left it (not modified); cfg = dict(fovy, near, far, mount_pos,
    mount_quat, res, alpha, self_half[, scan_dist_x, scan_dist_y, scan_row0]); depth [H, W].
    -> dict(map, origin, est, known, obs_out (when obs is given), touched [G, G] bool (slots step 3 reached), scan (sample()'s dict), and per pixel:
       valid [P] (near < d < far), point [P, 3], cell [P, 2], margin [P] (distance from the nearest cell border), kept [P] (valid, outside the
       self box), self_margin [P] (the L-infinity distance by which the point would have to move to change sides of the self box; inf without one))"""
    hmap, origin = np.array(state[0], float), np.array(state[1], np.int64)
    cfg = as_device(cfg)
    G, res, alpha = hmap.shape[0], float(cfg["res"]), float(cfg["alpha"])
    qpos = np.asarray(qpos, float)
    # 1. clear, 2. recentre
    new_origin = cell(qpos[0:2], res)
    if clear:
        hmap[:] = np.nan
    else:
        s = np.arange(G)
        for ax in (0, 1):
            lo_new, lo_old = new_origin[ax] - G // 2, origin[ax] - G // 2
            stale = (lo_new + (s - lo_new) % G) != (lo_old + (s - lo_old) % G)
            if ax == 0:
                hmap[stale, :] = np.nan
            else:
                hmap[:, stale] = np.nan
    origin = new_origin
    lo = origin - G // 2
    # 3. tick maximum
    d = np.asarray(depth, float).reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = (d > cfg["near"]) & (d < cfg["far"])
    p = unproject(qpos, np.where(valid, d, 1.0).reshape(depth.shape), cfg)
    half = np.asarray(cfg.get("self_half", (0, 0, 0)), float)
    q = qpos[3:7] / np.linalg.norm(qpos[3:7])
    local = (p - qpos[0:3]) @ dref.qmat(q)                                     # R^T (p - b)
    if half.any():
        over = np.abs(local) - half                                             # > 0 on an axis that puts the point outside
        inside_box = (over <= 0).all(1)
        self_margin = np.where(inside_box, (-over).min(1), over.max(1))
    else:
        inside_box, self_margin = np.zeros(len(p), bool), np.full(len(p), np.inf)
    kept = valid & ~inside_box
    c = cell(p[:, :2], res)
    rel = c - lo
    inwin = ((rel >= 0) & (rel < G)).all(1)
    m = np.full((G, G), -np.inf)
    use = kept & inwin
    np.maximum.at(m, (c[use, 0] % G, c[use, 1] % G), p[use, 2])
    touched = np.isfinite(m)
    # 4. fuse
    hmap[touched] = np.where(np.isnan(hmap[touched]), m[touched], hmap[touched] + alpha * (m[touched] - hmap[touched]))
    # 5. sample, 6. assemble
    sc = sample(hmap, origin, qpos, cfg)
    out = dict(map=hmap, origin=origin, est=sc["est"], known=sc["known"], touched=touched, scan=sc, valid=valid, point=p, cell=c,
               margin=border_margin(p[:, :2], res), kept=kept, self_margin=self_margin)
    if obs is not None:
        r0 = cfg.get("scan_row0", 38)
        out["obs_out"] = np.concatenate([obs[:r0], sc["est"], obs[r0 + NSCAN:]])
    return out


def world_cells(origin, G):
    """[G, G, 2]: the world cell each slot holds under the window centred at `origin`"""
    s = np.arange(G)
    lo = np.asarray(origin, np.int64) - G // 2
    wx, wy = lo[0] + (s - lo[0]) % G, lo[1] + (s - lo[1]) % G
    return np.stack(np.broadcast_arrays(wx[:, None], wy[None, :]), -1)


def doubtful_cells(out, res, eps):
    """the world cells a device whose points are within `eps` of this reference's could have filled differently in this tick: for every valid
    pixel within eps of a cell border, or within eps of changing sides of the self box, the cells of (x +- eps, y +- eps) -> a set of (ix, iy)"""
    res = float(np.float32(res))
    near = out["valid"] & ((out["margin"] < eps) | (out["self_margin"] < eps))
    cells = set()
    xy = out["point"][near, :2]
    for dx in (-eps, eps):
        for dy in (-eps, eps):
            cells.update(map(tuple, cell(xy + np.array([dx, dy]), res)))
    return cells
