"""fp64 numpy statement of pgtt_elevation_points() (include/pgtt_elevation.h) for ONE env: the six steps of tests/elevation_reference.py with
step 3 fed by world points instead of pixels.  It reuses that reference's cell, sample, border_margin and world_cells, returns the same
dictionary - `valid` is "every coordinate finite" here - and so takes the same doubtful_cells rule: what a comparison with the fp32 device needs
to know which cells a rounding error could have changed.  The device and this reference read the same fp32 points, so only a cell border or the
self box can put a cell in doubt.  No GPU, no test module imported."""
import numpy as np

import depth_reference as dref
import elevation_reference as eref
from elevation_reference import border_margin, cell, doubtful_cells, new_state, sample, world_cells  # noqa: F401  (the rules this one shares)

NSCAN = eref.NSCAN


def tick(state, qpos, points, cfg, clear=False, obs=None):
    """one call for one env.  state = (map, origin) as new_state / the last tick left it (not modified); cfg = dict(res, alpha, self_half[,
    scan_dist_x, scan_dist_y, scan_row0]) - no camera; points [P, 3] world points, NaN or non-finite rows are skipped.
    -> elevation_reference.tick's dictionary, per point where that one is per pixel"""
    hmap, origin = np.array(state[0], float), np.array(state[1], np.int64)
    cfg = eref.as_device(cfg)
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
    # 3. tick maximum over the points
    pts = np.asarray(points, float).reshape(-1, 3)
    valid = np.isfinite(pts).all(1)
    p = np.where(valid[:, None], pts, 0.0)
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
