"""fp64 numpy statement of the block "Visibility clean-up" of include/pgtt_elevation.h: one pgtt_elevation_visibility() call for ONE env - skip, rays,
samples, clean - on the geometry of tests/elevation_reference.py (unproject, cell, border_margin, world_cells) and tests/depth_reference.py.

The definition is by sampling, so a rounding error of an fp32 device can move a sample across a cell border, across the end guard, or change
whether its ray is cast at all, and the bound of a cell is a minimum: one such sample can change it by far more than a rounding error.  The
reference therefore returns TWO bounds per cell:
    bound_sure   the minimum over the samples that are not doubtful
    bound_any    the minimum over the sure and the doubtful samples; a doubtful sample counts for every cell it could fall into
A sample is doubtful when
    - it lies within `eps` of a cell border (it then counts for the cells of (x +- eps, y +- eps)), or
    - its r_k lies within eps of Lh - end_guard (the last sample of a ray, made or not), or
    - its ray's end point is within eps of a validity limit (0 < |d - near| < eps or 0 < |d - far| < eps: a depth that IS a limit, as a clamped
      pixel reads, is compared exactly on both sides) or within eps of changing sides of the self box.
A cell's bound is DECIDED when bound_sure == bound_any (both none, or the same number).  Its verdict is DECIDED when both bounds give the same
verdict and |h - bound - margin| exceeds the bar 2e-5 (1 + |h|) for both.  No GPU, no test module imported."""
import numpy as np

import depth_reference as dref
import elevation_reference as ref

BAR = 2e-5
ORIGIN_CLAMP = 1 << 30


def as_device(vis):
    """the settings as the device sees them: fp32 values carried in fp64"""
    out = dict(vis)
    for k in ("margin", "end_guard", "sigmas"):
        out[k] = float(np.float32(out.get(k, 0.0)))
    out["sensor_pos"] = np.asarray(out.get("sensor_pos", (0, 0, 0)), np.float32).astype(float)
    out["stride"] = int(out.get("stride", 1))
    return out


def selected_pixels(H, W, stride):
    """flat indices of the pixels that cast a ray: i % stride == 0 and j % stride == 0, row-major"""
    i, j = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    return (i * W + j).reshape(-1)


def rays(qpos, cfg, vis, depth=None, points=None, eps=BAR):
    """step 2 -> (s [3], p [R, 3] the end points of the rays that are cast or in doubt, doubt [R] bool: whether the ray is cast at all is in doubt)"""
    qpos = np.asarray(qpos, float)
    q = qpos[3:7] / np.linalg.norm(qpos[3:7])
    R = dref.qmat(q)
    half = np.asarray(cfg.get("self_half", (0, 0, 0)), float)
    if points is None:
        s = ref.camera_pose(qpos, cfg["mount_pos"], cfg["mount_quat"])[0]
        H, W = depth.shape
        sel = selected_pixels(H, W, vis["stride"])
        d = np.asarray(depth, float).reshape(-1)[sel]
        with np.errstate(invalid="ignore"):
            valid = (d > cfg["near"]) & (d < cfg["far"])
            lim_doubt = ((np.abs(d - cfg["near"]) < eps) & (d != cfg["near"])) | ((np.abs(d - cfg["far"]) < eps) & (d != cfg["far"]))
        p = ref.unproject(qpos, np.where(np.isfinite(np.asarray(depth, float)), depth, 1.0), cfg)[sel]
    else:
        s = qpos[0:3] + R @ vis["sensor_pos"]
        p = np.asarray(points, float)[::vis["stride"]]
        valid = np.isfinite(p).all(1)
        lim_doubt = np.zeros(len(p), bool)
        p = np.where(valid[:, None], p, 0.0)
    if half.any():
        over = np.abs((p - qpos[0:3]) @ R) - half
        inside = (over <= 0).all(1)
        self_margin = np.where(inside, (-over).min(1), over.max(1))
    else:
        inside, self_margin = np.zeros(len(p), bool), np.full(len(p), np.inf)
    cast = valid & ~inside
    doubt = (valid | lim_doubt) & ((self_margin < eps) | lim_doubt)
    keep = cast | doubt
    return s, p[keep], doubt[keep]


def visibility(state, qpos, cfg, vis, depth=None, points=None, var=None, skip=False, eps=BAR):
    """one call for one env.  state = (map [G, G], origin [2]) as the last tick left it (not modified); cfg: elevation_reference.tick's; vis =
    dict(margin, end_guard, stride, sigmas[, sensor_pos]); depth [H, W] or points [P, 3] (world); var [G, G] or None.
    -> dict(bound_sure, bound_any [G, G] (NaN = none), clear_sure, clear_any [G, G] bool, bound_decided, verdict_decided [G, G] bool,
            has_bound [G, G] bool (bound_any is there), map, var (cleaned by the SURE verdict), cleared (its count), samples (the number made))"""
    hmap, origin = np.array(state[0], float), np.clip(np.array(state[1], np.int64), -ORIGIN_CLAMP, ORIGIN_CLAMP)
    cfg, vis = ref.as_device(cfg), as_device(vis)
    G, res = hmap.shape[0], float(cfg["res"])
    none = np.full((G, G), np.inf)
    out_var = None if var is None else np.array(var, float)
    if skip:
        f = np.zeros((G, G), bool)
        return dict(bound_sure=np.full((G, G), np.nan), bound_any=np.full((G, G), np.nan), clear_sure=f, clear_any=f, bound_decided=~f,
                    verdict_decided=~f, has_bound=f, map=hmap, var=out_var, cleared=0, samples=0)
    s, p, ray_doubt = rays(qpos, cfg, vis, depth, points, eps)
    lo = origin - G // 2
    sure, anyb = none.copy(), none.copy()
    nsamp = 0
    if len(p):
        dxy = p[:, :2] - s[:2]
        Lh = np.hypot(dxy[:, 0], dxy[:, 1])
        lim = Lh - vis["end_guard"]
        rk = (np.arange(2 * G) + 0.5) * res                                       # [K]
        with np.errstate(invalid="ignore", divide="ignore"):
            u = np.where(Lh[:, None] > 0, dxy / Lh[:, None], 0.0)
            uz = np.where(Lh > 0, (p[:, 2] - s[2]) / Lh, 0.0)
        made = rk[None] <= lim[:, None]
        end_doubt = np.abs(rk[None] - lim[:, None]) < eps
        cand = (made | end_doubt) & (Lh[:, None] > 0)
        ri, ki = np.nonzero(cand)
        xy = s[None, :2] + rk[ki, None] * u[ri]
        z = s[2] + uz[ri] * rk[ki]
        bm = ref.border_margin(xy, res)
        doubtful = ray_doubt[ri] | end_doubt[ri, ki] | (bm < eps)
        nsamp = int((made[ri, ki] & ~ray_doubt[ri]).sum())

        def lower(b, xy_, z_):
            c = ref.cell(xy_, res)
            rel = c - lo
            inw = ((rel >= 0) & (rel < G)).all(1) & ~np.isnan(z_)
            np.minimum.at(b, (c[inw, 0] % G, c[inw, 1] % G), z_[inw])

        lower(sure, xy[~doubtful], z[~doubtful])
        lower(anyb, xy[~doubtful], z[~doubtful])
        for dx in (-eps, eps):
            for dy in (-eps, eps):
                lower(anyb, xy[doubtful] + np.array([dx, dy]), z[doubtful])
    has_sure, has_any = sure < np.inf, anyb < np.inf
    h = hmap if var is None else hmap - vis["sigmas"] * np.sqrt(out_var)
    with np.errstate(invalid="ignore"):
        clear_sure = has_sure & (h > sure + vis["margin"])
        clear_any = has_any & (h > anyb + vis["margin"])
        bar = BAR * (1 + np.abs(h))
        far_sure = ~has_sure | np.isnan(h) | (np.abs(h - sure - vis["margin"]) > bar)
        far_any = ~has_any | np.isnan(h) | (np.abs(h - anyb - vis["margin"]) > bar)
    bound_decided = (has_sure == has_any) & (~has_any | (sure == anyb))
    verdict_decided = (clear_sure == clear_any) & far_sure & far_any
    hmap[clear_sure] = np.nan
    if out_var is not None:
        out_var[clear_sure] = np.nan
    return dict(bound_sure=np.where(has_sure, sure, np.nan), bound_any=np.where(has_any, anyb, np.nan), clear_sure=clear_sure, clear_any=clear_any,
                bound_decided=bound_decided, verdict_decided=verdict_decided, has_bound=has_any, map=hmap, var=out_var, cleared=int(clear_sure.sum()),
                samples=nsamp)


def shares(out):
    """(share of the cells with a bound whose bound is undecided, ... whose verdict is undecided, the number of cells with a bound)"""
    n = int(out["has_bound"].sum())
    return (int((out["has_bound"] & ~out["bound_decided"]).sum()) / max(n, 1), int((out["has_bound"] & ~out["verdict_decided"]).sum()) / max(n, 1), n)
