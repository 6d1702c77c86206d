"""fp64 numpy statement of the variance tick of include/pgtt_elevation.h ("Variance-weighted fusion"): the nine steps of one pgtt_elevation_var()
or pgtt_elevation_var_points() call for ONE env.  Built on tests/elevation_reference.py and tests/elevation_points_reference.py by import: their
tick() states steps 1 - 3 (clear, recentre, validity, unprojection, self filter, window test, maximum) and their sample() step 8; this file adds
the band sums (integer, int64), the measurement, predict and update, and the variance at the scan points.  Next to the results it returns what a
comparison with an fp32 device needs: per cell, whether a pixel is within `eps` of the band's threshold, and whether the gate test is within a
relative 1e-3 of equality.  No GPU, no test module imported."""
import numpy as np

import elevation_points_reference as pref
import elevation_reference as ref

NSCAN = ref.NSCAN
BAND_SCALE = 2.0 ** 18
MAX_BAND = 0.5
DEFAULTS = dict(sigma0=0.005, sigma_rel=0.01, process=1e-6, gate=3.0, band=0.03, max_count=4, var_max=1.0)
GATE_DOUBT = 1e-3


def settings(over=None):
    return {**DEFAULTS, **(over or {})}


def as_device(var):
    """the settings as the device sees them: every real number rounded to fp32, then carried in fp64"""
    out = dict(var)
    for k in ("sigma0", "sigma_rel", "process", "gate", "band", "var_max"):
        out[k] = float(np.float32(out[k]))
    return out


def new_state(G):
    """an empty map: (map [G, G] of NaN, var [G, G] of NaN, origin [2])"""
    return np.full((G, G), np.nan), np.full((G, G), np.nan), np.zeros(2, np.int64)


def tick(state, qpos, source, cfg, var, clear=False, obs=None, points=False, eps=2e-5):
    """one call for one env.  state = (map, var, origin) as new_state / the last tick left it (not modified); cfg: elevation_reference.tick's (alpha is
    not read), or elevation_points_reference.tick's with points=True; source: the image [H, W], or the points [P, 3]; var: the settings
    (settings()).  -> what the base reference's tick returns (map, origin, est, known, touched, scan, valid, point, cell, margin, kept, self_margin,
    obs_out) and var [G, G], est_var [117], n and S [G, G] int64, zmax and m and r [G, G] (NaN where untouched), excluded [G, G] (pixels of the cell
    outside the band), band_doubt [G, G] bool, gate_doubt [G, G] bool, branch [G, G] int8 (0 untouched, 1 a new cell, 2 the gate passed, 3 replaced
    from above, 4 ignored from below)"""
    hmap, vmap, origin = np.array(state[0], float), np.array(state[1], float), np.array(state[2], np.int64)
    G = hmap.shape[0]
    var = as_device(var)
    base_tick = pref.tick if points else ref.tick
    base_cfg = dict(cfg, alpha=1.0)
    source = np.asarray(source)
    # steps 1 - 3 by the base reference.  On a map of zeros with nothing to fuse, what it leaves NaN is what steps 1 and 2 make NaN
    nothing = np.full(source.shape, np.nan) if points else np.full(source.shape, float(np.float32(cfg["far"])))
    stale = np.isnan(base_tick((np.zeros((G, G)), origin), qpos, nothing, base_cfg, clear=clear)["map"])
    hmap[stale] = np.nan
    vmap[stale] = np.nan
    out = base_tick((hmap, origin), qpos, source, base_cfg, clear=False)          # alpha = 1: a touched cell of its map is zmax itself
    touched, origin = out["touched"], out["origin"]
    lo = origin - G // 2
    zmax = np.where(touched, out["map"], np.nan)
    # 4. the band sums over the pixels step 3 admitted
    res = float(np.float32(cfg["res"]))
    rel = out["cell"] - lo
    use = out["kept"] & ((rel >= 0) & (rel < G)).all(1)
    sx, sy = out["cell"][use, 0] % G, out["cell"][use, 1] % G
    dz = zmax[sx, sy] - out["point"][use, 2]
    inband = dz <= var["band"]
    n, S, excluded = np.zeros((G, G), np.int64), np.zeros((G, G), np.int64), np.zeros((G, G), np.int64)
    np.add.at(n, (sx[inband], sy[inband]), 1)
    np.add.at(S, (sx[inband], sy[inband]), np.rint(dz[inband] * BAND_SCALE).astype(np.int64))
    np.add.at(excluded, (sx[~inband], sy[~inband]), 1)
    band_doubt = np.zeros((G, G), bool)
    close = (np.abs(dz - var["band"]) < eps) & (dz > 0)                            # the maximum itself (dz = 0) contributes whatever the band
    band_doubt[sx[close], sy[close]] = True
    # 5. the measurement
    wc = ref.world_cells(origin, G)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(touched, zmax - (S / np.maximum(n, 1)) / BAND_SCALE, np.nan)
        m = np.where(touched & (S == 0), zmax, m)
    qpos = np.asarray(qpos, float)
    cx, cy = (wc[..., 0] + 0.5) * res, (wc[..., 1] + 0.5) * res
    rho2 = (cx - qpos[0]) ** 2 + (cy - qpos[1]) ** 2 + (m - qpos[2]) ** 2
    r = (var["sigma0"] ** 2 + var["sigma_rel"] ** 2 * rho2) / np.minimum(np.maximum(n, 1), int(var["max_count"]))
    # 6. predict
    known = ~np.isnan(hmap)
    vmap[known] = np.fmin(vmap[known] + var["process"], var["var_max"])
    # 7. update
    branch = np.zeros((G, G), np.int8)
    gate_doubt = np.zeros((G, G), bool)
    g2 = var["gate"] ** 2
    for i, j in zip(*np.nonzero(touched)):
        h, v, mm, rr = hmap[i, j], vmap[i, j], m[i, j], r[i, j]
        if np.isnan(h):
            hmap[i, j], vmap[i, j], branch[i, j] = mm, min(rr, var["var_max"]), 1
            continue
        d2, bound = (mm - h) ** 2, g2 * (v + rr)
        gate_doubt[i, j] = abs(d2 - bound) <= GATE_DOUBT * max(d2, bound)
        if d2 <= bound:
            den = v + rr
            k = v / den if den > 0 else 0.0
            hmap[i, j], vmap[i, j], branch[i, j] = h + k * (mm - h), (v * rr / den if den > 0 else 0.0), 2
        elif mm > h:
            hmap[i, j], vmap[i, j], branch[i, j] = mm, min(rr, var["var_max"]), 3
        else:
            branch[i, j] = 4
    # 8. sample, 9. assemble
    sc = ref.sample(hmap, origin, qpos, cfg)
    c = sc["cell"]
    est_var = np.where(sc["known"], vmap[c[:, 0] % G, c[:, 1] % G], var["var_max"])
    out.update(map=hmap, var=vmap, origin=origin, est=sc["est"], known=sc["known"], scan=sc, est_var=est_var, n=n, S=S, zmax=zmax, m=m,
               r=np.where(touched, r, np.nan), excluded=excluded, band_doubt=band_doubt, gate_doubt=gate_doubt, branch=branch)
    if obs is not None:
        r0 = cfg.get("scan_row0", 38)
        out["obs_out"] = np.concatenate([obs[:r0], sc["est"], obs[r0 + NSCAN:]])
    return out


def doubtful_cells(out, res, eps):
    """the world cells an fp32 device may legitimately decide differently in this tick: elevation_reference.doubtful_cells (a pixel within eps of a
    cell border or of the self box), the cells with a pixel within eps of the band's threshold, and the cells whose gate test is within a relative
    1e-3 of equality -> a set of (ix, iy)"""
    cells = ref.doubtful_cells(out, res, eps)
    wc = ref.world_cells(out["origin"], out["map"].shape[0])
    cells.update(map(tuple, wc[out["band_doubt"] | out["gate_doubt"]]))
    return cells
