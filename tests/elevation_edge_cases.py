"""The elevation map's decisions at their exact edges (include/pgtt_elevation.h): an fp32 twin of the contract's comparisons and builders of named
case families whose inputs sit ON those comparisons.  Pure numpy: no torch, no GPU.  tests/test_elevation_edge_cases.py shows on the CPU that the
cases are what they claim; tests/test_gpu_elevation_edges.py holds the kernels to them.

The twin.  The point-cloud entries read the fp32 world points as they are, and with the base at the identity quaternion (or the half-turn about z,
or a positive or negative multiple of either) the base rotation is exactly +-1 and 0, so every decision of a tick is one or two IEEE operations:
    cell(x, res)      = floor(fl32(x) / fl32(res)), clamped to +-1e9       the tick, the origin, the scan ("floor(x / res)")
    cell_recip(x,res) = floor(fl32(x) * fl32(1 / fl32(res)))               the visibility samples alone ("NOT the tick's floor(x / res)")
    the window test and the slot (ix mod G, iy mod G); the recentre by "differs from its world cell under the old window"
    the key order of the maximum (-0 < +0, the result one of the inputs bit for bit)
    the self box   |fl32(p - b)| <= half on all three axes
    the band       dz = fl32(zmax - z) <= band, q = rint(dz * 2^18), m = fl32(zmax - fl32(fl32(S) / fl32(n)) * 2^-18), m = zmax when S == 0
    r = sigma0^2 / min(n, max_count) with sigma_rel = 0; predict v = min(fl32(v + process), var_max)
    the gate       fl32(d * d) <= fl32(gate^2 * fl32(v + r)), d = fl32(m - h), and its two failing branches
    the scan       wx = fl32(bx + fl32((6 - r) * sdx)) at yaw 0, est = fl32(z - zmin)
    visibility     r_k = fl32((k + 0.5) * res) <= fl32(Lh - end_guard), k < 2 G; the sample by one fused multiply-add per coordinate;
                   the verdict t > fl32(bound + margin), t = h or fl32(h - fl32(sigmas * sqrt(v)))
It is written from the header, not from the kernel.  Where an expression's bits would depend on whether a multiply-add is contracted (the alpha fuse
h + alpha (m - h), the Kalman update h + k (m - h), h - sigmas sqrt(v)), the twin also checks that the product is exact in fp32 - then every
evaluation order gives the same bits - and reports `exact`; a case that is held bit for bit has exact == True (dyadic values), any other case is
held to the project's bars, 2e-5 (1 + |ref|) on heights and 1e-4 relative on variances, against the fp64 references of tests/.

Sentences of the header this twin first misread, and how they are read now.  "skipped when p, expressed in the base frame, lies in the box |x| <=
self_half[0]": the edge is in fl32(p - b), not in p.  The last point inside is the last p whose difference ROUNDS to the half extent, which for a
base near 0.5 and a face near 0 is several floats beyond b + half; a case that put the point at fl32(b + half) and called its neighbour "outside" was
wrong, not the kernel.  The same holds for the gate (the last m whose fl32(m - h) is d) and for a ray's length (the last end whose fl32(px - sx) is Lh).

Not in the contract, so not a case here (and the current behaviour is not pinned): a zero base quaternion.

A case is dict(name, family, S = settings, ticks = [...], edges = [...], mode).  A tick is dict(op = "tick" | "hold" | "clean", qpos [7], points [P, 3]
or image [H, W], clear, origin_in (an origin the host writes first) and obs).  expected(case) -> per tick, {field: (mark, array)} with mark "bits" or
"bar".  An edge is (tick, "points" | "qpos", index, axis, direction): the named fp32 input sits on a comparison, and its neighbouring float in
`direction` (+1 up, -1 down) is on the other side.  No case carries a doubt mask or an exclusion list: every cell of every output is compared.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_follow_reference as fref  # noqa: E402
import elevation_points_reference as pref  # noqa: E402
import elevation_reference as eref  # noqa: E402
import elevation_variance_reference as varref  # noqa: E402

F = np.float32
NSCAN, SCAN_H, SCAN_W = 117, 13, 9
CLAMP = F(1.0e9)
ORIGIN_CLAMP = 1 << 30
BAND_SCALE = F(2.0 ** 18)
OBS_DIM = 171
HEIGHT_BAR, VAR_BAR = 2e-5, 1e-4                   # the project's bars: 2e-5 (1 + |ref|) on heights, 1e-4 relative on variances
NAN = F(np.nan)
FLT_MAX = np.finfo(F).max
Q_ID, Q_HALF = (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def dn(x):
    return np.nextafter(F(x), F(-np.inf))


def step(x, direction):
    return up(x) if direction > 0 else dn(x)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.int32)


def cell(x, res):
    """the tick's rule"""
    with np.errstate(all="ignore"):
        c = np.floor(np.asarray(x, F) / F(res))
    return np.fmin(np.fmax(c, -CLAMP), CLAMP).astype(np.int64)


def cell_recip(x, res):
    """the visibility samples' rule: the reciprocal formed once, in fp32"""
    with np.errstate(all="ignore"):
        c = np.floor(np.asarray(x, F) * (F(1) / F(res)))
    return np.fmin(np.fmax(c, -CLAMP), CLAMP).astype(np.int64)


def first_float(k, res, rule=cell):
    """the first fp32 value of cell k under `rule`, found by stepping nextafter; first_float(k) one step down is the last float of cell k - 1"""
    x = F(float(k) * float(F(res)))
    while rule(x, res) < k:
        x = up(x)
    while rule(dn(x), res) >= k:
        x = dn(x)
    assert rule(x, res) == k and rule(dn(x), res) == k - 1
    return x


def key_of(z):
    """the order-preserving key as an integer: the unsigned order of the keys is the total order of the floats, -0 < +0"""
    b = bits(z).astype(np.int64) & 0xFFFFFFFF
    return np.where((b >> 31) != 0, b ^ 0xFFFFFFFF, b | 0x80000000)


def quat_kind(q):
    q = np.asarray(q, F)
    if q[0] != 0 and not q[1:].any():
        return "identity"
    if q[3] != 0 and not q[:3].any():
        return "halfturn"
    raise ValueError("the twin knows the identity and the half-turn about z (and their multiples) alone")


def settings(grid=24, res=0.04, alpha=1.0, self_half=(0.0, 0.0, 0.0), row0=38, variance=None, visibility=None, follow=False, camera=None):
    return dict(grid=int(grid), res=float(res), alpha=float(alpha), self_half=tuple(float(x) for x in self_half), sdx=0.1, sdy=0.1, row0=int(row0),
                variance=None if variance is None else dict(variance), visibility=None if visibility is None else dict(visibility), follow=bool(follow),
                camera=None if camera is None else dict(camera))


def new_state(S):
    G = S["grid"]
    return dict(map=np.full((G, G), NAN), origin=np.zeros(2, np.int64), var=np.full((G, G), NAN) if S["variance"] else None)


def _stale(origin, new_origin, G, clear):
    if clear or (np.abs(origin) > ORIGIN_CLAMP).any():
        return np.ones((G, G), bool)
    s = np.arange(G)
    ax = []
    for a in (0, 1):
        lo_new, lo_old = int(new_origin[a]) - G // 2, int(origin[a]) - G // 2
        ax.append((lo_new + (s - lo_new) % G) != (lo_old + (s - lo_old) % G))
    return ax[0][:, None] | ax[1][None, :]


def scan(hmap, vmap, origin, qpos, S):
    """step 5 at yaw 0 (the identity) or yaw pi (the half-turn: sin(fl32(pi)) is 9e-8, so the points are asserted to be far from every border)"""
    G, res = S["grid"], F(S["res"])
    b = np.asarray(qpos[:3], F)
    kind = quat_kind(qpos[3:7])
    r, c = np.divmod(np.arange(NSCAN), SCAN_W)
    ox, oy = (F(6) - r.astype(F)) * F(S["sdx"]), (F(4) - c.astype(F)) * F(S["sdy"])
    sgn = F(1) if kind == "identity" else F(-1)
    wx, wy = b[0] + sgn * ox, b[1] + sgn * oy
    assert wx.dtype == F
    if kind == "halfturn":
        assert eref.border_margin(np.stack([wx, wy], 1).astype(float), float(res)).min() > 1e-4, "half-turn: a scan point too near a border"
    cx, cy = cell(wx, res), cell(wy, res)
    lo = np.asarray(origin, np.int64) - G // 2
    inside = (cx >= lo[0]) & (cx < lo[0] + G) & (cy >= lo[1]) & (cy < lo[1] + G)
    z = np.where(inside, hmap[cx % G, cy % G], NAN).astype(F)
    known = inside & ~np.isnan(z)
    est = np.zeros(NSCAN, F)
    if known.any():
        zmin = z[known].min()
        zero = z[known][z[known] == 0]
        assert zmin != 0 or len(set(np.signbit(zero))) <= 1, "the minimum of -0 and +0 is not fixed by the contract: keep them out of one scan"
        if zmin < np.inf:
            est[known] = z[known] - zmin
    est_var = None
    if vmap is not None:
        est_var = np.where(known, vmap[cx % G, cy % G], F(S["variance"]["var_max"])).astype(F)
    return est, known, est_var, np.stack([cx, cy], 1)


def _assemble(obs, est, S):
    if obs is None:
        obs = np.zeros(OBS_DIM, F)
    out = np.array(obs, F)
    out[S["row0"]:S["row0"] + NSCAN] = est
    return out


def tick(state, qpos, points, S, clear=False, obs=None):
    """one pgtt_elevation_points() or, with S["variance"], one pgtt_elevation_var_points() call for one env, in fp32.
    -> dict(map, origin, est, known, obs[, var, est_var], exact, decisions)"""
    G, res, alpha = S["grid"], F(S["res"]), F(S["alpha"])
    var = S["variance"]
    hmap = np.array(state["map"], F)
    vmap = np.array(state["var"], F) if var else None
    b = np.asarray(qpos[:3], F)
    quat_kind(qpos[3:7])
    origin = np.array([cell(b[0], res), cell(b[1], res)], np.int64)
    stale = _stale(np.asarray(state["origin"], np.int64), origin, G, clear)
    hmap[stale] = NAN
    if var:
        vmap[stale] = NAN
    lo = origin - G // 2
    P = np.asarray(points, F).reshape(-1, 3)
    valid = np.isfinite(P).all(1)
    half = np.asarray(S["self_half"], F)
    inside = np.zeros(len(P), bool)
    if half.any():
        with np.errstate(all="ignore"):
            inside = valid & (np.abs(P - b[None]) <= half[None]).all(1)
    cx, cy = cell(P[:, 0], res), cell(P[:, 1], res)
    use = valid & ~inside & (cx >= lo[0]) & (cx < lo[0] + G) & (cy >= lo[1]) & (cy < lo[1] + G)
    slot = np.where(use, (cx % G) * G + (cy % G), -1)
    keys = key_of(P[:, 2])
    best = np.full(G * G, -1, np.int64)
    winner = np.full(G * G, -1, np.int64)
    for k in np.nonzero(use)[0]:
        if keys[k] > best[slot[k]]:
            best[slot[k]], winner[slot[k]] = keys[k], k
    touched = (winner >= 0).reshape(G, G)
    zmax = np.where(winner >= 0, P[np.maximum(winner, 0), 2], NAN).astype(F).reshape(G, G)
    exact = True
    n = np.zeros((G, G), np.int64)
    branch = np.zeros((G, G), np.int8)
    if not var:
        h, m = hmap[touched], zmax[touched]
        with np.errstate(all="ignore"):
            d = m - h
            t = alpha * d
            fused = h + t
        plain = np.isnan(h) | (alpha == F(1))
        ok = plain | (t.astype(float) == float(alpha) * d.astype(float))
        exact = bool(ok.all())
        hmap[touched] = np.where(plain, m, fused)
    else:
        band, process, var_max = F(var["band"]), F(var["process"]), F(var["var_max"])
        s0sq, gate2 = F(float(F(var["sigma0"])) ** 2), F(float(F(var["gate"])) ** 2)
        srsq = F(float(F(var["sigma_rel"])) ** 2)
        S_ = np.zeros((G, G), np.int64)
        for k in np.nonzero(use)[0]:
            i, j = divmod(int(slot[k]), G)
            dz = zmax[i, j] - P[k, 2]
            if dz <= band:
                n[i, j] += 1
                S_[i, j] += int(np.rint(dz * BAND_SCALE))
        known = ~np.isnan(hmap)
        vmap[known] = np.fmin(vmap[known] + process, var_max)
        for i, j in zip(*np.nonzero(touched)):
            nn = max(int(n[i, j]), 1)
            m = zmax[i, j]
            if S_[i, j]:
                m = F(m - F(F(S_[i, j]) / F(nn)) * F(2.0 ** -18))
            if srsq == 0:
                r = F(s0sq / F(min(nn, int(var["max_count"]))))
            else:
                wc = (lo + (np.array([i, j]) - lo) % G).astype(F)
                dx, dy, dzz = (wc[0] + F(0.5)) * res - b[0], (wc[1] + F(0.5)) * res - b[1], m - b[2]
                r = F(F(s0sq + srsq * F(dx * dx + dy * dy + dzz * dzz)) / F(min(nn, int(var["max_count"]))))
                exact = False
            h, v = hmap[i, j], vmap[i, j]
            if np.isnan(h):
                hmap[i, j], vmap[i, j], branch[i, j] = m, min(r, var_max), 1
                continue
            d, den = F(m - h), F(v + r)
            if F(d * d) <= F(gate2 * den):
                k_ = F(v / den) if den > 0 else F(0)
                kd = F(k_ * d)
                exact &= float(kd) == float(k_) * float(d)
                hmap[i, j], vmap[i, j], branch[i, j] = F(h + kd), (F(F(v * r) / den) if den > 0 else F(0)), 2
            elif m > h:
                hmap[i, j], vmap[i, j], branch[i, j] = m, min(r, var_max), 3
            else:
                branch[i, j] = 4
    est, known, est_var, sc = scan(hmap, vmap, origin, qpos, S)
    out = dict(map=hmap, origin=origin, est=est, known=known.astype(np.uint8), obs=_assemble(obs, est, S), exact=exact,
               decisions=dict(origin=origin.copy(), slot=slot.copy(), winner=winner.copy(), n=n, branch=branch, nanmap=np.isnan(hmap), known=known.copy(), scan=sc))
    if var:
        out.update(var=vmap, est_var=est_var)
    return out


def hold(state, qpos, S, clear=False, obs=None):
    """one hold call of pgtt_elevation_follow() for one env"""
    G, res = S["grid"], F(S["res"])
    hmap, origin = np.array(state["map"], F), np.array(state["origin"], np.int64)
    if clear:
        hmap[:] = NAN
        origin = np.array([cell(F(qpos[0]), res), cell(F(qpos[1]), res)], np.int64)
    est, known, _, sc = scan(hmap, None, np.clip(origin, -ORIGIN_CLAMP, ORIGIN_CLAMP), qpos, S)
    return dict(map=hmap, origin=origin, est=est, known=known.astype(np.uint8), obs=_assemble(obs, est, S), exact=True,
                decisions=dict(origin=origin.copy(), nanmap=np.isnan(hmap), known=known.copy(), scan=sc))


def clean(state, qpos, points, S, skip=False):
    """one pgtt_elevation_visibility() call for one env from the points, at the identity pose, rays along one axis.
    -> dict(map, origin[, var], cleared, bound, exact, decisions, samples = [(x, y)] of the samples made)"""
    G, res = S["grid"], F(S["res"])
    vis = S["visibility"]
    hmap = np.array(state["map"], F)
    vmap = np.array(state["var"], F) if S["variance"] else None
    origin = np.array(state["origin"], np.int64)
    bound = np.full((G, G), NAN)
    out = dict(map=hmap, origin=origin, cleared=np.int32(0), bound=bound, exact=True, samples=[])
    if vmap is not None:
        out["var"] = vmap
    if skip:
        out["decisions"] = dict(cleared=0, nanmap=np.isnan(hmap), nobound=np.isnan(bound))
        return out
    assert quat_kind(qpos[3:7]) == "identity"
    b = np.asarray(qpos[:3], F)
    s = b + np.asarray(vis.get("sensor_pos", (0, 0, 0)), F)
    lo = np.clip(origin, -ORIGIN_CLAMP, ORIGIN_CLAMP) - G // 2
    half = np.asarray(S["self_half"], F)
    eg, margin, sig = F(vis["end_guard"]), F(vis["margin"]), F(vis.get("sigmas", 0.0))
    P = np.asarray(points, F).reshape(-1, 3)
    bkey = np.full((G, G), 1 << 40, np.int64)
    for k in range(0, len(P), int(vis["stride"])):
        p = P[k]
        if not np.isfinite(p).all():
            continue
        if half.any() and (np.abs(p - b) <= half).all():
            continue
        dx, dy = F(p[0] - s[0]), F(p[1] - s[1])
        assert dx == 0 or dy == 0, "the twin casts rays along one axis: hypot is then |d| exactly"
        Lh = F(max(abs(dx), abs(dy)))
        lim = F(Lh - eg)
        if not (F(0.5) * res <= lim):
            continue
        inv = F(1) / Lh
        ux, uy, uz = F(dx * inv), F(dy * inv), F(F(p[2] - s[2]) * inv)
        for kk in range(2 * G):
            rk = F(F(kk) + F(0.5)) * res
            if not (rk <= lim):
                break
            x, y, z = (F(float(rk) * float(u) + float(o)) for u, o in ((ux, s[0]), (uy, s[1]), (uz, s[2])))
            out["samples"].append((x, y))
            cx, cy = int(cell_recip(x, res)), int(cell_recip(y, res))
            if not (lo[0] <= cx < lo[0] + G and lo[1] <= cy < lo[1] + G) or np.isnan(z):
                continue
            kz = int(key_of(np.array([z]))[0])
            if kz < bkey[cx % G, cy % G]:
                bkey[cx % G, cy % G], bound[cx % G, cy % G] = kz, z
    cleared = np.zeros((G, G), bool)
    for i, j in zip(*np.nonzero(~np.isnan(bound) & ~np.isnan(hmap))):
        t = hmap[i, j]
        if vmap is not None:
            sv = F(sig * F(np.sqrt(vmap[i, j])))
            out["exact"] &= float(sv) == float(sig) * float(F(np.sqrt(vmap[i, j])))
            t = F(t - sv)
        cleared[i, j] = t > F(bound[i, j] + margin)
    hmap[cleared] = NAN
    if vmap is not None:
        vmap[cleared] = NAN
    out["cleared"] = np.int32(cleared.sum())
    out["decisions"] = dict(cleared=int(cleared.sum()), nanmap=np.isnan(hmap), nobound=np.isnan(bound), bound=bits(bound))
    return out


# ---------------------------------------------------------------- running a case
FIELDS = {"tick": ("map", "origin", "est", "known", "obs", "var", "est_var"), "hold": ("map", "origin", "est", "known", "obs"),
          "clean": ("map", "origin", "var", "cleared", "bound")}


def ref_cfg(S):
    c = dict(res=S["res"], alpha=S["alpha"], self_half=S["self_half"], scan_dist_x=S["sdx"], scan_dist_y=S["sdy"], scan_row0=S["row0"])
    if S["camera"]:
        c.update({k: S["camera"][k] for k in ("fovy", "near", "far", "mount_pos", "mount_quat")})
    return c


def run_twin(case):
    """the twin over the case's ticks -> per tick its output dict"""
    S = case["S"]
    st, outs = new_state(S), []
    for t in case["ticks"]:
        if t.get("origin_in") is not None:
            st["origin"] = np.array(t["origin_in"], np.int64)
        q = np.array(t["qpos"], F)
        if t["op"] == "tick":
            o = tick(st, q, t["points"], S, clear=t.get("clear", False), obs=t.get("obs"))
            if S["visibility"] and t.get("clear", False):                  # the clean-up in front of a clearing tick skips the env
                o.update(cleared=np.int32(0), bound=np.full((S["grid"],) * 2, NAN))
        elif t["op"] == "hold":
            o = hold(st, q, S, clear=t.get("clear", False), obs=t.get("obs"))
        else:
            o = clean(st, q, t["points"], S, skip=t.get("clear", False))
        st = dict(map=o["map"], origin=o["origin"], var=o.get("var", st.get("var")))
        outs.append(o)
    return outs


def run_reference(case):
    """the fp64 references of tests/ over the case's ticks (tick and hold; points or image) -> per tick dict(map, origin, est, known, obs[, var,
    est_var], branch)"""
    S = case["S"]
    G, cfg, var = S["grid"], ref_cfg(S), S["variance"]
    hmap, vmap, origin = np.full((G, G), np.nan), np.full((G, G), np.nan), np.zeros(2, np.int64)
    outs = []
    for t in case["ticks"]:
        if t.get("origin_in") is not None:
            origin = np.array(t["origin_in"], np.int64)
            if (np.abs(origin) > ORIGIN_CLAMP).any():                         # "an old origin outside the clamp ... everything is stale"
                hmap[:], vmap[:] = np.nan, np.nan
        q = np.array(t["qpos"], F).astype(float)
        obs = None if t.get("obs") is None else np.asarray(t["obs"], F).astype(float)
        image = t.get("image") is not None
        src = None if t["op"] == "hold" else np.asarray(t["image"] if image else t["points"], F)
        clear = t.get("clear", False)
        with np.errstate(all="ignore"):
            if t["op"] == "hold":
                o = fref.hold((hmap, origin), q, cfg, clear=clear, obs=obs)
            elif var:
                o = varref.tick((hmap, vmap, origin), q, src, cfg, var, clear=clear, obs=obs, points=not image)
            else:
                o = (eref.tick if image else pref.tick)((hmap, origin), q, src, cfg, clear=clear, obs=obs)
        hmap, origin = np.array(o["map"], float), np.array(o["origin"], np.int64)
        if var and "var" in o:
            vmap = o["var"]
        outs.append(o)
    return outs


def expected(case):
    """per tick {field: (mark, array)}: from the twin (mode "bits": float fields bit for bit unless the case overrides a field's mark) or from the fp64
    references (mode "ref": float fields at the bars, integers exactly)"""
    over = case.get("marks", {})
    res = []
    if case["mode"] == "bits":
        for t, o in zip(case["ticks"], run_twin(case)):
            assert o["exact"] or all(over.get(f) == "bar" for f in ("map", "var", "est", "obs", "est_var") if f in o), (case["name"], "inexact")
            res.append({f: (over.get(f, "bits"), o[f]) for f in FIELDS[t["op"]] + ("cleared", "bound") if o.get(f) is not None})
    else:
        for t, o in zip(case["ticks"], run_reference(case)):
            e = dict(map=("bar", o["map"]), origin=("bits", o["origin"]), est=("bar", o["est"]), known=("bits", np.asarray(o["known"], np.uint8)))
            if "obs_out" in o:
                e["obs"] = ("bar", o["obs_out"])
            if "var" in o and t["op"] == "tick" and case["S"]["variance"]:
                e["var"], e["est_var"] = ("bar", o["var"]), ("bar", o["est_var"])
            res.append(e)
    return res


def with_edge_moved(case, edge, by=None):
    """a copy of the case with one edge input replaced: by its neighbouring float across the edge (by = None), or moved by `by` metres (signed along
    the edge's direction)"""
    ti, what, idx, axis, direction = edge
    c = dict(case, ticks=[dict(t) for t in case["ticks"]])
    t = c["ticks"][ti]
    if what == "points":
        arr = np.array(t["points"], F)
        arr[idx, axis] = step(arr[idx, axis], direction) if by is None else F(float(arr[idx, axis]) + direction * by)
        t["points"] = arr
    else:
        arr = np.array(t["qpos"], F)
        arr[axis] = step(arr[axis], direction) if by is None else F(float(arr[axis]) + direction * by)
        t["qpos"] = arr
    return c


def decisions(case):
    return [o["decisions"] for o in run_twin(case)]


def same_decisions(a, b):
    return all(set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


# ---------------------------------------------------------------- the families
def _case(name, family, S, ticks, edges=(), mode="bits", marks=None, **more):
    # the points buffer of a handle has one size: the shorter point lists of a case end in rows of NaN ("a ray without a return")
    P = max([len(t["points"]) for t in ticks if t.get("points") is not None], default=0)
    for t in ticks:
        if t.get("points") is not None and len(t["points"]) < P:
            t["points"] = np.concatenate([np.asarray(t["points"], F), np.full((P - len(t["points"]), 3), NAN)])
    return dict(name=name, family=family, S=S, ticks=ticks, edges=list(edges), mode=mode, marks=dict(marks or {}), **more)


def _qpos(b, q=Q_ID):
    return np.array(list(b) + list(q), F)


def _z(i):
    """a height unique to point i"""
    return F(1.0 + i * 2.0 ** -10)


def _obs(seed):
    return np.random.default_rng(seed).normal(size=OBS_DIM).astype(F)


def _fill_points(origin, G, res, height=lambda a, b: F(0.25 + (a * 97 + b) * 2.0 ** -12), rule=cell):
    """one point at the centre of every window cell (the cell is checked), each with its own height"""
    lo = np.asarray(origin, np.int64) - G // 2
    pts = np.zeros((G * G, 3), F)
    for a in range(G):
        for b_ in range(G):
            x, y = F((lo[0] + a + 0.5) * float(F(res))), F((lo[1] + b_ + 0.5) * float(F(res)))
            assert rule(x, res) == lo[0] + a and rule(y, res) == lo[1] + b_
            pts[a * G + b_] = (x, y, height(a, b_))
    return pts


def family_a():
    """Cell borders and the origin: per res, window (astride 0, wholly negative), axis and base edge (the base on the first float of its cell or on
    the last float of the previous one), the first float of cell k and the last float of cell k - 1 at every border of the window.  Firsts and
    lasts of one axis lie in two different rows of the other, so every cell holds one point and a point in the wrong cell shows."""
    cases = []
    G = 24
    for res in (0.04, 0.12, 2.0 ** -5):
        for wname, k0 in (("astride", 3), ("negative", -40)):
            for axis in (0, 1):
                for bname, bdir in (("first", -1), ("last", +1)):
                    edge = first_float(k0, res) if bname == "first" else dn(first_float(k0, res))
                    other = F((k0 + 0.5) * float(F(res)))
                    b = [other, other, F(0.5)]
                    b[axis] = edge
                    origin = np.array([cell(b[0], res), cell(b[1], res)])
                    assert origin[axis] == (k0 if bname == "first" else k0 - 1) and origin[1 - axis] == k0
                    lo = origin - G // 2
                    rows = (F((lo[1 - axis] + 2.5) * float(F(res))), F((lo[1 - axis] + 5.5) * float(F(res))))
                    pts, edges = [], [(0, "qpos", 0, axis, bdir)]
                    for k in range(lo[axis], lo[axis] + G + 1):
                        for which, (x, d) in enumerate(((first_float(k, res), -1), (dn(first_float(k, res)), +1))):
                            p = [rows[which], rows[which], _z(len(pts))]
                            p[axis] = x
                            edges.append((0, "points", len(pts), axis, d))
                            pts.append(p)
                    cases.append(_case(f"A-res{res:g}-{wname}-axis{axis}-base{bname}", "A", settings(G, res), [dict(op="tick", qpos=_qpos(b), points=np.array(pts, F),
                                                                                                      clear=True, obs=_obs(len(cases)))], edges))
    return cases


def family_b():
    """Validity and the key"""
    G, res = 24, 0.12
    S = settings(G, res)
    b = (0.05, 0.05, 0.5)
    ctr = lambda k: F((k + 0.5) * float(F(res)))
    cases = []

    def add(name, pts):
        cases.append(_case("B-" + name, "B", S, [dict(op="tick", qpos=_qpos(b), points=np.array(pts, F), clear=True, obs=_obs(len(cases)))]))

    bad = []
    for i, v in enumerate((np.nan, np.inf, -np.inf)):
        for ax in range(3):
            p = [ctr(7 + i), ctr(-3 + ax), _z(len(bad))]
            p[ax] = v
            bad.append(p)
    add("nonfinite", bad + [[ctr(0), ctr(0), 0.75]])
    add("clamp", [[s * v, ctr(1), _z(i)] for i, (s, v) in enumerate(((1, 3e38), (-1, 3e38), (1, 1e12), (-1, 1e12)))] +
        [[ctr(1), s * v, _z(4 + i)] for i, (s, v) in enumerate(((1, 3e38), (-1, 3e38), (1, 1e12), (-1, 1e12)))] + [[ctr(0), ctr(0), 0.75]])
    # the zeros and the extremes sit at x = 9 cells, beyond the scan's footprint: the minimum of -0 and +0 is not fixed by the contract
    add("zeros", [[ctr(9), ctr(0), -0.0], [ctr(9), ctr(0), 0.0], [ctr(9), ctr(1), 0.0], [ctr(9), ctr(1), -0.0], [ctr(9), ctr(2), -0.0],
                  [ctr(9), ctr(3), 1e-41], [ctr(9), ctr(4), -1e-41], [ctr(9), ctr(4), -2e-41], [ctr(0), ctr(0), 0.75]])
    add("extremes", [[ctr(9), ctr(0), -FLT_MAX], [ctr(9), ctr(1), -FLT_MAX], [ctr(9), ctr(1), FLT_MAX], [ctr(9), ctr(2), -1.5], [ctr(9), ctr(2), -1.25],
                     [ctr(9), ctr(2), -1.75], [ctr(0), ctr(0), -0.75], [ctr(1), ctr(0), -FLT_MAX]])
    for P in (1, 255, 256, 257):
        add(f"P{P}", [[ctr(0), ctr(1), F(0.5 - (P - i) * 2.0 ** -12)] for i in range(P - 1)] + [[ctr(0), ctr(1), 0.5]])
    add("one-cell-300", [[ctr(-2), ctr(2), F(0.5 - abs(i - 170) * 2.0 ** -12)] for i in range(300)])
    return cases


def _outside(bc, h, sign):
    """the first float p beyond bc + sign * h with |fl32(p - bc)| > h"""
    p = F(F(bc) + F(sign * h))
    assert abs(F(p - F(bc))) == F(h)
    while abs(F(p - F(bc))) <= F(h):
        p = step(p, sign)
    return p


def family_c():
    """The self box, at the identity and at the half-turn: |l| = half is skipped, the next float outside is kept"""
    G, res = 48, 2.0 ** -5
    b = (0.515625, -0.265625, 0.75)
    cases = []
    for qname, q in (("identity", Q_ID), ("halfturn", Q_HALF)):
        def add(name, half, pts, edges):
            cases.append(_case(f"C-{name}-{qname}", "C", settings(G, res, self_half=half),
                               [dict(op="tick", qpos=_qpos(b, q), points=np.array(pts, F), clear=True, obs=_obs(len(cases)))], edges))
        half = (0.5, 0.25, 0.5)
        pts, edges = [], []
        off = ((0.0, 0.0625, 0.03125), (0.0625, 0.0, -0.03125), (-0.0625, 0.09375, 0.0))          # where the other two axes sit, inside the box
        for ax in range(3):
            for sign in (1, -1):
                for which in (0, 1):                                              # 0: exactly on the face (skipped), 1: the next float outside (kept)
                    p = [F(b[i] + off[ax][i] * (1 if which else -1) + 0.125 * sign * (i != ax)) for i in range(3)]
                    p[ax] = _outside(b[ax], half[ax], sign)
                    if which == 0:
                        p[ax] = step(p[ax], -sign)                                # the last float whose fl32(p - b) is the face: |l| == half exactly
                        assert abs(F(p[ax] - F(b[ax]))) == F(half[ax])
                    edges.append((0, "points", len(pts), ax, sign if which == 0 else -sign))
                    pts.append(p)
        add("faces", half, pts, edges)
        hc = (0.25, 0.25, 0.25)
        pts = [[dn(_outside(b[i], 0.25, 1)) for i in range(3)]]
        edges = [(0, "points", 0, ax, 1) for ax in range(3)]
        for ax in range(3):
            p = [F(b[i] - 0.25) for i in range(3)]
            p[ax] = _outside(b[ax], 0.25, -1)
            p[(ax + 1) % 3] = F(b[(ax + 1) % 3] + 0.0625 * (ax + 1))
            edges.append((0, "points", len(pts), ax, 1))
            pts.append(p)
        add("corner", hc, pts, edges)
        add("two-in-one-out", half, [[b[0] + 0.625, b[1] + 0.125, b[2] + 0.25], [b[0] - 0.25, b[1] - 0.375, b[2] - 0.125], [b[0] + 0.125, b[1] - 0.0625, b[2] + 0.625],
                                     [b[0] + 0.25, b[1] + 0.125, b[2] + 0.25]], [])
        add("off", (0.0, 0.0, 0.0), [list(b), [b[0] + 0.0625, b[1], b[2] + 0.125]], [])
        add("flat-y", (0.5, 0.0, 0.5), [[b[0] + 0.125, b[1], b[2] + 0.25], [b[0] - 0.125, up(b[1]), b[2] + 0.125], [b[0] + 0.25, dn(b[1]), b[2] - 0.125],
                                        [b[0] + 0.625, b[1], b[2]]], [(0, "points", 0, 1, 1), (0, "points", 0, 1, -1), (0, "points", 1, 1, -1), (0, "points", 2, 1, 1)])
    return cases


D_MOVES = lambda G: (1, -1, G - 1, -(G - 1), G, -G, G + 1, -(G + 1))


def family_d():
    """Recentre: one tick fills every window cell, then all-NaN ticks move the base by whole cells"""
    res = 2.0 ** -5
    ctr = lambda k: F((k + 0.5) * res)
    cases = []
    for G in (8, 9, 24):
        S = settings(G, res)
        starts = [((2, -3), "")]
        if G == 24:
            starts += [((2 ** 20, -2 ** 20 + 5), "-far"), ((-1, 0), "-zero")]
        for o0, tag in starts:
            fill = _fill_points(o0, G, res)
            for mv in D_MOVES(G):
                for dname, d in (("x", (1, 0)), ("y", (0, 1)), ("xy", (1, -1))):
                    if tag and (dname != "xy" or abs(mv) not in (1, G - 1)):
                        continue
                    o1 = (o0[0] + mv * d[0], o0[1] + mv * d[1])
                    ticks = [dict(op="tick", qpos=_qpos((ctr(o0[0]), ctr(o0[1]), 0.5)), points=fill, clear=True, obs=_obs(1)),
                             dict(op="tick", qpos=_qpos((ctr(o1[0]), ctr(o1[1]), 0.5)), points=np.full((G * G, 3), NAN), obs=_obs(2)),
                             dict(op="tick", qpos=_qpos((ctr(o0[0]), ctr(o0[1]), 0.5)), points=np.full((G * G, 3), NAN), obs=_obs(3))]
                    cases.append(_case(f"D-G{G}{tag}-{dname}{mv:+d}", "D", S, ticks, move=(mv, dname)))
        if G == 24:
            for name, o in (("int32min", (-2 ** 31, 2)), ("int32max", (2, 2 ** 31 - 1)), ("2^30+1", (2 ** 30 + 1, -3)), ("-2^30-1", (2, -2 ** 30 - 1))):
                ticks = [dict(op="tick", qpos=_qpos((ctr(2), ctr(-3), 0.5)), points=_fill_points((2, -3), G, res), clear=True),
                         dict(op="tick", qpos=_qpos((ctr(2), ctr(-3), 0.5)), points=np.full((G * G, 3), NAN), origin_in=o)]
                cases.append(_case(f"D-G{G}-origin-{name}", "D", S, ticks))
    G, o = 96, (-5, 7)
    ticks = [dict(op="tick", qpos=_qpos((ctr(o[0]), ctr(o[1]), 0.5)), points=_fill_points(o, G, res), clear=True)]
    for mx, my in ((1, 0), (0, -(G - 1)), (G + 1, -1), (-G, 0)):
        o = (o[0] + mx, o[1] + my)
        ticks.append(dict(op="tick", qpos=_qpos((ctr(o[0]), ctr(o[1]), 0.5)),
                          points=_fill_points(o, G, res) if (mx, my) == (G + 1, -1) else np.full((G * G, 3), NAN)))
    cases.append(_case("D-G96-sequence", "D", settings(G, res), ticks))
    return cases


def family_e():
    """Fuse"""
    G, res = 24, 2.0 ** -5
    ctr = lambda k: F((k + 0.5) * res)
    b = (ctr(0), ctr(0), 0.5)
    first = [[ctr(i - 4), ctr(2), F(0.5 + i * 0.125)] for i in range(8)]
    second = [[ctr(i - 4), ctr(2), F(1.75 - i * 0.375)] for i in range(6)] + [[ctr(i - 4), ctr(-2), F(0.3125 * i - 1)] for i in range(8)]
    ticks = lambda p0, p1: [dict(op="tick", qpos=_qpos(b), points=np.array(p0, F), clear=True, obs=_obs(5)), dict(op="tick", qpos=_qpos(b), points=np.array(p1, F), obs=_obs(6))]
    odd0 = [[ctr(i - 4), ctr(2), F(0.1 + i * 0.0123)] for i in range(8)]
    odd1 = [[ctr(i - 4), ctr(2), F(0.77 - i * 0.0371)] for i in range(6)] + [[ctr(i - 4), ctr(-2), F(0.031 * i - 0.1)] for i in range(8)]
    return [_case("E-alpha0.5-dyadic", "E", settings(G, res, alpha=0.5), ticks(first, second)),
            _case("E-alpha0.25-dyadic", "E", settings(G, res, alpha=0.25), ticks(first, second)),
            _case("E-alpha1", "E", settings(G, res, alpha=1.0), ticks(odd0, odd1)),
            _case("E-alpha0.3-bar", "E", settings(G, res, alpha=0.3), ticks(odd0, odd1), mode="ref")]


def _base_for_scan(res, row, k, last, sd=0.1):
    """a base coordinate such that the scan offset of `row`, fl32(b + fl32((6 - row) * sd)) under the tick's rule, is the first float of cell k (or
    the last float of cell k - 1)"""
    o = F(F(6 - row) * F(sd))
    target = dn(first_float(k, res)) if last else first_float(k, res)
    bb = F(float(target) - float(o))
    for _ in range(64):
        w = F(bb + o)
        if w == target:
            return bb
        bb = up(bb) if w < target else dn(bb)
    raise AssertionError("no base puts the scan point on the edge")


def family_f():
    """The scan at yaw 0 on a full window, through a fresh call and a hold call of pgtt_elevation_follow"""
    G, res = 24, 0.04
    cases = []
    height = lambda a, b: F(-0.5 + ((a * 7 + b * 13) % 101) * 2.0 ** -7)
    for row0 in (38, 30):
        S = settings(G, res, row0=row0, follow=True)
        for name, row, col, ky, last in (("first-r2-c3", 2, 3, -14, False), ("last-r2-c3", 2, 3, -14, True), ("first-r11-c0", 11, 0, -17, False), ("last-r7-c8", 7, 8, 28, True)):
            if row0 == 30 and name != "first-r2-c3":
                continue
            bx = _base_for_scan(res, row, 40 + row, last)
            by = _base_for_scan(res, col + 2, ky, not last)              # column c has the offset (4 - c) sd = (6 - (c + 2)) sd
            edges = [(t, "qpos", 0, 0, 1 if last else -1) for t in (0, 1)] + [(t, "qpos", 0, 1, -1 if last else 1) for t in (0, 1)]
            o = (int(cell(bx, res)), int(cell(by, res)))
            fill = _fill_points(o, G, res, height)
            mk = lambda q: [dict(op="tick", qpos=_qpos((bx, by, 0.5), q), points=fill, clear=True, obs=_obs(7)),
                            dict(op="hold", qpos=_qpos((bx, by, 0.5), q), obs=_obs(8))]
            cases.append(_case(f"F-row0-{row0}-{name}", "F", S, mk(Q_ID), edges))
            if name == "first-r2-c3":
                cases.append(_case(f"F-row0-{row0}-{name}-negated", "F", S, mk((-1.0, 0.0, 0.0, 0.0)), edges))
                cases.append(_case(f"F-row0-{row0}-{name}-doubled", "F", S, mk((2.0, 0.0, 0.0, 0.0)), edges))
                cases.append(_case(f"F-row0-{row0}-{name}-tripled", "F", S, mk((3.0, 0.0, 0.0, 0.0)), edges, marks=dict(map="bar", est="bar", obs="bar")))
        b = (F(1.63), F(-0.71), 0.5)
        o = (int(cell(b[0], res)), int(cell(b[1], res)))
        if row0 == 38:
            cases.append(_case("F-nothing-known", "F", S, [dict(op="tick", qpos=_qpos(b), points=np.full((G * G, 3), NAN), clear=True, obs=_obs(9)),
                                                          dict(op="hold", qpos=_qpos(b), obs=_obs(10))]))
            one = np.full((G * G, 3), NAN)
            one[0] = (b[0], b[1], -0.25)
            cases.append(_case("F-one-known", "F", S, [dict(op="tick", qpos=_qpos(b), points=one, clear=True, obs=_obs(11)), dict(op="hold", qpos=_qpos(b), obs=_obs(12)),
                                                       dict(op="hold", qpos=_qpos((b[0] + F(0.3), b[1], 0.5)), obs=_obs(13)),
                                                       dict(op="hold", qpos=_qpos(b), clear=True, obs=_obs(14))]))
    return cases


G_CAMERA = dict(fovy=60.0, near=0.25, far=0.8, mount_pos=(0.3, 0.0, 0.1), mount_quat=(0.9238795325112867, 0.0, 0.3826834323650898, 0.0))   # 45 degrees down
G_BASE = (0.0907, 0.0523, 0.697)                                                 # found by search: every lit pixel of every shape is 1.9 mm or more from a cell border
G_SHAPES = ((5, 3), (6, 2), (10, 6), (1, 1))
G_QUAT = (0.9961947, 0.0, 0.0, 0.0871557)                                        # 10 degrees of yaw


def family_g():
    """The image source: the depth's validity limits and one-hot images at widths whose float4 runs wrap a row, on the dword path and at 1 x 1"""
    G, res = 24, 0.12
    cases = []
    near, far = F(G_CAMERA["near"]), F(G_CAMERA["far"])
    for variance in (None, dict(varref.DEFAULTS)):
        tag = "var" if variance else "plain"
        for W, H in G_SHAPES:
            S = settings(G, res, variance=variance, camera=dict(G_CAMERA, width=W, height=H))
            for pix in range(W * H):
                img = np.full((H, W), far, F)
                img.reshape(-1)[pix] = F(0.5 + 0.01 * (pix % 7))
                cases.append(_case(f"G-{tag}-{W}x{H}-pixel{pix}", "G", S, [dict(op="tick", qpos=_qpos(G_BASE, G_QUAT), image=img, clear=True, obs=_obs(pix))], mode="ref"))
        S = settings(G, res, variance=variance, camera=dict(G_CAMERA, width=5, height=3))
        for i, d in enumerate((near, up(near), dn(far), far, np.nan, np.inf, -np.inf, -1.0, 0.0)):
            img = np.full((3, 5), np.nan, F)
            img[1, 3] = d
            cases.append(_case(f"G-{tag}-depth{i}", "G", S, [dict(op="tick", qpos=_qpos(G_BASE, G_QUAT), image=img, clear=True, obs=_obs(i))], mode="ref", lit=i in (1, 2)))
    return cases


H_BASE = dict(sigma0=0.25, sigma_rel=0.0, process=2.0 ** -6, gate=2.0, band=0.03, max_count=4, var_max=3.0 / 64)


H_SIGMA0_25128 = 0.4419417381286621                                           # an fp32 value whose square rounds to 25/128 in fp32


def _below(zmax, band, inside):
    """the lowest z with fl32(zmax - z) <= band (inside) or the float below it (excluded)"""
    z = F(float(zmax) - float(F(band)))
    while F(F(zmax) - z) <= F(band):
        z = dn(z)
    while F(F(zmax) - z) > F(band):
        z = up(z)
    assert F(F(zmax) - z) <= F(band) < F(F(zmax) - dn(z))
    return z if inside else dn(z)


def family_h():
    """The variance tick"""
    G, res = 24, 2.0 ** -5
    ctr = lambda k: F((k + 0.5) * res)
    b = (ctr(0), ctr(0), 0.5)
    nan_pts = lambda n: np.full((n, 3), NAN)
    cases = []

    def add(name, var, ticks, edges=(), **kw):
        cases.append(_case("H-" + name, "H", settings(G, res, variance=var), [dict(op="tick", qpos=_qpos(t.get("b", b)), points=np.array(t["p"], F), clear=i == 0, obs=_obs(i))
                                                                                for i, t in enumerate(ticks)], edges, **kw))
    at = lambda i, j, zs: [[ctr(i), ctr(j), z] for z in zs]
    v1 = dict(H_BASE)
    # the band's edge: the lowest z inside contributes (n = 2, v = r / 2), the float below does not (n = 1: v = min(r, var_max))
    pts = at(1, 1, [1.0, _below(1.0, 0.03, True)]) + at(3, 1, [1.0, _below(1.0, 0.03, False)]) + at(5, 1, [-2.0, _below(-2.0, 0.03, True)]) + \
        at(7, 1, [-2.0, _below(-2.0, 0.03, False)])
    add("band-edge", v1, [dict(p=pts)], [(0, "points", 1, 2, -1), (0, "points", 3, 2, 1), (0, "points", 5, 2, -1), (0, "points", 7, 2, 1)])
    # rint ties: dz = (j + 0.5) 2^-18 with n = 2 rounds half to even: q = 0, 2, 2, 4
    add("rint-ties", v1, [dict(p=sum((at(2 * j - 4, -2, [1.0, F(1.0 - (j + 0.5) * 2.0 ** -18)]) for j in range(4)), []))])
    # the cap: n = max_count - 1, max_count, max_count + 1
    add("max-count", v1, [dict(p=at(-3, 3, [0.5] * 3) + at(-1, 3, [0.5] * 4) + at(1, 3, [0.5] * 5) + at(3, 3, [0.5] * 9))])
    # var_max: a first touch with r = 1/16 > var_max = 3/64; a predict step that lands on var_max, and the next that crosses it
    add("var-max", v1, [dict(p=at(0, 5, [0.5]) + at(2, 5, [0.75, 0.75])), dict(p=nan_pts(3)), dict(p=nan_pts(3)), dict(p=nan_pts(3))])
    # the gate.  First touch with n = 4: v = 1/64; predict: 1/32; a measurement with n = 2: r = 1/32, v + r = 1/16, gate^2 (v + r) = 1/4: d = 1/2
    # max_count = 1 makes r = sigma0^2 whatever n is, and every cell takes ONE point, so the neighbouring float of its z is the neighbouring m.
    #   process > 0: sigma0 = 1/4, r = 1/16; first touch v = 1/16, predict 1/16 + 1/8 = 3/16, v + r = 1/4, gate^2 (v + r) = 1: d = 1, k = 3/4
    #   process = 0: sigma0^2 = 25/128 (H_SIGMA0_25128), v = r, v + r = 25/64, gate = 1: d = 5/8, k = 1/2
    assert F(float(F(H_SIGMA0_25128)) ** 2) == F(25.0 / 128)
    for name, var, d in (("process", dict(H_BASE, var_max=1.0, max_count=1, process=0.125), 1.0),
                         ("process0", dict(H_BASE, var_max=1.0, max_count=1, process=0.0, gate=1.0, sigma0=H_SIGMA0_25128), 0.625)):
        h = 1.5
        over, under = F(h + d), F(h - d)
        while F(over - F(h)) <= F(d):
            over = up(over)
        while F(under - F(h)) >= F(-d):
            under = dn(under)
        first = sum((at(2 * i - 5, 1, [h]) for i in range(6)), [])
        assert F(dn(over) - F(h)) == F(d) and F(up(under) - F(h)) == F(-d)         # the last m on either side whose fl32(m - h) is d: equality
        second = at(-5, 1, [dn(over)]) + at(-3, 1, [up(under)]) + at(-1, 1, [over]) + at(1, 1, [under]) + at(3, 1, [h]) + at(9, 1, [0.125])
        add(f"gate-{name}", var, [dict(p=first), dict(p=second), dict(p=nan_pts(2))],
            [(1, "points", 0, 2, 1), (1, "points", 1, 2, -1), (1, "points", 2, 2, -1), (1, "points", 3, 2, 1)])
    # a recentre clears var with map; est_var at an unknown point is var_max
    fill = _fill_points((0, 0), G, res)
    add("recentre", dict(H_BASE, var_max=1.0), [dict(p=fill), dict(p=nan_pts(G * G), b=(ctr(3), ctr(-G + 1), 0.5)), dict(p=nan_pts(G * G), b=(ctr(3 + G), ctr(-G + 1), 0.5))])
    add("band0", dict(H_BASE, band=0.0), [dict(p=at(1, 1, [1.0, 1.0]) + at(3, 1, [1.0, dn(1.0)]) + at(5, 1, [-0.0, 0.0]))], [(0, "points", 1, 2, -1), (0, "points", 3, 2, 1)])
    rng = np.random.default_rng(3)
    soft = [np.concatenate([rng.uniform(-0.3, 0.3, (60, 2)) + 0.0117, rng.uniform(0.0, 0.1, (60, 1))], 1) for _ in range(3)]
    add("sigma-rel-bar", dict(varref.DEFAULTS), [dict(p=p) for p in soft], mode="ref")
    return cases


def _guard_for(L, rk):
    """an end guard with fl32(L - guard) == rk exactly"""
    g = F(float(L) - float(rk))
    for _ in range(64):
        lim = F(F(L) - g)
        if lim == rk:
            return g
        g = dn(g) if lim < rk else up(g)
    raise AssertionError("no guard")


def family_j():
    """Visibility clean-up from the points at the identity pose, rays along an axis whose horizontal length is a power of two"""
    G = 24
    cases = []
    for res in (2.0 ** -5, 0.04):
        r = lambda k: F(F(k) + F(0.5)) * F(res)
        b = (F(0.5078125), F(0.2578125), F(1.0))
        o = (int(cell(b[0], res)), int(cell(b[1], res)))
        guard = _guard_for(0.5, r(10))
        for vname, variance in (("", None), ("-var", dict(H_BASE, sigma0=0.5, var_max=1.0))):
            vis = dict(margin=0.0625, end_guard=float(guard), stride=1, sigmas=2.0 if variance else 0.0, sensor_pos=(0.0, 0.0, 0.0))
            S = settings(G, res, variance=variance, visibility=vis)
            shift = F(1.0) if variance else F(0.0)                                 # with v = 1/4 and sigmas = 2 the test is on h - 1

            def seq(rays, heights=None, stride=1, sensor=(0.0, 0.0, 0.0), S=S):
                """tick 0 fills the window; `heights` maps a sample index k of the first ray to "keep" (h == bound + margin) or "forget" (next float)"""
                S = dict(S, visibility=dict(S["visibility"], stride=stride, sensor_pos=sensor))
                fill = _fill_points(o, G, res, lambda a, c: F(-3.0 + (a * 5 + c) * 2.0 ** -9), rule=cell)
                fill = np.concatenate([fill, np.full((1, 3), NAN)])                # P = G G + 1 = 577: no multiple of the stride 3
                edges = []
                if heights:
                    probe = clean(dict(map=np.zeros((G, G), F), origin=np.array(o), var=np.full((G, G), F(0.25)) if variance else None), _qpos(b), rays, S)
                    for (i, j) in zip(*np.nonzero(~np.isnan(probe["bound"]))):
                        T = F(probe["bound"][i, j] + F(vis["margin"]))              # the verdict is fl32(h - shift) > T
                        thr = F(T + shift)
                        while F(thr - shift) > T:
                            thr = dn(thr)
                        while F(up(thr) - shift) <= T:
                            thr = up(thr)                                          # the last h that is kept; h == T without a variance layer
                        assert shift != 0 or thr == T
                        kind = heights[(i + j) % len(heights)]
                        wa, wb = (o[0] - G // 2) + (i - (o[0] - G // 2)) % G, (o[1] - G // 2) + (j - (o[1] - G // 2)) % G
                        idx = (wa - (o[0] - G // 2)) * G + (wb - (o[1] - G // 2))
                        fill[idx, 2] = thr if kind == "keep" else up(thr)
                        edges.append((0, "points", idx, 2, 1 if kind == "keep" else -1))
                return [dict(op="tick", qpos=_qpos(b), points=fill, clear=True), dict(op="clean", qpos=_qpos(b), points=np.array(rays, F))], edges, S

            def add(name, rays, edges=(), **kw):
                ticks, e2, S2 = seq(np.array(rays, F), **kw)
                cases.append(_case(f"J-res{res:g}{vname}-{name}", "J", S2, ticks, list(edges) + e2))
            pad = [[np.nan] * 3] * 5
            xm = b[0] - F(0.5)                                                     # the end of the -x ray: the last float with fl32(x - sx) == -1/2
            while F(up(xm) - b[0]) == F(-0.5):
                xm = up(xm)
            down = [b[0] + F(0.5), b[1], b[2] - F(0.5)]                            # Lh = 1/2, the slope -1: z_k = bz - r_k
            add("guard-on", [down] + pad, [(1, "points", 0, 0, -1)], heights=("keep", "forget"))
            add("guard-below", [[dn(b[0] + F(0.5)), b[1], b[2]]] + pad, [(1, "points", 0, 0, 1)], heights=("forget", "keep"))
            add("minus-x", [[xm, b[1], b[2] - F(0.25)]] + pad, [(1, "points", 0, 0, 1)], heights=("keep", "forget", "forget"))
            add("plus-y", [[b[0], b[1] + F(0.5), b[2] - F(1.0)]] + pad, [(1, "points", 0, 1, -1)], heights=("forget", "keep"))
            add("no-length", [[b[0], b[1], b[2] - F(1.0)], [b[0] + F(0.0625), b[1], b[2] - F(1.0)], [b[0], b[1] - F(0.0625), -5.0]] + pad[:3])
            seven = [down, [b[0] - F(0.5), b[1], -9.0], [b[0], b[1] - F(0.5), -9.0], [b[0], b[1] + F(0.5), b[2] - F(1.0)], [b[0] - F(0.5), b[1], -9.0],
                     [b[0], b[1] - F(0.5), -9.0], [xm, b[1], b[2]]]
            # P = 577 points and a stride of 3: the points 0, 3, ..., 576 cast a ray, the last of them the point the buffer ends with
            last = G * G
            add("stride3-P577", seven[:6] + [[np.nan] * 3] * (last - 6) + seven[6:],
                [(1, "points", 0, 0, -1), (1, "points", 3, 1, -1), (1, "points", last, 0, 1)], stride=3, heights=("forget", "keep"))
            if not variance and res == 0.04:
                # the base at fl32(1.3): four of the ray's eleven samples are floats that floor(x / res) and floor(x * (1 / res)) put into different
                # cells, so the bound layer says which rule the kernel uses
                keep = b, o
                b = (F(1.3), b[1], b[2])
                o = (int(cell(b[0], res)), int(cell(b[1], res)))
                assert F(F(b[0] + F(0.5)) - b[0]) == F(0.5)
                add("rules-apart", [[F(b[0] + F(0.5)), b[1], b[2] - F(0.5)]] + pad, [(1, "points", 0, 0, -1)], heights=("keep", "forget"))
                cases[-1]["border_samples"] = True                                 # its samples sit ON borders: the fp64 reference is in doubt there
                b, o = keep
            if not variance:
                # the sensor 1.5 m behind the base: the ray enters the window at sample 36 and the cap of 2 G = 48 samples ends it inside
                far_ray = [[b[0] - F(1.5) + F(4.0), b[1], b[2] - F(2.0)]] + pad
                add("cap-2G", far_ray, sensor=(-1.5, 0.0, 0.0), heights=("keep", "forget"))
    return cases


FAMILIES = dict(A=family_a, B=family_b, C=family_c, D=family_d, E=family_e, F=family_f, G=family_g, H=family_h, J=family_j)
_cache = {}


def family(name):
    """the cases of one family, built once"""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def batches(cases, limit=63):
    """cases that share settings, the ops of their ticks and the shapes of their inputs, in groups of at most `limit` (a launch of limit + 1 envs:
    env 0 is a second copy of the last case, so that every case sits at a non-zero batch position)"""
    groups = {}
    for c in cases:
        shape = tuple((t["op"], np.shape(t.get("points", t.get("image")))) for t in c["ticks"])
        groups.setdefault(repr((sorted(c["S"].items(), key=str), shape)), []).append(c)
    out = []
    for g in groups.values():
        out += [g[i:i + limit] for i in range(0, len(g), limit)]
    return out
