"""fp64 numpy statement of "Sensor latency: capture-stamped fusion" (include/pgtt_elevation.h) for ONE env: the ring of frames and poses, the
integer draw of the latency, and the tick with two poses - steps 1, 2, 5 and 6 under the CURRENT pose, step 3 under the pose of the frame's
CAPTURE on the ring's frame, tested against the new window.  It is built from the pieces of tests/elevation_reference.py (unproject, cell, sample,
and so its doubtful_cells rule applies to what stamped_tick returns) and stands on depth_reference.philox4x32_10.  No GPU, no test module imported."""
import numpy as np

import depth_reference as dref
import elevation_reference as eref

RS_LATENCY = 35                        # include/pgtt_elevation.h
MAX_LATENCY = 8
NSCAN = eref.NSCAN


def draw(seed, env_ids, counter, lo, hi):
    """the latencies of envs cleared at a call that found the counter at `counter` -> [n] int64: lo + ((w0 * (hi - lo + 1)) >> 32), integers alone;
    w0 = word 0 of the block (global env id, (uint32) counter, RS_LATENCY, 0) under the key (seed lo, seed hi)"""
    ids = [int(g) & 0xFFFFFFFF for g in np.asarray(env_ids, dtype=object).reshape(-1)]
    ctr = np.zeros((len(ids), 4), np.uint32)
    ctr[:, 0] = np.array(ids, np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = int(counter) & 0xFFFFFFFF, RS_LATENCY, 0
    w = dref.philox4x32_10((int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF), ctr)
    return np.array([int(lo) + ((int(w0) * (int(hi) - int(lo) + 1)) >> 32) for w0 in w[:, 0]], np.int64)


def stamped_tick(state, qpos, capture, frame, cfg, clear=False, obs=None, points=False):
    """the tick with two poses for one env.  state = (map, origin) (not modified); qpos [7] the CURRENT pose; capture [7] the pose the frame was taken
    at and frame its image [H, W] (points: its world points [P, 3]) - both None when no frame is due: step 3 then admits nothing.  cfg as
    elevation_reference.tick's (the camera fields are not read with points).
    -> elevation_reference.tick's dictionary: per pixel (per point) valid, point, cell, margin, kept, self_margin - under the CAPTURE pose"""
    hmap, origin = np.array(state[0], float), np.array(state[1], np.int64)
    cfg = eref.as_device(cfg)
    G, res, alpha = hmap.shape[0], float(cfg["res"]), float(cfg["alpha"])
    qpos = np.asarray(qpos, float)
    # 1. clear, 2. recentre: the current pose
    new_origin = eref.cell(qpos[0:2], res)
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
    # 3. tick maximum: the capture pose, the ring's frame, the NEW window
    if frame is None:
        valid, p = np.zeros(0, bool), np.zeros((0, 3))
        cap = qpos
    else:
        cap = np.asarray(capture, float)
        if points:
            pts = np.asarray(frame, float).reshape(-1, 3)
            valid = np.isfinite(pts).all(1)
            p = np.where(valid[:, None], pts, 0.0)
        else:
            d = np.asarray(frame, float).reshape(-1)
            with np.errstate(invalid="ignore"):
                valid = (d > cfg["near"]) & (d < cfg["far"])
            p = eref.unproject(cap, np.where(valid, d, 1.0).reshape(np.shape(frame)), cfg)
    half = np.asarray(cfg.get("self_half", (0, 0, 0)), float)
    if half.any() and len(p):
        q = cap[3:7] / np.linalg.norm(cap[3:7])
        over = np.abs((p - cap[0:3]) @ dref.qmat(q)) - half                   # R^T (p - b) at capture; > 0 on an axis that puts the point outside
        inside_box = (over <= 0).all(1)
        self_margin = np.where(inside_box, (-over).min(1), over.max(1))
    else:
        inside_box, self_margin = np.zeros(len(p), bool), np.full(len(p), np.inf)
    kept = valid & ~inside_box
    c = eref.cell(p[:, :2], res)
    rel = c - lo
    use = kept & ((rel >= 0) & (rel < G)).all(1)
    m = np.full((G, G), -np.inf)
    np.maximum.at(m, (c[use, 0] % G, c[use, 1] % G), p[use, 2])
    touched = np.isfinite(m)
    # 4. fuse
    hmap[touched] = np.where(np.isnan(hmap[touched]), m[touched], hmap[touched] + alpha * (m[touched] - hmap[touched]))
    # 5. sample, 6. assemble: the current pose
    sc = eref.sample(hmap, origin, qpos, cfg)
    out = dict(map=hmap, origin=origin, est=sc["est"], known=sc["known"], touched=touched, scan=sc, valid=valid, point=p, cell=c,
               margin=eref.border_margin(p[:, :2], res) if len(p) else np.zeros(0), kept=kept, self_margin=self_margin)
    if obs is not None:
        r0 = cfg.get("scan_row0", 38)
        out["obs_out"] = np.concatenate([obs[:r0], sc["est"], obs[r0 + NSCAN:]])
    return out


class Delayed:
    """one env behind pgtt_elevation_delayed: its ring of D frames and poses, lat, age, and the map's state.  The counter is the caller's: every call
    is given the value the device's counter has BEFORE the call."""

    def __init__(self, G, lo, hi, seed=0, gid=0, D=None, points=False):
        assert 0 <= lo <= hi <= MAX_LATENCY
        self.D = hi + 1 if D is None else int(D)
        assert hi + 1 <= self.D <= MAX_LATENCY + 1
        self.lo, self.hi, self.seed, self.gid, self.points = lo, hi, seed, gid, points
        self.frames, self.poses = [None] * self.D, [None] * self.D
        self.lat, self.age = 0, 0
        self.state = eref.new_state(G)

    def call(self, c, qpos, frame, cfg, clear=False, obs=None):
        """one call that finds the counter at c -> stamped_tick's dictionary with lat, age, fused, slot (the slot pushed) and frame_slot (the slot
        fused, None without a frame)"""
        c = int(c)
        if clear:                                                            # 1. the clear rule
            self.lat, self.age = int(draw(self.seed, [self.gid], c, self.lo, self.hi)[0]), 0
        w = c % self.D                                                        # 2. push (Python's % is the floor-mod)
        self.frames[w], self.poses[w] = np.array(frame, copy=True), np.array(qpos, dtype=float, copy=True)
        self.age = min(self.age + 1, self.D)
        fused = self.lat < self.age                                           # 3. pick
        k = (c - self.lat) % self.D
        out = stamped_tick(self.state, qpos, self.poses[k] if fused else None, self.frames[k] if fused else None, cfg, clear=clear, obs=obs,
                           points=self.points)
        self.state = (out["map"], out["origin"])
        out.update(lat=self.lat, age=self.age, fused=fused, slot=w, frame_slot=k if fused else None)
        return out
