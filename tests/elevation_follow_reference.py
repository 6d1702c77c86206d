"""Numpy statement of pgtt_elevation_follow() (include/pgtt_elevation.h, "Following a slower sensor") for ONE env, composed from the references of the
calls it chooses between: elevation_reference.tick / elevation_points_reference.tick on a fresh call, and on a hold call elevation_reference.sample's
geometry on the map as it stands.  A hold computes nothing but `est`, one fp32 subtraction of two of the map's values, so `hold` works on the fp32
bits of the map it is given and the device can be held to it bit for bit wherever no scan point is within a rounding error of a cell border
(sample's `margin` says how far each is).  No GPU, no test module imported."""
import numpy as np

import elevation_points_reference as pref
import elevation_reference as ref

NSCAN = ref.NSCAN
CLAMP = 1 << 30


def fresh(counter, every, force=False):
    """the sensor's rule seen from behind the sensor's call: `counter` is the sensor's counter AFTER that call, c = counter - 1 its value before"""
    c = int(counter) - 1
    return bool(force) or (c >= 0 and c % int(every) == 0)


def hold(state, qpos, cfg, clear=False, obs=None):
    """one hold call.  state = (map [G, G], origin [2]) as the last call left it (not modified); the map's values are taken as fp32.
    -> dict(map fp32, origin, est fp32 [117], known [117] bool, obs_out (when obs is given), scan (elevation_reference.sample's dict: cell, margin))"""
    hmap, origin = np.array(state[0], np.float32), np.array(state[1], np.int64)
    cfg = ref.as_device(cfg)
    qpos = np.asarray(qpos, float)
    G = hmap.shape[0]
    if clear:
        hmap[:] = np.nan
        origin = ref.cell(qpos[0:2], cfg["res"])
    window = np.clip(origin, -CLAMP, CLAMP)                    # the stored origin is not rewritten; an absurd one is read as the clamp
    sc = ref.sample(hmap.astype(float), window, qpos, cfg)     # the geometry and `known`; its est is an fp64 difference, not used
    c, known = sc["cell"], sc["known"]
    z = hmap[c[:, 0] % G, c[:, 1] % G]
    est = np.zeros(NSCAN, np.float32)
    if known.any():
        est[known] = z[known] - z[known].min()                 # fp32 - fp32
    out = dict(map=hmap, origin=origin, est=est, known=known, scan=sc)
    if obs is not None:
        r0 = cfg.get("scan_row0", 38)
        out["obs_out"] = np.concatenate([np.asarray(obs, np.float32)[:r0], est, np.asarray(obs, np.float32)[r0 + NSCAN:]])
    return out


def follow(state, qpos, data, cfg, counter, every, force=False, clear=False, obs=None, points=False):
    """one pgtt_elevation_follow() call behind a sensor whose counter reads `counter` after its own call.  data: the depth image [H, W], or with
    points=True the world points [P, 3].  -> the dictionary of the tick (fresh) or of hold(), with "fresh" added"""
    if fresh(counter, every, force):
        out = (pref.tick if points else ref.tick)(state, qpos, data, cfg, clear=clear, obs=obs)
    else:
        out = hold(state, qpos, cfg, clear=clear, obs=obs)
    out["fresh"] = fresh(counter, every, force)
    return out
