"""Plain numpy statement of the hole filling of include/pgtt_elevation.h (pgtt_elevation_fill) for ONE env, over the geometry of
tests/elevation_reference.py: the Jacobi passes on the window, the minimum in the order of the tick's integer key, and the scan sampled from the
filled window.  Everything is fp32 bits in and out: the fill moves values, it computes none, and `est` is one fp32 subtraction.  No GPU, no test
module imported."""
import numpy as np

import elevation_reference as ref

UNKNOWN = 255
NO_KEY = np.int64(1) << 32                      # above every key


def key_of(x):
    """fp32 -> the key whose unsigned order is the order of the floats (key_of in pgtt_elevation.hip): -0 < +0, the infinities are the ends"""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b >> 31, b ^ 0xffffffff, b ^ 0x80000000)


def value_of(k):
    k = np.asarray(k, np.int64)
    b = np.where(k >> 31, k ^ 0x80000000, k ^ 0xffffffff)
    return b.astype(np.uint32).view(np.float32)


def window_slots(origin, G):
    """(sx [G], sy [G]): the slot row of window row a, the slot column of window column b"""
    lo = np.asarray(origin, np.int64) - G // 2
    return (lo[0] + np.arange(G)) % G, (lo[1] + np.arange(G)) % G


def to_window(slots, origin):
    """[G, G] in the map's slot layout -> [G, G] in window order (a, b)"""
    sx, sy = window_slots(origin, slots.shape[0])
    return slots[np.ix_(sx, sy)]


def to_slots(window, origin):
    sx, sy = window_slots(origin, window.shape[0])
    out = np.empty_like(window)
    out[np.ix_(sx, sy)] = window
    return out


def fill_window(W, K):
    """the passes on a window-ordered fp32 [G, G] (NaN = unknown) -> (W filled, D uint8)"""
    W = np.array(W, np.float32)
    G = W.shape[0]
    D = np.where(np.isnan(W), UNKNOWN, 0).astype(np.int64)
    key = key_of(W)
    for p in range(1, K + 1):
        src = np.full((G + 2, G + 2), NO_KEY)                       # the window's edges are edges: a border that is never a source
        src[1:-1, 1:-1] = np.where(D < p, key, NO_KEY)
        best = np.full((G, G), NO_KEY)
        for da in (0, 1, 2):
            for db in (0, 1, 2):
                if (da, db) != (1, 1):
                    best = np.minimum(best, src[da:da + G, db:db + G])
        new = (D == UNKNOWN) & (best < NO_KEY)                       # a Jacobi pass: `src` was taken before anything of this pass was written
        if not new.any():
            break
        key = np.where(new, best, key)
        D = np.where(new, p, D)
    out = np.where(D == UNKNOWN, W, value_of(np.where(D == UNKNOWN, 0, key)))
    return out.astype(np.float32), D.astype(np.uint8)


def fill(hmap, origin, K):
    """hmap [G, G] fp32 in the slot layout, origin [2] -> dict(map, dist: slot layout; W, D: window order)"""
    W, D = fill_window(to_window(np.asarray(hmap, np.float32), origin), K)
    return dict(map=to_slots(W, origin), dist=to_slots(D, origin), W=W, D=D)


def sample(filled, dist, origin, qpos, cfg):
    """the scan on a filled window (slot layout) -> dict(est fp32 [117], dist uint8 [117], z fp32, zmin, margin [117], cell)"""
    G = filled.shape[0]
    geo = ref.sample(np.full((G, G), np.nan), origin, qpos, cfg)      # the geometry alone: cells and margins
    c = geo["cell"]
    rel = c - (np.asarray(origin, np.int64) - G // 2)
    inside = ((rel >= 0) & (rel < G)).all(1)
    d = np.where(inside, dist[c[:, 0] % G, c[:, 1] % G], UNKNOWN).astype(np.uint8)
    z = np.where(inside, filled[c[:, 0] % G, c[:, 1] % G], np.float32(0)).astype(np.float32)
    known = d != UNKNOWN
    zmin = value_of(key_of(z[known]).min())[()] if known.any() else np.float32(0)
    z = np.where(known, z, zmin).astype(np.float32)
    with np.errstate(invalid="ignore"):
        est = (z - np.float32(zmin)).astype(np.float32)              # inf - inf is a NaN on both sides
    return dict(est=est, dist=d, z=z, zmin=zmin, margin=geo["margin"], cell=c, xy=geo["xy"])


def assemble(obs, est, row0=38):
    return np.concatenate([obs[:row0], est, obs[row0 + ref.NSCAN:]]).astype(np.float32)


def chebyshev(known):
    """[G, G] bool (window order) -> [G, G] the Chebyshev distance to the nearest True cell, by brute force; a large number when there is none"""
    G = known.shape[0]
    a, b = np.nonzero(known)
    if not len(a):
        return np.full((G, G), 10 ** 6)
    i, j = np.mgrid[0:G, 0:G]
    return np.maximum(np.abs(i[..., None] - a), np.abs(j[..., None] - b)).min(-1)
