"""fp64 numpy statement of include/pgtt_depth.h: the camera pose from the env's qpos (mjcf.kinematics_np), the ray grid, the plane, boxes,
spheres and capsules, the clamp, and the Philox noise.  Also the ambiguity mask of an image, computed from this reference alone: a pixel is
ambiguous when moving its ray by +-0.02 pixel in either image direction changes which primitive is nearest, or when its two nearest candidates
are within 1e-4 relative of each other.  No GPU, no test module imported (raycast_edge_cases.py is numpy alone)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_edge_cases as edge_cases  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, mjcf, render  # noqa: E402

RS_DEPTH = 32                         # include/pgtt_depth.h
ID_MISS, ID_PLANE, ID_BOX, ID_GEOM = -1, 0, 1, 1000
AMB_PIXEL, AMB_TIE = 0.02, 1e-4


def qmat(q):
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def pitch_quat(pitch_deg):
    """a camera pitched DOWN by pitch_deg: rotation about +y, which turns +x toward -z"""
    a = np.radians(pitch_deg) / 2
    return np.array([np.cos(a), 0.0, np.sin(a), 0.0])


def model_for_env(model, params=None, e=0):
    """the model with env e's hinge zero offsets (params rows P_QPOS0) in qpos0"""
    mm = dict(model)
    if params is not None:
        q0 = np.array(model["qpos0"], float)
        q0[7:] = params[abi.P_QPOS0:abi.P_QPOS0 + 12, e]
        mm["qpos0"] = q0
    return mm


def body_poses(model, qpos, params=None, e=0):
    xpos, xquat, _, _, _ = mjcf.kinematics_np(model_for_env(model, params, e), np.asarray(qpos, float))
    return xpos, xquat


def camera_basis(xpos, xquat, mount_body=0, mount_pos=(0, 0, 0), mount_quat=(1, 0, 0, 0)):
    """camera pose = body pose * mount pose; fwd = the camera frame's +x, up = its +z, right = fwd x up -> (pos, fwd, right, up)"""
    mq = np.asarray(mount_quat, float) / np.linalg.norm(mount_quat)
    R = qmat(qmul(xquat[mount_body], mq))
    fwd, up = R[:, 0], R[:, 2]
    return xpos[mount_body] + qmat(xquat[mount_body]) @ np.asarray(mount_pos, float), fwd, np.cross(fwd, up), up


def camera_rays(fwd, right, up, fovy, width, height, offset=(0.0, 0.0)):
    """unit ray directions [H * W, 3] through the pixel centres (+ offset in pixels): the formula of render.camera_rays"""
    th = np.tan(np.radians(float(fovy)) / 2)
    px = np.arange(width) + 0.5 + offset[0]
    py = np.arange(height) + 0.5 + offset[1]
    u = (2 * px / width - 1) * th * width / height
    v = (1 - 2 * py / height) * th
    d = fwd[None, None] + u[None, :, None] * right[None, None] + v[:, None, None] * up[None, None]
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)


# ---------------------------------------------------------------- primitives (ray o + t d, |d| = 1; a hit needs t > 0)
def hit_plane(o, d):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d[:, 2] != 0, -o[2] / d[:, 2], np.inf)
    return np.where(t > 0, t, np.inf)


def hit_box(o, d, c, A, h):
    """A: columns = the box's local axes in world coordinates; the entry distance (a ray that starts inside the box does not see it)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ol, dl = (o - c) @ A, d @ A
        t1, t2 = (-h - ol) / dl, (h - ol) / dl
        lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
    tn, tf = np.nanmax(lo, -1), np.nanmin(hi, -1)
    return np.where((tn <= tf) & (tn > 0), tn, np.inf)


def hit_sphere(o, d, c, r):
    oc = o - c
    b = np.sum(oc * d, -1)
    cc = np.sum(oc * oc, -1) - r * r
    disc = b * b - cc
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    return np.where((disc >= 0) & (t > 0), t, np.inf)


def hit_capsule(o, d, c, ax, r, hl):
    pa, ba = c - hl * ax, 2 * hl * ax
    oa = o - pa
    baba, bard, baoa = ba @ ba, d @ ba, oa @ ba
    rdoa, oaoa = np.sum(d * oa, -1), np.sum(oa * oa, -1)
    a = baba - bard * bard
    b = baba * rdoa - baoa * bard
    cc = baba * oaoa - baoa * baoa - r * r * baba
    h = b * b - a * cc
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (-b - np.sqrt(h)) / a
        y = baoa + t * bard
    body = (h >= 0) & (y > 0) & (y < baba)
    tb = np.where(body & (t > 0), t, np.inf)
    o2 = np.broadcast_to(o, d.shape)
    tc = np.where(y <= 0, hit_sphere(o2, d, pa, r), hit_sphere(o2, d, pa + ba, r))
    out = np.where(h < 0, np.inf, np.where(body, tb, tc))
    # within 1e-3 rad of the axis a, b and cc cancel, and at a = 0 the quadratic is 0 / 0 and picks the far cap: there the capsule is the union of
    # three pieces of raycast_edge_cases.py, which shares no expression with the above (tests/test_raycast_edge_cases.py compares the two elsewhere)
    along = a <= 1e-6 * baba
    if along.any():
        out[along] = edge_cases.hit_capsule(o2[along], d[along], c, ax, r, hl)
    return out


def terrain_boxes(tab_v):
    """rows [pos xyz, quat wxyz, half-size xyz] of one variant -> box dicts"""
    return [dict(c=np.asarray(r[0:3], float), A=qmat(r[3:7]), h=np.asarray(r[7:10], float)) for r in tab_v]


def place_geoms(xpos, xquat, geoms):
    out = []
    for g in geoms:
        b = g["body"]
        out.append(dict(type=g["type"], c=xpos[b] + qmat(xquat[b]) @ np.asarray(g["pos"], float), A=qmat(qmul(xquat[b], np.asarray(g["quat"], float))),
                        size=np.asarray(g["size"], float)))
    return out


def hit_geom(o, d, g):
    if g["type"] == render.SPHERE:
        return hit_sphere(o, d, g["c"], g["size"][0])
    if g["type"] == render.CAPSULE:
        return hit_capsule(o, d, g["c"], g["A"][:, 2], g["size"][0], g["size"][1])
    return hit_box(o, d, g["c"], g["A"], g["size"])


def cast(o, d, boxes=(), geoms=()):
    """-> (t of the nearest candidate [P] (inf = miss), its id [P], t of the second nearest [P])"""
    ts = [hit_plane(o, d)] + [hit_box(o, d, b["c"], b["A"], b["h"]) for b in boxes] + [hit_geom(o, d, g) for g in geoms]
    ids = np.array([ID_PLANE] + [ID_BOX + k for k in range(len(boxes))] + [ID_GEOM + k for k in range(len(geoms))])
    T = np.stack(ts, 1)
    order = np.argsort(T, 1, kind="stable")
    best = np.take_along_axis(T, order[:, :1], 1)[:, 0]
    second = np.take_along_axis(T, order[:, 1:2], 1)[:, 0] if T.shape[1] > 1 else np.full(len(best), np.inf)
    return best, np.where(np.isfinite(best), ids[order[:, 0]], ID_MISS), second


def depth_image(cam, fovy, width, height, near, far, boxes=(), geoms=()):
    """cam = (pos, fwd, right, up) -> dict(depth [H, W] clamped to [near, far] with far on a miss, id [H, W], ambiguous [H, W])"""
    o, fwd, right, up = cam
    res, amb = None, np.zeros(width * height, bool)
    for off in ((0, 0), (AMB_PIXEL, 0), (-AMB_PIXEL, 0), (0, AMB_PIXEL), (0, -AMB_PIXEL)):
        d = camera_rays(fwd, right, up, fovy, width, height, off)
        t, ids, second = cast(o, d, boxes, geoms)
        if res is None:
            with np.errstate(invalid="ignore"):
                z = np.where(ids >= 0, t * (d @ fwd), np.inf)
            res = dict(depth=np.clip(z, near, far).reshape(height, width), id=ids.reshape(height, width))
            first = ids
            amb |= (ids >= 0) & np.isfinite(second) & (second <= t * (1 + AMB_TIE))
        else:
            amb |= ids != first
    res["ambiguous"] = amb.reshape(height, width)
    return res


def env_image(model, qpos, cfg, terrain_v=None, geoms=None, params=None, e=0):
    """the image of one env: cfg = dict(width, height, fovy, near, far[, mount_body, mount_pos, mount_quat]); terrain_v: [B, 10] rows of the env's
    variant or None; geoms: the robot primitive dicts (render.default_robot_geoms form) when the robot is in the scene"""
    xpos, xquat = body_poses(model, qpos, params, e)
    cam = camera_basis(xpos, xquat, cfg.get("mount_body", 0), cfg.get("mount_pos", (0, 0, 0)), cfg.get("mount_quat", (1, 0, 0, 0)))
    return depth_image(cam, cfg["fovy"], cfg["width"], cfg["height"], cfg["near"], cfg["far"],
                       terrain_boxes(terrain_v) if terrain_v is not None else (), place_geoms(xpos, xquat, geoms) if geoms else ())


# ---------------------------------------------------------------- Philox4x32-10 and the sensor noise
def philox4x32_10(key, ctr):
    """key (k0, k1) ints, ctr [..., 4] uint32 -> [..., 4] uint32"""
    c = [np.asarray(ctr[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    M0, M1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, -1).astype(np.uint32)


def noise_uniforms(seed, env_id, counter, npix):
    """u_k = uniform(seed, env id, (uint32) counter, RS_DEPTH, 4 p + k), k = 0 .. 2 -> [npix, 3] exact multiples of 2^-24"""
    ctr = np.zeros((npix, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = env_id & 0xFFFFFFFF, counter & 0xFFFFFFFF, RS_DEPTH, np.arange(npix)
    w = philox4x32_10((seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), ctr)
    return (w[:, :3] >> 8).astype(np.float64) / 16777216.0


def apply_noise(depth, near, far, sigma, dropout, seed, env_id, counter):
    """depth [H, W] noise-free clamped values -> (noisy image, dropped mask)"""
    u = noise_uniforms(seed, env_id, counter, depth.size)
    dropped = (u[:, 0] < np.float64(np.float32(dropout))).reshape(depth.shape)
    z = (np.sqrt(-2 * np.log(1 - u[:, 1])) * np.cos(2 * np.pi * u[:, 2])).reshape(depth.shape)
    out = np.clip(depth * (1 + np.float64(np.float32(sigma)) * z), near, far)
    return np.where(dropped, far, out), dropped
