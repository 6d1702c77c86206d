"""fp64 numpy statement of the odometry drift of include/pgtt_elevation.h ("Odometry drift: the map on an estimated pose"): the error-state dead
reckoning per env, its Philox draws, the estimated pose and the re-registered points.  It stands on depth_reference.philox4x32_10 and rounds the
settings through fp32, as depth_reference.apply_noise does.  No GPU, no test module imported.

    odo [N, 12] = e_x, e_y, e_z, psi, prev_x, prev_y, prev_z, scale_e, bias_e, 0, 0, 0
    state [>= 7, N]: rows 0..2 the true base position b, rows 3..6 the true base quaternion q (wxyz, raw)
"""
import numpy as np

from depth_reference import philox4x32_10, qmat

RS_ODOMETRY = 34                      # include/pgtt_elevation.h
ODO_WORDS = 12
NAMES = ("dt", "sigma_xy", "sigma_z", "sigma_yaw", "yaw_bias", "scale")
ZERO = dict(sigma_xy=0.0, sigma_z=0.0, sigma_yaw=0.0, yaw_bias=0.0, scale=0.0)


def f32(x):
    return np.float64(np.float32(x))


def uniforms(seed, env_ids, counter, block):
    """u_0 .. u_3 of the block (global env id, (uint32) counter, RS_ODOMETRY, block) per env -> [N, 4], exact multiples of 2^-24"""
    ids = np.asarray(env_ids, dtype=object)
    ctr = np.zeros((len(ids), 4), np.uint32)
    ctr[:, 0] = np.array([int(g) & 0xFFFFFFFF for g in ids], np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = int(counter) & 0xFFFFFFFF, RS_ODOMETRY, block
    w = philox4x32_10((int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF), ctr)
    return (w >> 8).astype(np.float64) / 16777216.0


def normals(u):
    """[N, 4] uniforms -> (n [N, 4] = n_x, n_y, n_z, n_psi; r [N, 4] = the Box-Muller radius each came from)"""
    r01, r23 = np.sqrt(-2 * np.log(1 - u[:, 0])), np.sqrt(-2 * np.log(1 - u[:, 2]))
    n = np.stack([r01 * np.cos(2 * np.pi * u[:, 1]), r01 * np.sin(2 * np.pi * u[:, 1]),
                  r23 * np.cos(2 * np.pi * u[:, 3]), r23 * np.sin(2 * np.pi * u[:, 3])], 1)
    return n, np.stack([r01, r01, r23, r23], 1)


def qz_mul(psi, q):
    """qz(psi) (x) q for q [4, N] wxyz, qz = (cos psi/2, 0, 0, sin psi/2); not normalised"""
    c, s = np.cos(psi / 2), np.sin(psi / 2)
    return np.stack([c * q[0] - s * q[3], c * q[1] - s * q[2], c * q[2] + s * q[1], c * q[3] + s * q[0]])


def update(state, odo, settings, seed=0, env_id_offset=0, counter=0, clear=None, points=None):
    """one call.  state [>= 7, N], odo [N, 12] (the values before the call), settings: dt and the five of ZERO, clear: [N] bool or None (nobody),
    points [N, P, 3] or None -> dict(odo [N, 12], pose_est [7, N], points_est or None, and for the bars of a test: D [N, 3], L, n, r [N, 4], cleared)"""
    s = {k: f32(settings[k]) for k in NAMES}
    state, odo = np.asarray(state, np.float64), np.asarray(odo, np.float64)
    N = state.shape[1]
    clear = np.zeros(N, bool) if clear is None else np.asarray(clear, bool)
    ids = [int(env_id_offset) + e for e in range(N)]
    b, q = state[0:3].T, state[3:7]
    u_clear, u_step = uniforms(seed, ids, counter, 1), uniforms(seed, ids, counter, 0)
    n, r = normals(u_step)
    e, psi, prev, scale_e, bias_e = odo[:, 0:3], odo[:, 3], odo[:, 4:7], odo[:, 7], odo[:, 8]
    D = b - prev
    L = np.sqrt((D * D).sum(1))
    Dp = (1 + scale_e)[:, None] * D
    c, sn = np.cos(psi), np.sin(psi)
    step_e = np.stack([(c * Dp[:, 0] - sn * Dp[:, 1]) - D[:, 0] + s["sigma_xy"] * np.sqrt(L) * n[:, 0],
                       (sn * Dp[:, 0] + c * Dp[:, 1]) - D[:, 1] + s["sigma_xy"] * np.sqrt(L) * n[:, 1],
                       (Dp[:, 2] - D[:, 2]) + s["sigma_z"] * np.sqrt(L) * n[:, 2]], 1)
    step_psi = bias_e * s["dt"] + s["sigma_yaw"] * np.sqrt(s["dt"]) * n[:, 3]
    out = np.zeros((N, ODO_WORDS))
    out[:, 0:3] = np.where(clear[:, None], 0.0, e + step_e)
    out[:, 3] = np.where(clear, 0.0, psi + step_psi)
    out[:, 4:7] = b
    out[:, 7] = np.where(clear, s["scale"] * (2 * u_clear[:, 0] - 1), scale_e)
    out[:, 8] = np.where(clear, s["yaw_bias"] * (2 * u_clear[:, 1] - 1), bias_e)
    pose = np.concatenate([(b + out[:, 0:3]).T, qz_mul(out[:, 3], q)])
    pts = None
    if points is not None:
        pts = register(np.asarray(points, np.float64), b, out[:, 0:3], out[:, 3])
    return dict(odo=out, pose_est=pose, points_est=pts, D=D, L=L, n=n, r=r, cleared=clear, step_e=step_e, step_psi=step_psi, Dp=Dp)


def register(points, b, e, psi):
    """points_est = p + ((Rz(psi) r) - r) + e with r = p - b; a point with a coordinate that is not finite -> three NaNs.  points [N, P, 3]"""
    r = points - b[:, None, :]
    c, s = np.cos(psi)[:, None], np.sin(psi)[:, None]
    with np.errstate(invalid="ignore"):
        rot = np.stack([c * r[..., 0] - s * r[..., 1], s * r[..., 0] + c * r[..., 1], r[..., 2]], -1)
        out = points + (rot - r) + e[:, None, :]
    out[~np.isfinite(points).all(-1)] = np.nan
    return out


def register_by_quaternions(points, q_true, b_true, q_est, b_est):
    """the same transform from the two poses: R_est R_true^T (p - b_true) + b_est, for ONE env (points [P, 3], q wxyz of any norm)"""
    return (qmat(q_est) @ qmat(q_true).T @ (points - b_true).T).T + b_est
