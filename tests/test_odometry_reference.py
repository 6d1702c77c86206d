"""tests/odometry_reference.py, the fp64 statement of the odometry drift (include/pgtt_elevation.h), held to facts of its own: what all-zero
settings return, the closed forms of a constant yaw error and of a scale error, the variances of the two random walks inside a chi-square
quantile, the ranges of the per-episode draws, and the points transform against the one computed from the two poses' quaternions.  No GPU."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odometry_reference as oref  # noqa: E402

DT = 0.02


def random_walk(n, ticks, seed=0, step=0.03):
    """`ticks` + 1 states [7, n] (fp32 values): random start poses and raw quaternions, steps of up to `step` metres per axis"""
    rng = np.random.default_rng(seed)
    b = rng.uniform(-3, 3, (3, n))
    out = []
    for _ in range(ticks + 1):
        q = rng.normal(size=(4, n)) * rng.uniform(0.5, 2.0, n)
        out.append(np.concatenate([b, q]).astype(np.float32).astype(np.float64))
        b = b + rng.uniform(-step, step, (3, n))
    return out


def run(states, settings, seed=0, offset=0, counter0=0, points=None):
    """clear on the first state, then one step per further state -> the list of update() results"""
    n = states[0].shape[1]
    odo, res = np.zeros((n, oref.ODO_WORDS)), []
    for t, s in enumerate(states):
        res.append(oref.update(s, odo, settings, seed, offset, counter0 + t, clear=np.full(n, t == 0), points=points))
        odo = res[-1]["odo"]
    return res


def test_zero_settings_return_the_true_pose_by_value():
    states = random_walk(33, 12)
    pts = np.random.default_rng(1).uniform(-4, 4, (33, 7, 3))
    pts[3, 2, 1] = np.nan
    pts[5, 0, 0] = np.inf
    for r, s in zip(run(states, dict(oref.ZERO, dt=DT), seed=7, points=pts), states):
        assert np.array_equal(r["odo"][:, 0:4], np.zeros((33, 4))) and np.array_equal(r["odo"][:, 7:], np.zeros((33, 5)))
        assert np.array_equal(r["pose_est"], s) and np.array_equal(r["odo"][:, 4:7], s[0:3].T)
        ok = np.isfinite(pts).all(-1)
        assert np.array_equal(r["points_est"][ok], pts[ok]) and np.isnan(r["points_est"][~ok]).all() and (~ok).sum() == 2


def test_a_constant_yaw_error_rotates_the_path():
    """every sigma and the bias 0, psi set by hand: over a straight path L, e = (Rz(psi) - I) L"""
    n, psi = 5, np.array([0.1, -0.3, 0.5, 0.0, 1.2])
    step = np.array([0.031, -0.012, 0.004])
    s0 = random_walk(n, 0)[0]
    odo = oref.update(s0, np.zeros((n, 12)), dict(oref.ZERO, dt=DT), clear=np.ones(n, bool))["odo"]
    odo[:, 3] = psi
    for t in range(1, 26):
        s = s0.copy()
        s[0:3] += t * step[:, None]
        odo = oref.update(s, odo, dict(oref.ZERO, dt=DT), counter=t)["odo"]
    path = 25 * step
    want = np.stack([np.cos(psi) * path[0] - np.sin(psi) * path[1] - path[0], np.sin(psi) * path[0] + np.cos(psi) * path[1] - path[1], 0 * psi], 1)
    assert np.abs(odo[:, 0:3] - want).max() < 1e-6                       # s0 holds fp32 values: the steps are exact to 1e-7 only
    assert np.array_equal(odo[:, 3], psi)


def test_a_scale_error_alone_scales_the_path():
    states = random_walk(64, 15)
    res = run(states, dict(oref.ZERO, dt=DT, scale=0.05), seed=3)
    scale_e = res[0]["odo"][:, 7]
    assert (np.abs(scale_e) <= oref.f32(0.05)).all() and np.ptp(scale_e) > 0.05
    path = (states[-1] - states[0])[0:3].T
    assert np.abs(res[-1]["odo"][:, 0:3] - scale_e[:, None] * path).max() < 1e-12
    assert np.array_equal(res[-1]["odo"][:, 7], scale_e) and np.array_equal(res[-1]["odo"][:, 3], np.zeros(64))


def chi_square_band(dof, z):
    """the Wilson-Hilferty quantiles of chi-square(dof) / dof at the standard-normal quantiles -z and +z"""
    a = 2.0 / (9.0 * dof)
    return (1 - a - z * math.sqrt(a)) ** 3, (1 - a + z * math.sqrt(a)) ** 3


def test_the_random_walks_have_the_stated_variances():
    """4096 envs at constant speed: psi is a sum of K independent N(0, sigma_yaw^2 dt), e_x (with no yaw error) a sum of K independent
    N(0, sigma_xy^2 L), so (N - 1) s^2 / var is chi-square with N - 1 degrees of freedom.  The band is its +-4.5 sigma quantile pair (two-sided
    7e-6), derived from the env count; the means are held to 4.5 standard errors."""
    n, K, z = 4096, 24, 4.5
    lo, hi = chi_square_band(n - 1, z)
    assert 0.85 < lo < 1 < hi < 1.15
    s0 = random_walk(n, 0)[0]
    step = np.array([0.03, 0.04, 0.0])                                    # L = 0.05 m per tick
    states = []
    for t in range(K + 1):
        s = s0.copy()
        s[0:3] += t * step[:, None]
        states.append(s)
    Lsum = sum(np.sqrt((((b - a)[0:3]) ** 2).sum(0)) for a, b in zip(states, states[1:]))     # per env: fp32 start values make it 0.05 K to 1e-6
    yaw = run(states, dict(oref.ZERO, dt=DT, sigma_yaw=0.1), seed=11)[-1]["odo"][:, 3]
    var = K * oref.f32(0.1) ** 2 * oref.f32(DT)
    assert lo < yaw.var(ddof=1) / var < hi, yaw.var(ddof=1) / var
    assert abs(yaw.mean()) < z * math.sqrt(var / n)
    ex = run(states, dict(oref.ZERO, dt=DT, sigma_xy=0.02), seed=11)[-1]["odo"][:, 0]
    ratio = (ex / (oref.f32(0.02) * np.sqrt(Lsum))).var(ddof=1)
    assert lo < ratio < hi, ratio
    assert abs(ex.mean()) < z * math.sqrt((oref.f32(0.02) ** 2 * Lsum.mean()) / n)


def test_episode_draws_lie_in_their_ranges_and_differ():
    n = 257
    s0 = random_walk(n, 0)[0]
    st = dict(oref.ZERO, dt=DT, scale=0.02, yaw_bias=0.005)
    a = oref.update(s0, np.ones((n, 12)), st, seed=5, counter=3, clear=np.ones(n, bool))["odo"]
    b = oref.update(s0, a, st, seed=5, counter=4, clear=np.ones(n, bool))["odo"]
    for o in (a, b):
        assert (np.abs(o[:, 7]) <= oref.f32(0.02)).all() and (np.abs(o[:, 8]) <= oref.f32(0.005)).all()
        assert len(np.unique(o[:, 7])) > n - 3 and len(np.unique(o[:, 8])) > n - 3          # between envs
        assert np.array_equal(o[:, 0:4], np.zeros((n, 4))) and np.array_equal(o[:, 4:7], s0[0:3].T) and np.array_equal(o[:, 9:], np.zeros((n, 3)))
    assert (a[:, 7] != b[:, 7]).mean() > 0.99 and (a[:, 8] != b[:, 8]).mean() > 0.99          # between episodes
    # an env that is not cleared keeps its draws, and the step's block is another one than the clear's
    c = oref.update(s0, a, st, seed=5, counter=4, clear=np.arange(n) % 2 == 0)["odo"]
    assert np.array_equal(c[1::2, 7:9], a[1::2, 7:9]) and np.array_equal(c[0::2, 7:9], b[0::2, 7:9])
    assert not np.array_equal(oref.uniforms(5, range(n), 4, 0), oref.uniforms(5, range(n), 4, 1))


def test_points_transform_is_the_one_of_the_two_poses():
    """points_est = R_est R_true^T (p - b) + b_est with the rotations of pose_est's and the state's quaternions"""
    n, P = 6, 40
    rng = np.random.default_rng(2)
    states = random_walk(n, 3, seed=4)
    pts = rng.uniform(-5, 5, (n, P, 3))
    res = run(states, dict(dt=DT, sigma_xy=0.05, sigma_z=0.02, sigma_yaw=0.3, yaw_bias=0.2, scale=0.1), seed=9, points=pts)
    r, s = res[-1], states[-1]
    assert np.abs(r["odo"][:, 3]).min() > 1e-3 and np.abs(r["odo"][:, 0:3]).max() > 1e-3
    for e in range(n):
        want = oref.register_by_quaternions(pts[e], s[3:7, e], s[0:3, e], r["pose_est"][3:7, e], r["pose_est"][0:3, e])
        assert np.abs(r["points_est"][e] - want).max() < 1e-12
        # the estimated quaternion keeps the raw one's norm, and roll and pitch: its rotation is Rz(psi) times the true one
        assert abs(np.linalg.norm(r["pose_est"][3:7, e]) - np.linalg.norm(s[3:7, e])) < 1e-12
