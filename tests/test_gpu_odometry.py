"""pgtt_elevation_odometry on the GPU, through the bare C ABI (include/pgtt_elevation.h, "Odometry drift"), against the fp64 statement of
tests/odometry_reference.py: one step on crafted states, all-zero settings, the draws, the clears, the points, the refusals and graph capture.
Every device buffer sits between guard bands of a sentinel at an odd offset of one allocation; the bands are held after every call.

Bars.  U = 2^-24, the unit roundoff of fp32; the device's own previous `odo` (fp32) is taken as exact and the reference is run on it, so a bar
covers ONE call.  They are sums of the roundings the header's order implies, on the reference's operand magnitudes, and are not tuned to the output
(a fused multiply-add only removes a rounding).  With c, s = cos, sin of the old psi (2 U absolute each: sincosf, the figure
tests/test_gpu_acting_edges.py uses), D = b - prev (U |D|), D' = (1 + scale_e) D (3 U |D'|: the sum, the product, D's own), rot = the rotated D',
noise = sigma sqrtf(L) n with sqrtf(L) = sqrtf(sqrtf(sum of squares)) (3 U relative), the draw n held to 8 U r (r its Box-Muller radius: the
draw bar of test_gpu_acting_edges.py, and the half-turn cosine and sine the kernel uses carry no rounding of the angle):
    e_x, e_y:  U (6 (|D'x| + |D'y|) + |rot| + |D| + |rot - D| + 5 |noise| + |step| + |e_new|) + 8 U sigma_xy sqrt(L) r
    e_z:       U (3 |D'z| + |Dz| + |D'z - Dz| + 5 |noise| + |step| + |e_new|) + 8 U sigma_z sqrt(L) r
    psi:       U (|bias_e dt| + 3 |noise| + |step| + |psi_new|) + 8 U sigma_yaw sqrt(dt) r
    pose_est position:   the bar of e + U |b + e|
    pose_est quaternion: (3 U + bar_psi / 2) (|q_a| + |q_b|) + U |result| for result = cos(psi/2) q_a -+ sin(psi/2) q_b
    points_est x, y:     (4 U + bar_psi) (|r_x| + |r_y|) + U (|rot| + |r| + |rot - r| + |p + (rot - r)| + |result|) + the bar of e
    points_est z:        U |result| + the bar of e_z
prev, the untouched words, the reserved words, a cleared env and everything under all-zero settings are held exactly.
Measured on an MI355X: the printed worst error / bar per quantity."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odometry_reference as oref  # noqa: E402

from phase_guided_terrain_traversal_amd import elevation  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DRAW_ULPS = 8                                   # tests/test_gpu_acting_edges.py
SENTINEL = -777.25
LO, HI = 37, 29                                 # guard bands, in elements: an odd offset
DT = 0.02
SETTINGS = dict(dt=DT, sigma_xy=0.02, sigma_z=0.01, sigma_yaw=0.01, yaw_bias=0.005, scale=0.02)
SEED = 0x9E3779B97F4A7C15


class Guarded:
    """`shape` elements of dtype between two bands of SENTINEL in one allocation; `t` is the view the library gets"""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        n = int(np.prod(shape))
        self.sentinel = SENTINEL if dtype.is_floating_point else -777
        self.all = torch.full((LO + n + HI,), self.sentinel, dtype=dtype, device="cuda:0")
        self.t = self.all[LO:LO + n].view(*shape)
        if fill is not None:
            self.t.fill_(fill)
        self.n = n

    def intact(self):
        return bool((self.all[:LO] == self.sentinel).all() and (self.all[LO + self.n:] == self.sentinel).all())

    def ptr(self):
        return self.t.data_ptr()


class Odo:
    """a handle for n envs with an odometry bound on guarded buffers the test fills"""

    def __init__(self, n, P=0, settings=SETTINGS, seed=SEED, offset=0, counter=0, done=False, bind=True):
        self.n, self.P, self.settings, self.seed, self.offset = n, P, dict(settings), seed, offset
        self.L = elevation.lib()
        self.h = C.c_void_p()
        cfg = elevation.config_struct(**elevation.PLACEHOLDER_CAMERA)
        elevation.check(self.L.pgtt_elevation_create(C.byref(cfg), 0, n, C.byref(self.h)))
        self.state, self.pose, self.odo = Guarded((7, n), fill=0.0), Guarded((7, n)), Guarded((n, 12), fill=0.0)
        self.counter = Guarded((1,), torch.int64, fill=counter)             # element LO of an int64 allocation: 8-byte aligned, odd in elements
        self.done = Guarded((n,), fill=0.0) if done else None
        self.points = Guarded((n, P, 3), fill=0.0) if P else None
        self.points_est = Guarded((n, P, 3)) if P else None
        self.bufs = [b for b in (self.state, self.pose, self.odo, self.counter, self.done, self.points, self.points_est) if b is not None]
        if bind:
            assert self.bind() == 0, self.error()

    def struct(self, **over):
        kw = dict(state=self.state.ptr(), done=self.done.ptr() if self.done else None, points=self.points.ptr() if self.P else None,
                  points_est=self.points_est.ptr() if self.P else None, P=self.P, pose_est=self.pose.ptr(), odo=self.odo.ptr(),
                  counter=self.counter.ptr(), seed=self.seed, env_id_offset=self.offset, **self.settings)
        kw.update(over)
        return elevation.odometry_struct(**kw)

    def bind(self, **over):
        return self.L.pgtt_elevation_bind_odometry(self.h, C.byref(self.struct(**over)))

    def error(self):
        return self.L.pgtt_elevation_last_error().decode()

    def put(self, state=None, odo=None, points=None, done=None):
        for buf, v in ((self.state, state), (self.odo, odo), (self.points, points), (self.done, done)):
            if v is not None:
                buf.t.copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32)))

    def call(self, mask=None, clear_all=False, use_done=False):
        m = None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).cuda()
        rc = self.L.pgtt_elevation_odometry(self.h, None if m is None else m.data_ptr(), int(clear_all), int(use_done),
                                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def get(self):
        out = dict(odo=self.odo.t.cpu().numpy().copy(), pose=self.pose.t.cpu().numpy().copy(), counter=int(self.counter.t.item()))
        if self.P:
            out["points"] = self.points_est.t.cpu().numpy().copy()
        return out

    def intact(self):
        return all(b.intact() for b in self.bufs)

    def close(self):
        self.L.pgtt_elevation_destroy(self.h)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def crafted(n, rng):
    """(state [7, n], odo [n, 12]) as fp32: random poses with raw quaternions, D = b - prev from 0 to 5 cm per axis (env 0: exactly 0), psi up to
    +-0.5, errors up to +-0.3 m, the episode's draws inside the default ranges, and the reserved words seeded with something that is not 0"""
    state = np.concatenate([rng.uniform(-3, 3, (3, n)), rng.normal(size=(4, n)) * rng.uniform(0.5, 2.0, n)]).astype(np.float32)
    odo = np.zeros((n, 12), np.float32)
    odo[:, 0:3], odo[:, 3] = rng.uniform(-0.3, 0.3, (n, 3)), rng.uniform(-0.5, 0.5, n)
    D = rng.uniform(0, 0.05, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    D[0] = 0.0
    odo[:, 4:7] = state[0:3].T - D
    odo[:, 7], odo[:, 8], odo[:, 9:] = rng.uniform(-0.02, 0.02, n), rng.uniform(-0.005, 0.005, n), 5.5
    return state, odo


def step_bars(ref, before, state, s):
    """(bar_e [n, 3], bar_psi [n], bar_pos [n, 3], bar_quat [4, n]) of one step, per the module docstring, from the reference's own numbers"""
    s = {k: oref.f32(v) for k, v in s.items()}
    psi, D, Dp, n, r = before[:, 3].astype(float), ref["D"], ref["Dp"], ref["n"], ref["r"]
    c, sn, sl = np.cos(psi), np.sin(psi), np.sqrt(ref["L"])
    rot = np.stack([c * Dp[:, 0] - sn * Dp[:, 1], sn * Dp[:, 0] + c * Dp[:, 1]], 1)
    new = ref["odo"]
    bar_e = np.zeros((len(psi), 3))
    for k in range(2):
        noise = s["sigma_xy"] * sl * n[:, k]
        bar_e[:, k] = U * (6 * (np.abs(Dp[:, 0]) + np.abs(Dp[:, 1])) + np.abs(rot[:, k]) + np.abs(D[:, k]) + np.abs(rot[:, k] - D[:, k])
                           + 5 * np.abs(noise) + np.abs(ref["step_e"][:, k]) + np.abs(new[:, k])) + DRAW_ULPS * U * s["sigma_xy"] * sl * r[:, k]
    noise = s["sigma_z"] * sl * n[:, 2]
    bar_e[:, 2] = U * (3 * np.abs(Dp[:, 2]) + np.abs(D[:, 2]) + np.abs(Dp[:, 2] - D[:, 2]) + 5 * np.abs(noise) + np.abs(ref["step_e"][:, 2])
                       + np.abs(new[:, 2])) + DRAW_ULPS * U * s["sigma_z"] * sl * r[:, 2]
    noise = s["sigma_yaw"] * np.sqrt(s["dt"]) * n[:, 3]
    bar_psi = U * (np.abs(before[:, 8] * s["dt"]) + 3 * np.abs(noise) + np.abs(ref["step_psi"]) + np.abs(new[:, 3])) \
        + DRAW_ULPS * U * s["sigma_yaw"] * np.sqrt(s["dt"]) * r[:, 3]
    bar_pos = bar_e + U * np.abs(ref["pose_est"][0:3].T)
    q = np.abs(state[3:7].astype(float))
    pair = np.stack([q[0] + q[3], q[1] + q[2], q[2] + q[1], q[3] + q[0]])
    bar_quat = (3 * U + bar_psi / 2) * pair + U * np.abs(ref["pose_est"][3:7])
    return bar_e, bar_psi, bar_pos, bar_quat


def points_bars(ref, pts, state, bar_e, bar_psi):
    """[n, P, 3] for the finite points, per the module docstring"""
    b, psi, e = state[0:3].T.astype(float)[:, None, :], ref["odo"][:, 3][:, None], ref["odo"][:, 0:3][:, None, :]
    with np.errstate(invalid="ignore"):
        r = pts.astype(float) - b
        c, s = np.cos(psi), np.sin(psi)
        rot = np.stack([c * r[..., 0] - s * r[..., 1], s * r[..., 0] + c * r[..., 1]], -1)
        bar = np.zeros(pts.shape)
        for k in range(2):
            mid = pts[..., k].astype(float) + (rot[..., k] - r[..., k])
            bar[..., k] = (4 * U + bar_psi[:, None]) * (np.abs(r[..., 0]) + np.abs(r[..., 1])) + U * (np.abs(rot[..., k]) + np.abs(r[..., k])
                                                                                                  + np.abs(rot[..., k] - r[..., k]) + np.abs(mid)
                                                                                                  + np.abs(mid + e[..., k])) + bar_e[:, None, k]
        bar[..., 2] = U * np.abs(pts[..., 2].astype(float) + e[..., 2]) + bar_e[:, None, 2]
    return bar


def worst(err, bar):
    ok = bar > 0
    assert (err[~ok] == 0).all()
    ratio = float((err[ok] / bar[ok]).max()) if ok.any() else 0.0
    assert ratio <= 1, ratio
    return ratio


def check_step(o, before, state, counter, pts=None):
    """the device's outputs after one step call (nobody cleared) against the reference run on `before` -> the worst error / bar per quantity"""
    got = o.get()
    ref = oref.update(state, before, o.settings, o.seed, o.offset, counter, points=pts)
    bar_e, bar_psi, bar_pos, bar_quat = step_bars(ref, before, state, o.settings)
    res = dict(e=worst(np.abs(got["odo"][:, 0:3] - ref["odo"][:, 0:3]), bar_e), psi=worst(np.abs(got["odo"][:, 3] - ref["odo"][:, 3]), bar_psi),
               pos=worst(np.abs(got["pose"][0:3].T - ref["pose_est"][0:3].T), bar_pos), quat=worst(np.abs(got["pose"][3:7] - ref["pose_est"][3:7]), bar_quat))
    assert np.array_equal(bits(got["odo"][:, 4:7]), bits(state[0:3].T))                          # prev = b
    assert np.array_equal(bits(got["odo"][:, 7:9]), bits(before[:, 7:9]))                        # the episode's draws stay
    assert np.array_equal(got["odo"][:, 9:], np.zeros((o.n, 3), np.float32))                     # reserved: written as 0
    assert got["counter"] == counter + 1 and o.intact()
    if pts is not None:
        fin = np.isfinite(pts).all(-1)
        assert np.isnan(got["points"][~fin]).all() and np.isfinite(got["points"][fin]).all()
        bar = points_bars(ref, pts, state, bar_e, bar_psi)
        res["points"] = worst(np.abs(got["points"][fin] - ref["points_est"][fin]), bar[fin])
    return res


# ---------------------------------------------------------------- 1. one step against the reference
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_one_step_against_the_reference(n):
    """three consecutive calls on crafted states; before each the device's own odo is read back and taken as exact"""
    rng = np.random.default_rng(100 + n)
    state, odo = crafted(n, rng)
    o = Odo(n, counter=41)
    o.put(state, odo)
    for t in range(3):
        before = o.odo.t.cpu().numpy().copy()
        assert o.call() == 0, o.error()
        res = check_step(o, before, state, 41 + t)
        print(f"n {n} call {t}: worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
        step = rng.uniform(0, 0.05, (3, n)) * rng.choice([-1.0, 1.0], (3, n))
        state = state.copy()
        state[0:3] = (state[0:3] + step).astype(np.float32)
        state[3:7] = (rng.normal(size=(4, n)) * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        o.put(state)
    o.close()


# ---------------------------------------------------------------- 2. zero settings
@pytest.mark.parametrize("n,P", [(65, 0), (3, 257)])
def test_zero_settings_return_the_truth_by_value(n, P):
    rng = np.random.default_rng(7)
    o = Odo(n, P, settings=dict(oref.ZERO, dt=DT))
    pts = None
    if P:
        pts = rng.uniform(-6, 6, (n, P, 3)).astype(np.float32)
        pts[0, 3, 1], pts[1, 0, 0], pts[2, P - 1, 2], pts[2, 100] = np.nan, np.inf, -np.inf, np.nan
    state, _ = crafted(n, rng)
    for t in range(4):
        o.put(state, points=pts)
        assert o.call(clear_all=t == 0) == 0, o.error()
        got = o.get()
        assert (got["pose"] == state).all() and (got["odo"][:, 0:4] == 0).all() and (got["odo"][:, 7:] == 0).all()
        assert np.array_equal(bits(got["odo"][:, 4:7]), bits(state[0:3].T)) and o.intact()
        if P:
            fin = np.isfinite(pts).all(-1)
            assert (got["points"][fin] == pts[fin]).all() and np.isnan(got["points"][~fin]).all() and (~fin).sum() == 4
        state = state.copy()
        state[0:3] += rng.uniform(-0.05, 0.05, (3, n)).astype(np.float32)
        state[3:7] = rng.normal(size=(4, n)).astype(np.float32)
    o.close()


# ---------------------------------------------------------------- 3. the draws
def isolated_draws(n, seed, offset, counter):
    """(n_x, n_y, n_z, n_psi) [n, 4] as the kernel drew them: psi = 0, scale_e = bias_e = 0, D = (1/16, 0, 0) exactly (sqrtf(L) = 1/4), dt = 1/4,
    every sigma 1/2 - then e = n / 8 and psi = n_psi / 4 with every scale a power of two, so the quotient is the draw itself; and the episode's
    draws of a clear at the same counter, with scale = yaw_bias = 1/2"""
    st = dict(dt=0.25, sigma_xy=0.5, sigma_z=0.5, sigma_yaw=0.5, yaw_bias=0.5, scale=0.5)
    o = Odo(n, settings=st, seed=seed, offset=offset, counter=counter)
    state = np.zeros((7, n), np.float32)
    state[0], state[3] = 0.0625, 1.0
    o.put(state, np.zeros((n, 12), np.float32))
    assert o.call() == 0, o.error()
    got = o.get()
    draws = np.concatenate([got["odo"][:, 0:3].astype(float) * 8, got["odo"][:, 3:4].astype(float) * 4], 1)
    rows = np.concatenate([got["odo"], got["pose"].T], 1)
    o.counter.t.fill_(counter)
    assert o.call(clear_all=True) == 0
    episode = o.get()["odo"][:, 7:9].copy()
    assert o.intact()
    o.close()
    return draws, rows, episode


@pytest.mark.parametrize("counter", [0, 1, 2 ** 32 - 1, 2 ** 32])
@pytest.mark.parametrize("offset", [0, 1000003, 2 ** 31 + 5])
def test_draws_are_the_reference_draws(offset, counter):
    """the four normals of a step and the two uniforms of a clear against the reference's Philox blocks: seeds with and without a high word,
    env-id offsets up to 2^31 + 5, counters on both sides of 2^32 (the epoch is its low word)"""
    n, seen = 65, []
    for seed in (SEED, SEED & 0xFFFFFFFF):
        draws, rows, episode = isolated_draws(n, seed, offset, counter)
        ids = [offset + e for e in range(n)]
        want, r = oref.normals(oref.uniforms(seed, ids, counter, 0))
        ratio = worst(np.abs(draws - want), DRAW_ULPS * U * r)
        print(f"draws offset {offset} counter {counter} seed {seed:#x}: worst |n - n64| / (8 2^-24 r) = {ratio:.3f}")
        u = oref.uniforms(seed, ids, counter, 1)
        assert np.array_equal(episode.astype(float), 0.5 * (2 * u[:, 0:2] - 1))                  # exact: 2 u - 1 and the halving round nothing
        seen.append(draws)
    assert (seen[0] != seen[1]).mean() > 0.99                            # the seed's high word is part of the key
    if counter in (0, 2 ** 32 - 1):
        nxt, _, _ = isolated_draws(n, SEED, offset, counter + 1)
        assert (nxt != seen[0]).mean() > 0.99                            # c and c + 1 differ
    if counter == 2 ** 32:
        low, _, _ = isolated_draws(n, SEED, offset, 0)
        assert np.array_equal(low, seen[0])                              # (uint32) c


def test_an_env_alone_has_the_bits_of_its_place_in_a_batch():
    _, batch, ep_batch = isolated_draws(65, SEED, 1000003, 5)
    for k in (0, 1, 63, 64):
        _, one, ep_one = isolated_draws(1, SEED, 1000003 + k, 5)
        assert np.array_equal(bits(one[0]), bits(batch[k])) and np.array_equal(bits(ep_one[0]), bits(ep_batch[k])), k


# ---------------------------------------------------------------- 4. the clears
def test_clears():
    """clear_all, a mask, use_done with done, and use_done with a NULL done; a cleared env is the truth again with fresh episode draws, its
    neighbours step as they would have, and the counter advances by one per call"""
    n = 257
    rng = np.random.default_rng(3)
    state, odo = crafted(n, rng)
    picked = np.zeros(n, bool)
    picked[[0, 1, 63, 64, 130, 255, 256]] = True
    cases = [("clear_all", dict(clear_all=True), np.ones(n, bool), True), ("mask", dict(mask=picked), picked, True),
             ("use_done", dict(use_done=True), picked, True), ("use_done, NULL done", dict(use_done=True), np.zeros(n, bool), False),
             ("done without use_done", dict(), np.zeros(n, bool), True)]
    for c, (name, kw, cleared, with_done) in enumerate(cases):
        o = Odo(n, counter=7 + c, done=with_done)
        o.put(state, odo, done=picked.astype(np.float32) if with_done else None)
        assert o.call(**kw) == 0, o.error()
        got = o.get()
        ref = oref.update(state, odo, o.settings, o.seed, 0, 7 + c, clear=cleared)
        k = cleared
        assert (got["odo"][k, 0:4] == 0).all() and np.array_equal(bits(got["odo"][k, 4:7]), bits(state[0:3].T[k])), name
        assert np.array_equal(bits(got["pose"][:, k]), bits(state[:, k])), name               # the cosine of 0 is 1, the sine 0: q by value
        u = oref.uniforms(o.seed, range(n), 7 + c, 1)
        want = np.stack([np.float32(0.02) * (2 * u[:, 0] - 1).astype(np.float32), np.float32(0.005) * (2 * u[:, 1] - 1).astype(np.float32)], 1)
        assert np.array_equal(bits(got["odo"][k, 7:9]), bits(want[k])), name                  # one fp32 product each
        assert (got["odo"][:, 9:] == 0).all() and got["counter"] == 8 + c and o.intact(), name
        # the others made the step they would have made in a call that clears nobody
        bar_e, bar_psi, _, _ = step_bars(ref, odo, state, o.settings)
        worst(np.abs(got["odo"][~k, 0:3] - ref["odo"][~k, 0:3]), bar_e[~k])
        worst(np.abs(got["odo"][~k, 3] - ref["odo"][~k, 3]), bar_psi[~k])
        assert np.array_equal(bits(got["odo"][~k, 7:9]), bits(odo[~k, 7:9])), name
        if name == "mask":
            plain = Odo(n, counter=7 + c)
            plain.put(state, odo)
            assert plain.call() == 0
            assert np.array_equal(bits(plain.get()["odo"][~k]), bits(got["odo"][~k])) and np.array_equal(bits(plain.get()["pose"][:, ~k]), bits(got["pose"][:, ~k]))
            plain.close()
        o.close()


# ---------------------------------------------------------------- 5. the points
@pytest.mark.parametrize("P", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("n", [1, 3])
def test_points_against_the_reference(n, P):
    """one step with points: sizes around the tile of 256 points, rows that are not finite, and the same pose outputs as without points"""
    rng = np.random.default_rng(1000 * n + P)
    state, odo = crafted(n, rng)
    pts = (state[0:3].T[:, None, :] + rng.uniform(-6, 6, (n, P, 3))).astype(np.float32)
    if P > 1:                                                            # P = 1 keeps its one point per env finite
        for e, k, j, v in ((0, 0, 2, np.nan), (n - 1, P - 1, 0, np.inf), (n // 2, P // 2, 1, -np.inf), (0, P // 3, 0, np.nan)):
            pts[e, k, j] = v
    o = Odo(n, P, counter=2 ** 32 + 9)
    o.put(state, odo, points=pts)
    assert o.call() == 0, o.error()
    res = check_step(o, odo, state, 2 ** 32 + 9, pts)
    print(f"n {n} P {P}: worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    plain = Odo(n, counter=2 ** 32 + 9)
    plain.put(state, odo)
    assert plain.call() == 0
    assert np.array_equal(bits(plain.get()["odo"]), bits(o.get()["odo"])) and np.array_equal(bits(plain.get()["pose"]), bits(o.get()["pose"]))
    plain.close(); o.close()


# ---------------------------------------------------------------- 6. the refusals
def test_refusals_leave_everything_alone():
    o = Odo(5, P=4, bind=False)
    assert o.call() == -2 and "pgtt_elevation_bind_odometry" in o.error()                      # PGTT_E_STATE before the bind
    for name in ("state", "pose_est", "odo", "counter"):
        assert o.bind(**{name: None}) == -1 and "required" in o.error(), name
    assert o.bind(points_est=None) == -1 and "together" in o.error()
    assert o.bind(points=None) == -1 and "together" in o.error()
    assert o.bind(P=0) == -1 and "P >= 1" in o.error()
    for kw in (dict(dt=0.0), dict(sigma_z=-0.01), dict(sigma_yaw=float("nan")), dict(scale=1.0)):
        assert o.bind(**kw) == -1 and o.error(), kw
    assert o.L.pgtt_elevation_bind_odometry(o.h, None) == -1 and o.error()
    assert o.call() == -2                                                                       # a refused bind binds nothing
    torch.cuda.synchronize()
    assert o.intact() and (o.pose.t == SENTINEL).all() and (o.points_est.t == SENTINEL).all() and int(o.counter.t.item()) == 0
    # without points P is not looked at, and the binding survives a bind of the map's buffers
    assert o.bind(points=None, points_est=None, P=0) == 0
    assert o.call(clear_all=True) == 0 and int(o.counter.t.item()) == 1 and (o.points_est.t == SENTINEL).all() and o.intact()
    o.close()


# ---------------------------------------------------------------- 7. graph capture
def test_graph_replays_have_the_bits_of_eager_calls():
    """the call captured once and replayed five times against five eager calls: two kernel nodes in a line, no parallel branches"""
    n, P = 65, 300
    rng = np.random.default_rng(11)
    state, odo = crafted(n, rng)
    pts = rng.uniform(-6, 6, (n, P, 3)).astype(np.float32)
    a, b = Odo(n, P, counter=3), Odo(n, P, counter=3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                           # a warm-up launch outside the capture, on buffers that are reset below
        a.L.pgtt_elevation_odometry(a.h, None, 0, 0, s.cuda_stream)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    a.counter.t.fill_(3)
    for o in (a, b):
        o.put(state, odo, points=pts)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert a.L.pgtt_elevation_odometry(a.h, None, 0, 0, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    a.counter.t.fill_(3)
    a.put(state, odo, points=pts)
    for t in range(5):
        g.replay()
        assert b.call() == 0
        torch.cuda.synchronize()
        ga, gb = a.get(), b.get()
        for k in ("odo", "pose", "points"):
            assert np.array_equal(bits(ga[k]), bits(gb[k])), (k, t)
        assert ga["counter"] == gb["counter"] == 4 + t
        state = state.copy()
        state[0:3] += rng.uniform(-0.05, 0.05, (3, n)).astype(np.float32)
        for o in (a, b):
            o.put(state)
    assert not np.array_equal(ga["odo"][:, 0:4], odo[:, 0:4]) and a.intact() and b.intact()
    a.close(); b.close()
