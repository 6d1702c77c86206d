"""Crafted single-env task steps that sit ON the task layer's branch edges, and the helpers every task-layer test shares (no GPU, no torch).

The task layer (observe_kernel<OBS_STEP>, or observe_kernel<OBS_STEP_OBS> + task_kernel; oracle/task_impl.h task_post) is a chain of selects and index
computations: termination, the command timer, the phase clock, the contact bookkeeping of four feet, twelve joint terms, the quadrant statistics of 117
scan cells, two histories, two reward clips.  A roll-out visits the edges of those selects by accident, if at all; the cases here place one env on each.

* `PostIn`, `pack_step_cases`, `post_in`, `oracle_task_post`: the packing of reference-generated records into the SoA buffers and the per-env call of
  the oracle's task layer (tests/test_golden_task.py, tests/test_gpu_golden.py and tests/test_gpu_fullsize.py import them from here).
* `edge_config(method, which)`: the shipped training config, or one with all 21 reward scales non-zero (the override recipe of
  tests/test_gpu_parity.py::test_config_values_are_read_not_assumed), history_update_steps = 3 and a lin_vel_z scale large enough for the upper clip.
* `build_cases(cfg, model)`: the cases.  Each starts from one plausible standing state in which the four feet and the twelve joints all carry different
  values, and moves only what it targets.  Every number is a float32: the device buffers hold nothing else, and both oracle builds are fed these bits.
* `TaskOracle`: runs a case through the fp32 or the fp64 build of the oracle.

A case whose input sits EXACTLY on a float32 threshold, where the fp64 build (which widens the float32 input and compares it with the double constant)
lands on the other side, carries `threshold` = the reason, worked out here from the number formats alone.  For those the fp32 build is the arbiter: it
states the reference's float32 comparison.  Every other case must be decided (both builds agree on every discrete output)."""
import ctypes as C

import numpy as np

from oracle import oracle
from phase_guided_terrain_traversal_amd import abi, configs

F32 = np.float32
PI32, TWO_PI32 = F32(np.pi), F32(2 * np.pi)
PHILOX_SEED = 0x5DEECE66D                       # != 0, and wider than 32 bits: both key words are in play
ENV_ID_OFFSETS = (0, 1000003, 2 ** 31 + 5)
METHODS, CONFIGS = ("pgtt", "baseline"), ("shipped", "allscales")


def below(x):
    return np.nextafter(F32(x), F32(-np.inf))


def above(x):
    return np.nextafter(F32(x), F32(np.inf))


class PostIn(C.Structure):
    d = C.c_double
    _fields_ = [("qpos", d * 19), ("qvel", d * 18), ("sensordata", d * 49), ("site_imu_mat", d * 9),
                ("site_foot_z", d * 4), ("actuator_force", d * 12), ("action", d * 12), ("scan_z", d * 117),
                ("contact", C.c_int32 * 4)]


def pack_step_cases(g, key_qpos, action_scale):
    """the reference-generated Joystick.step records `g` (conftest.GoldenCases) as the SoA buffers a step starts from: state [NSTATE][n], istate
    [NISTATE][n], frame [NFRAME][n], scan_z [n][117], action [n][12]"""
    n = g.ncases
    S = np.zeros((abi.NSTATE, n), np.float32); I = np.zeros((abi.NISTATE, n), np.int32)
    F = np.zeros((abi.NFRAME, n), np.float32); Z = np.zeros((n, abi.NSCAN), np.float32); A = np.zeros((n, 12), np.float32)
    key = np.asarray(key_qpos, dtype=np.float64)
    for i in range(n):
        k = lambda name: g[f"c{i}_{name}"]
        S[abi.S_QPOS:abi.S_QPOS + 19, i] = k("qpos"); S[abi.S_QVEL:abi.S_QVEL + 18, i] = k("qvel")
        S[abi.S_CMD:abi.S_CMD + 3, i] = k("in_command"); S[abi.S_PHASE:abi.S_PHASE + 4, i] = k("in_phase")
        S[abi.S_PHASE_DT, i] = k("in_phase_dt"); S[abi.S_GAIT_FREQ, i] = k("in_gait_freq")
        S[abi.S_LAST_ACT:abi.S_LAST_ACT + 12, i] = k("in_last_act"); S[abi.S_LAST_LAST_ACT:abi.S_LAST_LAST_ACT + 12, i] = k("in_last_last_act")
        S[abi.S_AIR_TIME:abi.S_AIR_TIME + 4, i] = k("in_feet_air_time"); S[abi.S_SWING_PEAK:abi.S_SWING_PEAK + 4, i] = k("in_swing_peak")
        S[abi.S_HMAX:abi.S_HMAX + 4, i] = k("in_H_max"); S[abi.S_HMIN:abi.S_HMIN + 4, i] = k("in_H_min")
        # info["motor_targets"] of THIS step (joystick_pgtt.py:145,149): what the physics kernel leaves in the row
        S[abi.S_MOTOR_TARGETS:abi.S_MOTOR_TARGETS + 12, i] = key[7:] + k("action") * action_scale
        S[abi.S_QERR_HIST:abi.S_QERR_HIST + 24, i] = k("in_qpos_error_history"); S[abi.S_QVEL_HIST:abi.S_QVEL_HIST + 24, i] = k("in_qvel_history")
        S[abi.S_LAST_CONTACT:abi.S_LAST_CONTACT + 4, i] = k("in_last_contact")
        I[abi.I_STEP, i] = int(k("in_step")); I[abi.I_STEPS_UNTIL_CMD, i] = int(k("in_steps_until_next_cmd"))
        s = k("sensordata")          # sensor layout of go2_mjx_feetonly.xml:258-274
        F[abi.F_GYRO:abi.F_GYRO + 3, i] = s[0:3]; F[abi.F_ACCEL:abi.F_ACCEL + 3, i] = s[3:6]
        F[abi.F_GLOBAL_LINVEL:abi.F_GLOBAL_LINVEL + 3, i] = s[13:16]; F[abi.F_GLOBAL_ANGVEL:abi.F_GLOBAL_ANGVEL + 3, i] = s[16:19]
        F[abi.F_LOCAL_LINVEL:abi.F_LOCAL_LINVEL + 3, i] = s[19:22]; F[abi.F_UPVECTOR:abi.F_UPVECTOR + 3, i] = s[22:25]
        F[abi.F_GRAVITY:abi.F_GRAVITY + 3, i] = -k("site_imu_mat")[2]             # imu_xmat^T (0, 0, -1), go2/base.py:129-131
        F[abi.F_FEET_POS:abi.F_FEET_POS + 12, i] = s[25:37]; F[abi.F_FEET_VEL:abi.F_FEET_VEL + 12, i] = s[37:49]
        F[abi.F_ACT_FORCE:abi.F_ACT_FORCE + 12, i] = k("actuator_force"); F[abi.F_CONTACT:abi.F_CONTACT + 4, i] = k("contact")
        F[abi.F_FOOT_SITE_Z:abi.F_FOOT_SITE_Z + 4, i] = k("site_foot_z")
        Z[i] = k("scan_z"); A[i] = k("action")
    return S, I, F, Z, A


def post_in(state_col, frame_col, scan_row, action_row):
    """what the oracle's task layer reads of a step's physics outputs (PgttOraclePostIn), from one env's buffers AFTER the physics: the state column
    (qpos, qvel), the 65-row sensor frame, the 117 scan heights, the action"""
    pin = PostIn()
    q = np.asarray(state_col[:19], dtype=np.float64)
    np.ctypeslib.as_array(pin.qpos)[:] = q
    np.ctypeslib.as_array(pin.qvel)[:] = state_col[19:37]
    Fr = frame_col
    sd = np.zeros(49)
    sd[0:3] = Fr[abi.F_GYRO:abi.F_GYRO + 3]; sd[3:6] = Fr[abi.F_ACCEL:abi.F_ACCEL + 3]; sd[6:10] = q[3:7]
    sd[13:16] = Fr[abi.F_GLOBAL_LINVEL:abi.F_GLOBAL_LINVEL + 3]; sd[16:19] = Fr[abi.F_GLOBAL_ANGVEL:abi.F_GLOBAL_ANGVEL + 3]
    sd[19:22] = Fr[abi.F_LOCAL_LINVEL:abi.F_LOCAL_LINVEL + 3]; sd[22:25] = Fr[abi.F_UPVECTOR:abi.F_UPVECTOR + 3]
    sd[25:37] = Fr[abi.F_FEET_POS:abi.F_FEET_POS + 12]; sd[37:49] = Fr[abi.F_FEET_VEL:abi.F_FEET_VEL + 12]
    np.ctypeslib.as_array(pin.sensordata)[:] = sd
    mat = np.zeros(9); mat[6:9] = -np.asarray(Fr[abi.F_GRAVITY:abi.F_GRAVITY + 3], dtype=np.float64)     # the task layer reads the IMU frame's third row only (gravity)
    np.ctypeslib.as_array(pin.site_imu_mat)[:] = mat
    np.ctypeslib.as_array(pin.site_foot_z)[:] = Fr[abi.F_FOOT_SITE_Z:abi.F_FOOT_SITE_Z + 4]
    np.ctypeslib.as_array(pin.actuator_force)[:] = Fr[abi.F_ACT_FORCE:abi.F_ACT_FORCE + 12]
    np.ctypeslib.as_array(pin.action)[:] = action_row
    np.ctypeslib.as_array(pin.scan_z)[:] = scan_row
    np.ctypeslib.as_array(pin.contact)[:] = np.asarray(Fr[abi.F_CONTACT:abi.F_CONTACT + 4]).astype(np.int32)
    return pin


def oracle_task_post(cs, ms, hb, pin, fp64, seed=0, env_id=0):
    """the oracle's task layer on ONE env: `hb` (oracle.HostBuffers(1)) holds the env's state / istate rows before the step and receives the rows after
    it, the observations, reward, done and metrics; `pin` the step's physics outputs; (seed, env_id) the env's Philox key"""
    L = oracle.lib()
    L.pgtt_oracle_task_post_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32]
    b = hb.struct()
    L.pgtt_oracle_task_post_ex(C.byref(cs), C.byref(ms), C.byref(b), C.byref(pin), int(fp64), C.c_uint64(seed), C.c_uint32(env_id & 0xFFFFFFFF))
    return hb


class TaskOracle:
    """one config + model; `run` = one case through one build of the oracle's task layer -> copies of everything a step writes"""

    def __init__(self, cfg, model, method):
        self.cs, self.ms, self.method = abi.config_struct(cfg), abi.model_struct(model), method
        self.hb = oracle.HostBuffers(1, method=method)
        L = oracle.lib()
        L.pgtt_oracle_set_rng_override_value.argtypes = [C.c_float]

    def run(self, S, I, F, Z, A, fp64, u=0.5, seed=0, env_id=0):
        """u: every uniform draw pinned to this value; None: the Philox draws of (seed, env_id, I[I_RNG_CTR])"""
        hb, L = self.hb, oracle.lib()
        hb["state"][:, 0] = S; hb["istate"][:, 0] = I
        try:
            if u is None:
                L.pgtt_oracle_set_rng_override(0)
            else:
                L.pgtt_oracle_set_rng_override_value(C.c_float(float(u)))
            oracle_task_post(self.cs, self.ms, hb, post_in(S, F, Z, A), fp64, seed, env_id)
        finally:
            L.pgtt_oracle_set_rng_override(0)
        return dict(obs=hb["obs_state"][0].copy(), priv=hb["obs_priv"][0].copy(), reward=float(hb["reward"][0]), done=float(hb["done"][0]),
                    metrics=hb["metrics"][:, 0].copy(), state=hb["state"][:, 0].copy(), istate=hb["istate"][:, 0].copy())


def edge_config(method, which):
    cfg = configs.training_config(method)
    if which == "shipped":
        return cfg
    assert which == "allscales"
    rng = np.random.default_rng(5)            # the recipe of test_config_values_are_read_not_assumed: every scale non-zero, every scalar off its default
    over = {"reward_config.scales." + k: float(np.sign(v if v != 0 else rng.choice([-1.0, 1.0])) * rng.uniform(0.2, 1.5) * (abs(v) if v != 0 else 0.3))
            for k, v in configs.default_config()["reward_config"]["scales"].items()}
    over.update({"reward_config.tracking_sigma": 0.31, "reward_config.swing_height": -0.17, "reward_config.base_feet_distance": -0.27, "reward_config.phase_sigma": 0.08,
                 "command_config.u_max": [0.9, 0.5, 0.8], "command_config.u_min": [-0.4, -0.6, -1.1], "command_config.b": [0.7, 0.4, 0.6], "gait_freq": [1.5, 2.5],
                 "scan_dist_x": 0.08, "scan_dist_y": 0.12, "scan_z_offset": 0.45, "action_scale": 0.35, "soft_joint_pos_limit_factor": 0.9, "history_update_steps": 3})
    over.update({"noise_config.scales." + k: v for k, v in dict(joint_pos=0.05, joint_vel=1.0, gyro=0.3, gravity=0.08, linvel=0.2, heightscan=0.02).items()})
    # the one large scale: lin_vel_z^2 * 4e4 * ctrl_dt passes 10000 at |v_z| > 3.54 m/s and stays ~0.8 at the standing state's 0.03125 m/s
    over["reward_config.scales.lin_vel_z"] = 4.0e4
    return configs.with_overrides(cfg, **over)


# ------------------------------------------------------------------ the independent statements the coverage counts use
def quadrant_of(cell):
    """joystick_pgtt.py:169-190 with n = 6 on both axes of the 13 x 9 grid: 0 top right, 1 top left, 2 back right, 3 back left, -1 = row 6 / column 6"""
    r, c = divmod(cell, abi.SCAN_W)
    top, back, left, right = r < 6, r >= 7, c < 6, c >= 7
    return 0 if top and right else 1 if top and left else 2 if back and right else 3 if back and left else -1


def soft_limits(cs, ms):
    """float32 soft limits as the reference holds them (jnt_range * factor, rounded once)"""
    jr = np.ctypeslib.as_array(ms.jnt_range).reshape(12, 2).astype(np.float32)
    return jr * F32(cs.soft_joint_pos_limit_factor), jr


def slow_fmod(S):
    """does any foot leave fmod_once's fast range 0 <= phase + phase_dt < 2 * float(2 pi) (float32 sum)?"""
    x = S[abi.S_PHASE:abi.S_PHASE + 4].astype(np.float32) + F32(S[abi.S_PHASE_DT])
    return bool((~((x >= 0) & (x < F32(2) * TWO_PI32))).any())


def swing_mask(S):
    return S[abi.S_PHASE:abi.S_PHASE + 4].astype(np.float32) / TWO_PI32 >= F32(0.5)


FOOT_COMBOS = [(air, con, last) for air in (0.0, 0.3) for con in (0, 1) for last in (0, 1)]


def foot_combo(S, F, f):
    return (float(S[abi.S_AIR_TIME + f]) > 0, bool(F[abi.F_CONTACT + f]), bool(S[abi.S_LAST_CONTACT + f]))


class Case:
    def __init__(self, name, family, branch, base):
        self.name, self.family, self.branch = name, family, branch
        self.S, self.I, self.F, self.Z, self.A = (a.copy() for a in base)
        self.u = 0.5                  # pinned draw of this case's launch; None = the real Philox draws
        self.threshold = None         # reason, if the input sits exactly on a float32 threshold and the fp64 build lands on the other side
        self.index = -1               # position in the batch = local env id

    def __repr__(self):
        return f"<{self.index} {self.family}/{self.name}>"


def _base(cs, ms):
    key = np.ctypeslib.as_array(ms.key_qpos).astype(np.float32)
    S = np.zeros(abi.NSTATE, np.float32); I = np.zeros(abi.NISTATE, np.int32); F = np.zeros(abi.NFRAME, np.float32)
    j = np.arange(12)
    S[0:7] = [0.1, -0.2, 0.30, np.cos(0.15), 0.0, 0.0, np.sin(0.15)]
    S[7:19] = key[7:] + (0.01 * (j + 1) * (-1.0) ** j).astype(np.float32)
    S[abi.S_QVEL:abi.S_QVEL + 18] = np.linspace(-0.4, 0.45, 18)
    S[abi.S_CMD:abi.S_CMD + 3] = [0.3, -0.1, 0.2]
    S[abi.S_PHASE:abi.S_PHASE + 4] = [0.5, 3.6, 3.9, 0.7]          # the two feet in contact are in stance, the two in the air in swing
    S[abi.S_GAIT_FREQ] = 2.0; S[abi.S_PHASE_DT] = TWO_PI32 * F32(cs.ctrl_dt) * F32(2.0)
    S[abi.S_LAST_ACT:abi.S_LAST_ACT + 12] = np.linspace(-0.5, 0.6, 12); S[abi.S_LAST_LAST_ACT:abi.S_LAST_LAST_ACT + 12] = np.linspace(0.4, -0.3, 12)
    S[abi.S_AIR_TIME:abi.S_AIR_TIME + 4] = [0.0, 0.12, 0.2, 0.0]; S[abi.S_SWING_PEAK:abi.S_SWING_PEAK + 4] = [-0.25, -0.2, -0.22, -0.27]
    S[abi.S_HMAX:abi.S_HMAX + 4] = [0.11, 0.12, 0.13, 0.14]; S[abi.S_HMIN:abi.S_HMIN + 4] = [0.01, 0.02, 0.03, 0.04]
    S[abi.S_QERR_HIST:abi.S_QERR_HIST + 24] = 0.001 * np.arange(1, 25); S[abi.S_QVEL_HIST:abi.S_QVEL_HIST + 24] = -0.01 * np.arange(1, 25) - 0.005
    S[abi.S_LAST_CONTACT:abi.S_LAST_CONTACT + 4] = [1, 0, 1, 0]
    I[abi.I_STEP], I[abi.I_STEPS_UNTIL_CMD], I[abi.I_RNG_CTR] = 7, 3, 4
    F[abi.F_GYRO:abi.F_GYRO + 3] = [0.02, -0.03, 0.05]; F[abi.F_ACCEL:abi.F_ACCEL + 3] = [0.1, -0.2, 9.7]
    F[abi.F_GLOBAL_LINVEL:abi.F_GLOBAL_LINVEL + 3] = [0.2, -0.05, 0.03125]; F[abi.F_GLOBAL_ANGVEL:abi.F_GLOBAL_ANGVEL + 3] = [0.04, -0.06, 0.1]
    F[abi.F_LOCAL_LINVEL:abi.F_LOCAL_LINVEL + 3] = [0.21, -0.04, 0.03]; F[abi.F_UPVECTOR:abi.F_UPVECTOR + 3] = [0.02, -0.01, 0.9997]
    F[abi.F_GRAVITY:abi.F_GRAVITY + 3] = [0.02, -0.01, -0.9997]
    F[abi.F_FEET_POS:abi.F_FEET_POS + 12] = [0.19, -0.13, -0.29, 0.20, 0.14, -0.24, -0.21, -0.12, -0.26, -0.22, 0.15, -0.285]
    F[abi.F_FEET_VEL:abi.F_FEET_VEL + 12] = [0.10, 0.03, 0.0, 0.15, 0.01, 0.01, 0.20, -0.01, 0.02, 0.25, -0.03, 0.03]
    F[abi.F_ACT_FORCE:abi.F_ACT_FORCE + 12] = [3, -4.5, 6, -2, 5.5, -7, 1.5, -3.5, 8, -6.5, 2.5, -1]
    F[abi.F_CONTACT:abi.F_CONTACT + 4] = [1, 0, 0, 1]; F[abi.F_FOOT_SITE_Z:abi.F_FOOT_SITE_Z + 4] = [0.021, 0.07, 0.055, 0.023]
    r, c = np.divmod(np.arange(abi.NSCAN), abi.SCAN_W)
    Z = (0.01 + 0.002 * r + 0.0003 * c).astype(np.float32)        # a slope: 117 different heights, the lowest at cell 0, the highest at cell 116
    A = np.linspace(-0.3, 0.5, 12).astype(np.float32)
    return S, I, F, Z, A


def pinned_draws(cs):
    """the draws a resampling step is pinned to, one launch each: both ends of [0, 1), and either side of every threshold of sample_command"""
    us = [F32(0.0)]
    for i in range(3):
        us += [below(cs.cmd_b[i]), F32(cs.cmd_b[i])]
    us += [below(0.5), F32(0.5), F32(1.0) - F32(2.0 ** -24)]
    return sorted(set(float(u) for u in us))


def build_cases(cfg, model):
    cs, ms = abi.config_struct(cfg), abi.model_struct(model)
    base = _base(cs, ms)
    key = np.ctypeslib.as_array(ms.key_qpos).astype(np.float32)
    cases = []

    def new(name, family, branch):
        c = Case(name, family, branch, base)
        cases.append(c)
        return c

    new("standing", "base", "the state every case starts from")

    # ---- termination: done = upvector.z < 0 (joystick_pgtt.py:191), crossed with a timer that runs out or not.  -0.0 is not < 0; a negative
    #      denormal (-1e-40) is, in IEEE arithmetic - a compare that flushed its input to zero would lose it
    for z in (-1e-9, -0.0, 0.0, 1e-9, -1.0, -1e-40, 1e-40):
        for timer in (3, 1):
            c = new(f"upz={z!r},timer={timer}", "termination", "done x timer")
            c.F[abi.F_UPVECTOR + 2] = F32(z); c.I[abi.I_STEPS_UNTIL_CMD] = timer

    # ---- timer and command
    for timer in (2, 1, 0, -1):
        c = new(f"timer={timer}", "timer", "steps_until_next_cmd - 1 <= 0")
        c.I[abi.I_STEPS_UNTIL_CMD] = timer
    for u in pinned_draws(cs):
        c = new(f"resample,u={u!r}", "draws", "sample_command's z / w selects and exp_timer at a pinned draw")
        c.I[abi.I_STEPS_UNTIL_CMD] = 1; c.u = u
        c = new(f"done-only,u={u!r}", "draws", "done with a running timer: the timer is redrawn, the command is not")
        c.I[abi.I_STEPS_UNTIL_CMD] = 3; c.F[abi.F_UPVECTOR + 2] = F32(-0.5); c.u = u
    for ctr in (0, 1, 2 ** 31 - 1):
        c = new(f"philox,resample,ctr={ctr}", "philox", "real draws: epoch counter")
        c.I[abi.I_STEPS_UNTIL_CMD] = 1; c.I[abi.I_RNG_CTR] = ctr; c.u = None
        c = new(f"philox,noise-only,ctr={ctr}", "philox", "real draws: the 147 noise words")
        c.I[abi.I_RNG_CTR] = ctr; c.u = None
    c = new("philox,done-only", "philox", "real draws: timer stream alone")
    c.F[abi.F_UPVECTOR + 2] = F32(-0.25); c.u = None

    # ---- phase clock, fast path: phase + phase_dt one ulp below, at, one ulp above float(2 pi), a different foot each time
    dt32 = F32(base[0][abi.S_PHASE_DT])
    for k, target in enumerate((below(TWO_PI32), TWO_PI32, above(TWO_PI32))):
        ph = F32(target - dt32)
        for cand in (ph, below(ph), above(ph), below(below(ph)), above(above(ph))):
            if F32(cand + dt32) == target:
                ph = cand
                break
        assert F32(ph + dt32) == target
        c = new(f"wrap,sum=2pi{('-1ulp', '', '+1ulp')[k]}", "phase-fast", "fmod_once: x >= y")
        c.S[abi.S_PHASE + k] = ph
    for k, ph in enumerate((below(PI32), PI32, above(PI32))):
        for con, f in ((con, f) for con in (0, 1) for f in range(4)):
            c = new(f"swing,phase=pi{('-1ulp', '', '+1ulp')[k]},contact={con},foot={f}", "phase-fast", "swing mask: phase / 2 pi >= 0.5; get_z's first piece boundary")
            c.S[abi.S_PHASE + f] = ph; c.F[abi.F_CONTACT + f] = con
    # ---- gait pieces: get_z's second boundary T_peak = float(1.5 pi) (the first, T_stance = float(pi), is the swing cases above)
    T_peak = F32(2 * np.pi * 1.5 / 2)
    for k, ph in enumerate((below(T_peak), T_peak, above(T_peak))):
        c = new(f"get_z,phase=1.5pi{('-1ulp', '', '+1ulp')[k]}", "gait", "gait_get_z: phi <= T_peak")
        c.S[abi.S_PHASE + (k + 1) % 4] = ph
    # ---- phase clock, slow path (fmodf): no caller produces these - phase_dt = 2 pi ctrl_dt gait_freq < 0.4 with the shipped gait range, phases in
    #      [0, 2 pi) - the kernel must still do what fmodf does, sign of the dividend included
    for name, dt, phases in (("dt=0", 0.0, None), ("dt=2pi", TWO_PI32, [0.5, 3.6, below(TWO_PI32), 6.2]), ("dt=7.5", 7.5, [5.5, 3.6, 6.0, 0.7]),
                             ("dt=-0.3", -0.3, [0.2, 3.6, 0.3, 5.0]), ("phase<0", None, [0.5, -0.4, 3.9, -7.0])):
        c = new("fmod," + name, "phase-slow", "fmod_once's library call")
        if dt is not None:
            c.S[abi.S_PHASE_DT] = F32(dt)
        if phases is not None:
            c.S[abi.S_PHASE:abi.S_PHASE + 4] = phases

    # ---- command norm: stand_still (< 0.01) / feet_slip, feet_air_time, feet_height (> 0.01) switch; the standing state has joint offsets, slip,
    #      air time and a first contact, so each switch shows in a metric
    for comp in (0, 2):
        for nm, v in (("0", F32(0)), ("0.01-1ulp", below(0.01)), ("0.01", F32(0.01)), ("0.01+1ulp", above(0.01))):
            c = new(f"cmd[{comp}]={nm}", "cmd-norm", "cmd_norm < 0.01, cmd_norm > 0.01")
            c.S[abi.S_CMD:abi.S_CMD + 3] = 0.0; c.S[abi.S_CMD + comp] = v
            n32 = np.sqrt(F32(v * v))                               # the float32 norm of (v, 0, 0): sqrtf(fl(v^2))
            n64 = np.sqrt(float(v) * float(v))
            # (a discrete output shows the switch only if one of the four gated terms has a non-zero scale: the shipped pgtt config has none)
            gated = any(float(cs.reward_scale[abi.REWARD_KEYS.index(k)]) != 0 for k in ("stand_still", "feet_slip", "feet_air_time", "feet_height"))
            if gated and (n32 < F32(0.01), n32 > F32(0.01)) != (n64 < 0.01, n64 > 0.01):
                c.threshold = "cmd_norm == 0.01f: (double)0.01f < 0.01"

    # ---- foot bookkeeping: all eight (air time > 0, contact, last contact) combinations on every foot, four different ones in each case
    for r in range(8):
        c = new(f"feet,rot={r}", "feet", "first_contact / air time / last contact table")
        for f in range(4):
            air, con, last = FOOT_COMBOS[(r + 2 * f) % 8]
            c.S[abi.S_AIR_TIME + f] = F32(air) + F32(0.01 * f) * F32(air > 0); c.F[abi.F_CONTACT + f] = con; c.S[abi.S_LAST_CONTACT + f] = last
    for r in range(2):
        c = new(f"swing_peak,{('below', 'above')[r]}-on-feet-0-2", "feet", "swing_peak = max(swing_peak, foot z)")
        for f in range(4):
            up = (f % 2 == 0) == (r == 1)
            c.S[abi.S_SWING_PEAK + f] = c.F[abi.F_FEET_POS + 3 * f + 2] + F32(0.05 + 0.01 * f) * F32(1 if up else -1)
            c.F[abi.F_CONTACT + f] = 0                   # in the air: the peak survives the step

    # ---- joints: each one below / at / at / above its soft limits, the other eleven inside
    soft, jr = soft_limits(cs, ms)
    fac64 = float(F32(cs.soft_joint_pos_limit_factor))
    for jn in range(12):
        for side, where in ((0, "below"), (0, "at"), (1, "at"), (1, "above")):
            c = new(f"joint{jn},{where}-{('lower', 'upper')[side]}", "joint-limits", "dof_pos_limits: clip(q - lo, max 0), clip(q - hi, min 0)")
            lim = soft[jn, side]
            c.S[7 + jn] = lim if where == "at" else F32(lim + F32(0.1) * F32(1 if side else -1))
            if where == "at":
                # the fp64 build forms the limit as (double)range * (double)factor: the float32 limit is beyond it or not, by its rounding
                lim64 = float(jr[jn, side]) * fac64
                if (float(lim) < lim64) if side == 0 else (float(lim) > lim64):
                    c.threshold = "q == float32 soft limit, which lies beyond the unrounded product"
    c = new("forces,large", "joints", "torques / energy sums at large mixed-sign forces")
    c.F[abi.F_ACT_FORCE:abi.F_ACT_FORCE + 12] = [(150.0 + 10.0 * i) * (-1.0) ** (i // 2) for i in range(12)]
    for jn in range(12):
        c = new(f"action_rate,joint{jn}", "joints", "action - last_act on one joint")
        c.A[:] = c.S[abi.S_LAST_ACT:abi.S_LAST_ACT + 12]; c.A[jn] += F32(0.25)

    # ---- scan quadrants: each of the 117 cells as the only maximum, then the only minimum, of the whole scan
    #      on the sloped background.  All four feet are in swing here, so that feet_phase (get_z's target height) reads H_max of every quadrant
    #      (and in the air: a foot that is in swing AND in contact costs 2.0 under the shipped scales, which would park every reward at the lower clip)
    zb, swing_phases = base[3], [3.5, 3.6, 3.9, 4.4]

    def airborne_swing(c):
        c.S[abi.S_PHASE:abi.S_PHASE + 4] = swing_phases; c.F[abi.F_CONTACT:abi.F_CONTACT + 4] = 0
        return c

    airborne_swing(new("scan,background", "scan-background", "the slope alone"))
    for k in range(abi.NSCAN):
        c = new(f"scan,max@{k}", "scan-max", f"obs_quad_cell: quadrant {quadrant_of(k)}")
        c.Z[k] = zb.max() + F32(0.05); airborne_swing(c)
        c = new(f"scan,min@{k}", "scan-min", f"obs_quad_cell: quadrant {quadrant_of(k)}")
        c.Z[k] = zb.min() - F32(0.05); airborne_swing(c)

    # ---- history: shifted when step % history_update_steps == 0 (the step counter BEFORE it advances), left alone otherwise
    h = int(cs.history_update_steps)
    for step in (0, 1, h - 1, h, 2 * h, 2 ** 31 - 2):
        c = new(f"history,step={step}", "history", "step % history_update_steps == 0")
        c.I[abi.I_STEP] = step

    # ---- reward clips
    c = new("clip,low", "clips", "reward = clip(sum * dt, 0, 10000): negative sum")
    c.S[7:19] = key[7:] + np.where(np.arange(12) % 2 == 0, 1.0, -1.0).astype(np.float32) * F32(1.0)
    c.S[abi.S_CMD:abi.S_CMD + 3] = [0.6, 0.6, 1.0]; c.F[abi.F_LOCAL_LINVEL:abi.F_LOCAL_LINVEL + 2] = [-1.0, -1.0]; c.F[abi.F_GYRO + 2] = -2.0
    c.F[abi.F_GLOBAL_LINVEL + 2] = 0.0; c.F[abi.F_UPVECTOR:abi.F_UPVECTOR + 3] = [0.6, 0.5, 0.62]; c.F[abi.F_GLOBAL_ANGVEL:abi.F_GLOBAL_ANGVEL + 2] = [3.0, -2.0]
    c = new("clip,vz=4", "clips", "reward = clip(sum * dt, 0, 10000): lin_vel_z^2 = 16 (the upper clip under the all-scales config)")
    c.F[abi.F_GLOBAL_LINVEL + 2] = 4.0

    if len(cases) % 64 == 0:              # the batch is deliberately no multiple of the wave / of task_kernel's block
        new("standing,again", "base", "padding")
    for i, c in enumerate(cases):
        c.index = i
        c.S[abi.S_MOTOR_TARGETS:abi.S_MOTOR_TARGETS + 12] = key[7:] + c.A * F32(cs.action_scale)     # what this step's physics launch left in the row
    return cases


def pack_cases(cases):
    """the cases as the SoA buffers of one batch"""
    S = np.stack([c.S for c in cases], 1); I = np.stack([c.I for c in cases], 1); F = np.stack([c.F for c in cases], 1)
    Z = np.stack([c.Z for c in cases], 0); A = np.stack([c.A for c in cases], 0)
    return S, I, F, Z, A


def discrete(inp_S, out):
    """the discrete outputs of a step (`out`: TaskOracle.run's dict, or the same keys read off the device)"""
    st, it = out["state"], out["istate"]
    return dict(done=bool(out["done"]), timer=int(it[abi.I_STEPS_UNTIL_CMD]), step=int(it[abi.I_STEP]), rng_ctr=int(np.uint32(it[abi.I_RNG_CTR])),
                last_contact=tuple(bool(v) for v in st[abi.S_LAST_CONTACT:abi.S_LAST_CONTACT + 4]),
                cmd_changed=not np.array_equal(st[abi.S_CMD:abi.S_CMD + 3], inp_S[abi.S_CMD:abi.S_CMD + 3]),
                zero_terms=tuple(bool(v == 0) for v in out["metrics"][:abi.NREW]))
