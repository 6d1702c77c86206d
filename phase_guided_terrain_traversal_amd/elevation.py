"""Depth-fused elevation map: a geometric height scan per env (libpgtt_elevation.so, include/pgtt_elevation.h).  The onboard depth image is
unprojected with the camera pose, fused into a rolling robot-centred map of world heights, and the observation's 117 scan rows are sampled from
the map: what a deployed robot's elevation-mapping stack provides, with nothing to train.  With source="lidar" the map is fused from the world
points of the env's LiDAR (lidar.py) instead: the sensor such a stack reads on the robot, which sees all round it.

    em = ElevationMap(env, grid=64, res=0.04, alpha=1.0)     # env: a Joystick with a torso depth camera of period 1
    em.tick(clear_all=True)                                  # one launch on the env's current stream, no synchronisation
    em.map, em.origin, em.est, em.known, em.obs              # [N, G, G] heights (NaN = unknown), [N, 2], [N, 117], [N, 117] uint8, [N, obs_dim]

    em = ElevationMap(env, fill=16)                          # hole filling behind every tick: a second launch with outputs of its own
    em.filled_est, em.filled_dist, em.filled_obs             # [N, 117], [N, 117] uint8 (0 measured, 1..16 the pass that filled it, 255 unknown), [N, obs_dim]

    em = ElevationMap(env, follow_sensor=True)               # env's sensor may have any period: tick() behind the sensor's tick fuses when the
    em.tick(use_done=True, force=False)                      # sensor has new data and otherwise samples the held map at the current pose

    em = ElevationMap(env, variance=True)                    # variance-weighted (Kalman) fusion in place of the maximum and alpha: a measurement
    em.var, em.est_var                                       # noise per cell from its distance, [N, G, G] variances (m^2) and [N, 117] at the scan

    em = ElevationMap(env, odometry=True)                    # the map is registered with a dead-reckoned pose that drifts in x, y, z and yaw
    em.pose_est, em.odo                                      # (ODOMETRY_DEFAULTS), not with the simulator's: [7, N] and [N, 12] (e_xyz, psi, ...)

    em = ElevationMap(env, visibility=True)                  # visibility clean-up in front of every tick: a ray that passed below a cell's height
    em.cleared                                               # on its way to the ground forgets the cell (VISIBILITY_DEFAULTS); [N] int32 per call

    em = ElevationMap(env, latency=2)                        # sensor latency: every frame is fused 2 ticks after it was taken, under the pose of
    em.latency, em.fused                                     # its capture; latency=(0, 4) draws it per env per episode; [N] int32, [N] uint8

`Joystick(..., depth=dict(...), elevation=dict(...) | True)` owns one and ticks it behind the camera (env.elevation_obs);
`Joystick(..., lidar=dict(...), elevation=dict(source="lidar"))` one that is ticked behind the LiDAR.  The module is not imported by env.py unless
an elevation map is asked for.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _sidelib, abi

# include/pgtt_elevation.h
MAX_DIM, MIN_GRID, MAX_GRID = 256, 8, 96
NSCAN = abi.NSCAN
SCAN_ROW0 = {"pgtt": 38, "baseline": 30}           # perceive.SCAN_ROW0: the scan rows sit between phase / joint_vel and gait_freq / last_act
# Joystick(elevation=True) / evaluate.py --elevation: a 2.56 m window of 4 cm cells, the newest view replaces the old one, and a box around the
# torso that drops the robot's own legs from a camera that sees them - settings, not measured facts about a robot
DEFAULTS = dict(grid=64, res=0.04, alpha=1.0, self_half=(0.45, 0.25, 0.45))
# fill=True: the self box's 0.45 m is 12 cells of 4 cm, and 16 passes reach 0.64 m - a setting too; fill=0, the default, fills nothing
FILL_PASSES = 16
MAX_FILL = MAX_GRID - 1
DIST_UNKNOWN = 255                                 # filled_dist of a scan point (filled_dist_map of a cell) that no pass reached
SOURCES = ("depth", "lidar")                       # ElevationMap(source=...): what the map is fused from; "depth" unless said otherwise
# the camera fields of a map that is fused from points: never read by pgtt_elevation_points, but pgtt_elevation_create checks them
PLACEHOLDER_CAMERA = dict(width=1, height=1, fovy=90.0, near=0.1, far=1.0)
# variance=True: 5 mm of range-independent noise and 1 % of the distance, a map that forgets slowly (1e-6 m^2 per tick), a 3-sigma gate, the top 3 cm
# of a cell's pixels taken as one surface, at most 4 of them counted as independent, and a prior of 1 m^2 - settings, not measured facts about a sensor
VARIANCE_DEFAULTS = dict(sigma0=0.005, sigma_rel=0.01, process=1e-6, gate=3.0, band=0.03, max_count=4, var_max=1.0)
MAX_BAND, VAR_MAX_GRID = 0.5, 64                   # PGTT_ELEVATION_MAX_BAND, PGTT_ELEVATION_VAR_MAX_GRID
# odometry=True: 2 cm of horizontal and 1 cm of vertical random walk per sqrt(metre walked), 0.01 rad / sqrt(s) of yaw random walk, a gyro bias of up
# to 0.005 rad / s and an odometry scale error of up to 2 %, both drawn once per episode - settings, not measured facts about a robot
ODOMETRY_DEFAULTS = dict(sigma_xy=0.02, sigma_z=0.01, sigma_yaw=0.01, yaw_bias=0.005, scale=0.02, seed=0)
RS_ODOMETRY, ODO_WORDS = 34, 12                    # PGTT_RS_ODOMETRY, PGTT_ELEVATION_ODO_WORDS
# visibility=True: a cell is forgotten when it stands more than 5 cm above a ray, no sample within one and a half cells (of DEFAULTS' 4 cm) of the
# ray's end - the cell that was hit and its neighbour are the tick's business -, every second row and column of the image (every second point)
# casts a ray, and with a variance layer the height is taken as it stands (sigmas = 0) - settings, not facts; end_guard=None is 1.5 res
VISIBILITY_DEFAULTS = dict(margin=0.05, end_guard=None, stride=2, sigmas=0.0)
# latency=K or (lo, hi): the ticks between a frame's capture and its fusion, fixed or drawn per env per episode in [lo, hi] - a setting; the default
# of the dict form is no latency at all
LATENCY_DEFAULTS = dict(ticks=(0, 0), seed=0)
RS_LATENCY, MAX_LATENCY = 35, 8                    # PGTT_RS_LATENCY, PGTT_ELEVATION_MAX_LATENCY

f, i32 = C.c_float, C.c_int32


class PgttElevationConfig(C.Structure):
    _fields_ = [("width", i32), ("height", i32), ("fovy_deg", f), ("near", f), ("far", f), ("mount_body", i32), ("mount_pos", f * 3),
                ("mount_quat", f * 4), ("grid", i32), ("res", f), ("alpha", f), ("self_half", f * 3), ("scan_dist_x", f), ("scan_dist_y", f),
                ("obs_dim", i32), ("scan_row0", i32)]


class PgttElevationBuffers(C.Structure):
    _fields_ = [("state", C.c_void_p), ("depth", C.c_void_p), ("obs", C.c_void_p), ("done", C.c_void_p), ("map", C.c_void_p),
                ("origin", C.c_void_p), ("est", C.c_void_p), ("known", C.c_void_p), ("obs_out", C.c_void_p)]


class PgttElevationFill(C.Structure):
    _fields_ = [("est", C.c_void_p), ("dist", C.c_void_p), ("obs_out", C.c_void_p), ("map_out", C.c_void_p), ("dist_out", C.c_void_p)]


class PgttElevationVar(C.Structure):
    _fields_ = [("var", C.c_void_p), ("est_var", C.c_void_p), ("sigma0", f), ("sigma_rel", f), ("process", f), ("gate", f), ("band", f),
                ("max_count", i32), ("var_max", f)]


assert C.sizeof(PgttElevationConfig) == 92 and C.sizeof(PgttElevationBuffers) == 72 and C.sizeof(PgttElevationFill) == 40
class PgttElevationOdometry(C.Structure):
    _fields_ = [("state", C.c_void_p), ("done", C.c_void_p), ("points", C.c_void_p), ("points_est", C.c_void_p), ("P", i32),
                ("pose_est", C.c_void_p), ("odo", C.c_void_p), ("counter", C.c_void_p), ("seed", C.c_uint64), ("env_id_offset", C.c_int64),
                ("dt", f), ("sigma_xy", f), ("sigma_z", f), ("sigma_yaw", f), ("yaw_bias", f), ("scale", f)]


class PgttElevationVisibility(C.Structure):
    _fields_ = [("margin", f), ("end_guard", f), ("stride", i32), ("sigmas", f), ("sensor_pos", f * 3), ("cleared", C.c_void_p),
                ("bound_out", C.c_void_p)]


class PgttElevationLatency(C.Structure):
    _fields_ = [("ring_data", C.c_void_p), ("ring_pose", C.c_void_p), ("lat", C.c_void_p), ("age", C.c_void_p), ("fused", C.c_void_p),
                ("counter", C.c_void_p), ("D", i32), ("lat_lo", i32), ("lat_hi", i32), ("seed", C.c_uint64), ("env_id_offset", C.c_int64)]


assert C.sizeof(PgttElevationVar) == 48 and C.sizeof(PgttElevationOdometry) == 104 and C.sizeof(PgttElevationVisibility) == 48
assert C.sizeof(PgttElevationLatency) == 80


class ElevationError(RuntimeError):
    pass


vp, cp = C.c_void_p, C.POINTER(PgttElevationConfig)
SIDE = _sidelib.SideLib("elevation", ElevationError, {
    "pgtt_elevation_check": (None, [cp]), "pgtt_elevation_create": (None, [cp, C.c_int, C.c_int, C.POINTER(vp)]),
    "pgtt_elevation_destroy": (None, [vp]), "pgtt_elevation_bind": (None, [vp, C.POINTER(PgttElevationBuffers)]),
    "pgtt_elevation": (None, [vp, vp, C.c_int, C.c_int, vp]),
    "pgtt_elevation_bind_points": (None, [vp, C.POINTER(PgttElevationBuffers), vp, C.c_int]),
    "pgtt_elevation_points": (None, [vp, vp, C.c_int, C.c_int, vp]),
    "pgtt_elevation_bind_fill": (None, [vp, C.POINTER(PgttElevationFill), C.c_int]), "pgtt_elevation_fill": (None, [vp, vp]),
    "pgtt_elevation_bind_rate": (None, [vp, vp, C.c_int]), "pgtt_elevation_follow": (None, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "pgtt_elevation_check_var": (None, [C.POINTER(PgttElevationVar)]), "pgtt_elevation_bind_var": (None, [vp, C.POINTER(PgttElevationVar)]),
    "pgtt_elevation_var": (None, [vp, vp, C.c_int, C.c_int, vp]), "pgtt_elevation_var_points": (None, [vp, vp, C.c_int, C.c_int, vp]),
    "pgtt_elevation_check_odometry": (None, [C.POINTER(PgttElevationOdometry)]),
    "pgtt_elevation_bind_odometry": (None, [vp, C.POINTER(PgttElevationOdometry)]), "pgtt_elevation_odometry": (None, [vp, vp, C.c_int, C.c_int, vp]),
    "pgtt_elevation_check_visibility": (None, [C.POINTER(PgttElevationVisibility)]),
    "pgtt_elevation_bind_visibility": (None, [vp, C.POINTER(PgttElevationVisibility)]),
    "pgtt_elevation_visibility": (None, [vp, vp, C.c_int, C.c_int, vp]),
    "pgtt_elevation_check_latency": (None, [C.POINTER(PgttElevationLatency)]),
    "pgtt_elevation_bind_latency": (None, [vp, C.POINTER(PgttElevationLatency)]),
    "pgtt_elevation_delayed": (None, [vp, vp, C.c_int, C.c_int, vp]),
}, {"pgtt_elevation_sizeof_config": PgttElevationConfig, "pgtt_elevation_sizeof_buffers": PgttElevationBuffers,
    "pgtt_elevation_sizeof_fill": PgttElevationFill, "pgtt_elevation_sizeof_var": PgttElevationVar,
    "pgtt_elevation_sizeof_odometry": PgttElevationOdometry, "pgtt_elevation_sizeof_visibility": PgttElevationVisibility,
    "pgtt_elevation_sizeof_latency": PgttElevationLatency})
LIB_PATH, EXPORTS, lib, check, build_info = SIDE.path, SIDE.exports, SIDE.lib, SIDE.check, SIDE.build_info


def settings(overrides=None) -> Dict:
    """ElevationMap's keyword arguments: DEFAULTS with `overrides` on top (True or None = the defaults)"""
    return {**DEFAULTS, **({} if overrides is None or overrides is True else dict(overrides))}


def variance_settings(variance=None) -> Optional[Dict]:
    """ElevationMap's `variance` argument as a full dict: None / False -> None (no variance layer), True -> VARIANCE_DEFAULTS, a dict -> the
    defaults with it on top.  ValueError for a key that is no setting."""
    if variance is None or variance is False:
        return None
    over = {} if variance is True else dict(variance)
    unknown = sorted(set(over) - set(VARIANCE_DEFAULTS))
    if unknown:
        raise ValueError(f"ElevationMap(variance=...): unknown setting(s) {unknown}; the settings are {sorted(VARIANCE_DEFAULTS)}")
    return {**VARIANCE_DEFAULTS, **over}


def variance_struct(sigma0=0.005, sigma_rel=0.01, process=1e-6, gate=3.0, band=0.03, max_count=4, var_max=1.0, var=None, est_var=None) -> PgttElevationVar:
    """no checks: the library makes its own (pgtt_elevation_check_var)"""
    v = PgttElevationVar()
    v.var, v.est_var = var, est_var
    v.sigma0, v.sigma_rel, v.process, v.gate, v.band, v.max_count, v.var_max = (float(sigma0), float(sigma_rel), float(process), float(gate),
                                                                                 float(band), int(max_count), float(var_max))
    return v


def odometry_settings(odometry=None) -> Optional[Dict]:
    """ElevationMap's `odometry` argument as a full dict: None / False -> None (the map is registered with the true pose), True ->
    ODOMETRY_DEFAULTS, a dict -> the defaults with it on top.  ValueError for a key that is no setting or for anything else."""
    if odometry is None or odometry is False:
        return None
    if odometry is not True and not isinstance(odometry, dict):
        raise ValueError(f"ElevationMap(odometry=...): odometry must be True or a dict of settings, not {odometry!r}")
    over = {} if odometry is True else dict(odometry)
    unknown = sorted(set(over) - set(ODOMETRY_DEFAULTS))
    if unknown:
        raise ValueError(f"ElevationMap(odometry=...): unknown setting(s) {unknown}; the settings are {sorted(ODOMETRY_DEFAULTS)}")
    return {**ODOMETRY_DEFAULTS, **over}


def odometry_struct(dt, sigma_xy=0.02, sigma_z=0.01, sigma_yaw=0.01, yaw_bias=0.005, scale=0.02, seed=0, env_id_offset=0, state=None, done=None,
                    points=None, points_est=None, P=0, pose_est=None, odo=None, counter=None) -> PgttElevationOdometry:
    """no checks: the library makes its own (pgtt_elevation_check_odometry)"""
    o = PgttElevationOdometry()
    o.state, o.done, o.points, o.points_est, o.P = state, done, points, points_est, int(P)
    o.pose_est, o.odo, o.counter = pose_est, odo, counter
    o.seed, o.env_id_offset = int(seed) & (2 ** 64 - 1), int(env_id_offset)
    o.dt, o.sigma_xy, o.sigma_z, o.sigma_yaw, o.yaw_bias, o.scale = (float(dt), float(sigma_xy), float(sigma_z), float(sigma_yaw), float(yaw_bias),
                                                                    float(scale))
    return o


def visibility_settings(visibility=None, res=DEFAULTS["res"]) -> Optional[Dict]:
    """ElevationMap's `visibility` argument as a full dict: None / False -> None (no clean-up), True -> VISIBILITY_DEFAULTS, a dict -> the defaults
    with it on top; an end_guard of None becomes 1.5 res.  ValueError for a key that is no setting or for anything else."""
    if visibility is None or visibility is False:
        return None
    if visibility is not True and not isinstance(visibility, dict):
        raise ValueError(f"ElevationMap(visibility=...): visibility must be True or a dict of settings, not {visibility!r}")
    over = {} if visibility is True else dict(visibility)
    unknown = sorted(set(over) - set(VISIBILITY_DEFAULTS))
    if unknown:
        raise ValueError(f"ElevationMap(visibility=...): unknown setting(s) {unknown}; the settings are {sorted(VISIBILITY_DEFAULTS)}")
    out = {**VISIBILITY_DEFAULTS, **over}
    if out["end_guard"] is None:
        out["end_guard"] = 1.5 * float(res)
    return out


def visibility_struct(margin=0.05, end_guard=0.06, stride=2, sigmas=0.0, sensor_pos=(0.0, 0.0, 0.0), cleared=None, bound_out=None) -> PgttElevationVisibility:
    """no checks: the library makes its own (pgtt_elevation_check_visibility)"""
    v = PgttElevationVisibility()
    v.margin, v.end_guard, v.stride, v.sigmas = float(margin), float(end_guard), int(stride), float(sigmas)
    v.sensor_pos[:] = [float(x) for x in sensor_pos]
    v.cleared, v.bound_out = cleared, bound_out
    return v


def latency_settings(latency=None) -> Optional[Dict]:
    """ElevationMap's `latency` argument as a full dict: None / False -> None (every frame is fused in the tick it was taken), an int K ->
    dict(ticks=(K, K), seed=0), a pair (lo, hi) -> that range, drawn per env per episode, a dict -> LATENCY_DEFAULTS with it on top (its `ticks` an
    int or a pair).  ValueError for a key that is no setting or for anything else; the ranges are the library's to check."""
    if latency is None or latency is False:
        return None

    def pair(t):
        if isinstance(t, int) and not isinstance(t, bool):
            return (t, t)
        if isinstance(t, (tuple, list)) and len(t) == 2 and all(isinstance(x, int) and not isinstance(x, bool) for x in t):
            return (int(t[0]), int(t[1]))
        raise ValueError(f"ElevationMap(latency=...): the ticks must be an int or a pair (lo, hi) of ints, not {t!r}")
    if isinstance(latency, dict):
        unknown = sorted(set(latency) - set(LATENCY_DEFAULTS))
        if unknown:
            raise ValueError(f"ElevationMap(latency=...): unknown setting(s) {unknown}; the settings are {sorted(LATENCY_DEFAULTS)}")
        out = {**LATENCY_DEFAULTS, **latency}
        if isinstance(out["seed"], bool) or not isinstance(out["seed"], int):
            raise ValueError(f"ElevationMap(latency=...): seed must be an int, not {out['seed']!r}")
        return dict(ticks=pair(out["ticks"]), seed=out["seed"])
    if isinstance(latency, bool):
        raise ValueError("ElevationMap(latency=...): latency must be an int, a pair (lo, hi) or a dict of settings, not True")
    return dict(ticks=pair(latency), seed=0)


def latency_struct(ticks=(0, 0), seed=0, env_id_offset=0, D=None, ring_data=None, ring_pose=None, lat=None, age=None, fused=None,
                   counter=None) -> PgttElevationLatency:
    """no checks: the library makes its own (pgtt_elevation_check_latency).  D=None: hi + 1 slots"""
    l = PgttElevationLatency()
    l.ring_data, l.ring_pose, l.lat, l.age, l.fused, l.counter = ring_data, ring_pose, lat, age, fused, counter
    l.lat_lo, l.lat_hi = int(ticks[0]), int(ticks[1])
    l.D = int(ticks[1]) + 1 if D is None else int(D)
    l.seed, l.env_id_offset = int(seed) & (2 ** 64 - 1), int(env_id_offset)
    return l


def config_struct(width, height, fovy, near, far, mount_pos=(0.0, 0.0, 0.0), mount_quat=(1.0, 0.0, 0.0, 0.0), mount_body=0, grid=64, res=0.04,
                  alpha=1.0, self_half=(0.0, 0.0, 0.0), scan_dist_x=0.1, scan_dist_y=0.1, obs_dim=abi.OBS, scan_row0=38) -> PgttElevationConfig:
    """no checks: the library makes its own"""
    c = PgttElevationConfig()
    c.width, c.height, c.fovy_deg, c.near, c.far, c.mount_body = int(width), int(height), float(fovy), float(near), float(far), int(mount_body)
    c.mount_pos[:] = [float(x) for x in mount_pos]
    c.mount_quat[:] = [float(x) for x in mount_quat]
    c.grid, c.res, c.alpha = int(grid), float(res), float(alpha)
    c.self_half[:] = [float(x) for x in self_half]
    c.scan_dist_x, c.scan_dist_y, c.obs_dim, c.scan_row0 = float(scan_dist_x), float(scan_dist_y), int(obs_dim), int(scan_row0)
    return c


class ElevationMap(_sidelib.Handle):
    """The elevation map of one Joystick with a depth camera or a LiDAR: owns the handle and the tensors `map` [N, G, G] (world heights, NaN =
    unknown; world cell (ix, iy) at map[ix mod G, iy mod G]), `origin` [N, 2] int32 (the base's cell), `est` [N, 117], `known` [N, 117] uint8 and
    `obs` [N, obs_dim] (the obs_out buffer: the env's observation with the scan rows replaced by est).  source="depth": the camera's intrinsics
    and mount are those of env.depth_camera; source="lidar": the map is fused from env.lidar_scanner.points, world points that need no camera (the
    config's camera fields hold placeholders).  grid / res: the window is grid x grid cells of res metres; alpha: fusion gain in (0, 1], 1 = the
    newest view replaces the old; self_half: half extents of a box in the base frame whose points are dropped (the robot's own body in a sensor
    that sees it), zeros = none.  The defaults are settings, not facts.
    fill = K > 0 (True = FILL_PASSES): after every tick a second launch closes the map's holes on a copy - K Jacobi passes, an unknown cell takes the
    minimum of its known neighbours inside the window - and samples the scan from it: `filled_est` [N, 117], `filled_dist` [N, 117] uint8 (0 = a
    measured cell, p = filled in pass p, 255 = still unknown) and `filled_obs` [N, obs_dim]; with dense=True also `filled_map` [N, G, G] (the layout
    of `map`) and `filled_dist_map` [N, G, G] uint8.  The map and the other outputs never see a filled height.  fill = 0: none of this exists.
    follow_sensor=True: the sensor may have any period (every=K).  tick() is then pgtt_elevation_follow: called behind the sensor's tick with the
    same `force`, it decides on the device, from the sensor's counter, whether the sensor has just taken new data - then it is the tick it always
    was - or not: then the map and the origin are left alone (but for the clears) and the scan is sampled from the held map at the current pose.
    follow_sensor=False, the default: a sensor of period 1 is required and tick() enqueues what it always did.
    variance = True (VARIANCE_DEFAULTS) or a dict over them: tick() is the variance tick (pgtt_elevation_var / pgtt_elevation_var_points) in place of
    the plain one - a Kalman update per cell with the measurement noise sigma0^2 + sigma_rel^2 distance^2, the mean of the top `band` metres of a
    cell's pixels as the measurement, a Mahalanobis gate and `process` noise per tick; alpha is not read.  `var` [N, G, G] is the variance layer (m^2,
    NaN where `map` is) and `est_var` [N, 117] the variance at the scan points (var_max at an unknown one).  It needs grid <= 64 and is not built for
    follow_sensor yet.  variance=None, the default: nothing of this is allocated or called.
    odometry = True (ODOMETRY_DEFAULTS) or a dict over them: the map is registered with a dead-reckoned pose, not with the simulator's.  tick()
    first enqueues pgtt_elevation_odometry with the same clear arguments - the pose estimate `pose_est` [7, N] walks away from the env's true pose in
    x, y, z and yaw (`odo` [N, 12]: the position error, the yaw error psi, ...; include/pgtt_elevation.h), and for source="lidar" the LiDAR's world
    points are re-registered at it (`points_est` [N, P, 3]) - and the map is bound to those in place of the env's state and the LiDAR's points.  dt is
    the env's control step, the draws are keyed by `seed` and env.env_id_offset.  Works with fill, variance and follow_sensor; nothing is corrected
    (no loop closure).  The defaults are settings, not facts about a robot.  odometry=None, the default: nothing of this is allocated or called.
    visibility = True (VISIBILITY_DEFAULTS) or a dict over them: tick() enqueues pgtt_elevation_visibility behind the odometry call and in front of
    the tick, with the same clear arguments - every stride-th ray of the image (or point of the LiDAR, from its mount on the torso) lowers a bound
    over the cells it passes, and a cell that stands more than `margin` above its bound is forgotten (NaN, in `var` too).  `cleared` [N] int32 is the
    number of cells the last call forgot; with dense_bound=True `bound` [N, G, G] is the bound layer (NaN = no ray passed).  Not with follow_sensor: a
    hold step must not clean with a stale image.  visibility=None, the default: nothing of this is allocated or called.
    latency = K, (lo, hi) or a dict over LATENCY_DEFAULTS: tick() is pgtt_elevation_delayed in place of the plain tick - every call pushes the image
    (or the points) and the pose rows into a ring on the device, and each env fuses the frame of `latency[e]` calls ago under the pose of its
    CAPTURE, while the window and the scan follow the current pose.  `latency` [N] int32 is the env's latency of this episode, K or drawn in
    [lo, hi] when the env's map is cleared (keyed by `seed` and env.env_id_offset); `fused` [N] uint8 is 0 while the frame that is due predates the
    episode - the first latency[e] calls after a clear fuse nothing.  Latency 0 is the plain tick bit for bit.  Odometry goes in front as ever (the
    ring then stores the pose estimate and the re-registered points) and the fill behind.  The ring costs D N H W 4 bytes with D = hi + 1 (3 P in
    place of H W for the LiDAR): 252 MB at 4096 envs, 64 x 48 and hi = 4.  Not built with variance, visibility or follow_sensor.  latency=None,
    the default: nothing of this is allocated, bound or called.
    Runs on the env's device and current stream; reads env.depth or the LiDAR's points, env.buffers["state" | "obs_state" | "done"] and writes nothing
    but its own tensors."""
    _prefix, _check = "pgtt_elevation", staticmethod(check)

    def __init__(self, env, grid: int = 64, res: float = 0.04, alpha: float = 1.0, self_half: Sequence[float] = (0.45, 0.25, 0.45),
                 source: str = "depth", fill: int = 0, dense: bool = False, follow_sensor: bool = False, variance=None, odometry=None,
                 visibility=None, dense_bound: bool = False, latency=None):
        self.latency_cfg = latency_settings(latency)
        if self.latency_cfg is not None:
            for name, on in (("variance", variance), ("visibility", visibility), ("follow_sensor", follow_sensor)):
                if on is not None and on is not False:
                    raise ValueError(f"ElevationMap: latency with {name} is not built (the stamped tick is the plain tick's alone)")
        self.variance = variance_settings(variance)
        self.odometry = odometry_settings(odometry)
        self.visibility = visibility_settings(visibility, res)
        if self.visibility is not None and follow_sensor:
            raise ValueError("ElevationMap: visibility with follow_sensor=True is not built (a hold step must not clean with a stale image)")
        if dense_bound and self.visibility is None:
            raise ValueError("ElevationMap: dense_bound=True asks for the clean-up's bound layer, so it needs visibility")
        self._sensor_pos = (0.0, 0.0, 0.0)
        if self.variance is not None:
            if follow_sensor:
                raise ValueError("ElevationMap: variance with follow_sensor=True is not built yet (the hold call would have to leave var alone)")
            if int(grid) > VAR_MAX_GRID:
                raise ValueError(f"ElevationMap: the variance tick supports grid <= {VAR_MAX_GRID}, not {grid}")
        self.passes = FILL_PASSES if fill is True else int(fill or 0)
        if self.passes < 0 or self.passes > MAX_FILL:
            raise ValueError(f"ElevationMap: fill must be 0 (none), True or a number of passes in [1, {MAX_FILL}], not {fill!r}")
        if dense and not self.passes:
            raise ValueError("ElevationMap: dense=True asks for the filled map, so it needs fill > 0")
        if source not in SOURCES:
            raise ValueError(f"ElevationMap: source must be one of {SOURCES}, not {source!r}")
        self.source, self.follow_sensor = source, bool(follow_sensor)
        if source == "lidar":
            lid = getattr(env, "lidar_scanner", None)
            if lid is None or lid.points is None:
                raise ValueError("ElevationMap(source='lidar') needs an env with a LiDAR that writes points: Joystick(..., lidar=dict(...))")
            if lid.config.every != 1 and not self.follow_sensor:
                raise ValueError(f"ElevationMap needs a LiDAR of period 1 (every={lid.config.every}): the map would fuse a stale scan again at every tick")
            if self.visibility is not None:
                if lid.config.mount_body != 0:
                    raise ValueError(f"ElevationMap(visibility=...) supports a LiDAR on the torso only (mount_body == 0), not on body "
                                     f"{lid.config.mount_body}: the rays start at the mount, which the map knows in the base frame alone")
                self._sensor_pos = tuple(lid.config.mount_pos)
            od = env.observation_size["state"]
            self.config = config_struct(**PLACEHOLDER_CAMERA, grid=grid, res=res, alpha=alpha, self_half=self_half,
                                        scan_dist_x=env.config["scan_dist_x"], scan_dist_y=env.config["scan_dist_y"], obs_dim=od,
                                        scan_row0=SCAN_ROW0[env.method])
        else:
            cam = getattr(env, "depth_camera", None)
            if cam is None:
                raise ValueError("ElevationMap needs an env with a depth camera: Joystick(..., depth=dict(...))")
            cc = cam.config
            if cc.mount_body != 0:
                raise ValueError(f"ElevationMap supports a camera on the torso only (mount_body == 0), not on body {cc.mount_body}")
            if cc.every != 1 and not self.follow_sensor:
                raise ValueError(f"ElevationMap needs a camera of period 1 (every={cc.every}): a stale image under a moved pose would be unprojected wrongly")
            od = env.observation_size["state"]
            self.config = config_struct(cc.width, cc.height, cc.fovy_deg, cc.near, cc.far, list(cc.mount_pos), list(cc.mount_quat), cc.mount_body, grid, res,
                                        alpha, self_half, env.config["scan_dist_x"], env.config["scan_dist_y"], od, SCAN_ROW0[env.method])
        self.env, self.grid, self.res, self.alpha = env, int(grid), float(res), float(alpha)
        self._lib = lib()
        self._h = C.c_void_p()
        check(self._lib.pgtt_elevation_create(C.byref(self.config), env.device.index or 0, env.num_envs, C.byref(self._h)))
        dev, n = env.device, env.num_envs
        self.map = torch.full((n, self.grid, self.grid), float("nan"), dtype=torch.float32, device=dev)
        self.origin = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        self.est = torch.zeros((n, NSCAN), dtype=torch.float32, device=dev)
        self.known = torch.zeros((n, NSCAN), dtype=torch.uint8, device=dev)
        self.obs = torch.zeros((n, od), dtype=torch.float32, device=dev)
        self._mask = None
        if self.passes:
            self.filled_est = torch.zeros((n, NSCAN), dtype=torch.float32, device=dev)
            self.filled_dist = torch.full((n, NSCAN), DIST_UNKNOWN, dtype=torch.uint8, device=dev)
            self.filled_obs = torch.zeros((n, od), dtype=torch.float32, device=dev)
            if dense:
                self.filled_map = torch.full((n, self.grid, self.grid), float("nan"), dtype=torch.float32, device=dev)
                self.filled_dist_map = torch.full((n, self.grid, self.grid), DIST_UNKNOWN, dtype=torch.uint8, device=dev)
        self.dense = bool(dense)
        if self.variance is not None:
            self.var = torch.full((n, self.grid, self.grid), float("nan"), dtype=torch.float32, device=dev)
            self.est_var = torch.full((n, NSCAN), float(self.variance["var_max"]), dtype=torch.float32, device=dev)
        if self.odometry is not None:
            self.pose_est = torch.zeros((7, n), dtype=torch.float32, device=dev)
            self.odo = torch.zeros((n, ODO_WORDS), dtype=torch.float32, device=dev)
            self.odo_counter = torch.zeros(1, dtype=torch.int64, device=dev)
            if source == "lidar":
                self.points_est = torch.full_like(env.lidar_scanner.points, float("nan"))
        if self.visibility is not None:
            self.cleared = torch.zeros(n, dtype=torch.int32, device=dev)
            if dense_bound:
                self.bound = torch.full((n, self.grid, self.grid), float("nan"), dtype=torch.float32, device=dev)
        self.dense_bound = bool(dense_bound)
        if self.latency_cfg is not None:
            slots = self.latency_cfg["ticks"][1] + 1
            check(self._lib.pgtt_elevation_check_latency(C.byref(latency_struct(**self.latency_cfg))))      # before the ring is sized by it
            frame = tuple(env.lidar_scanner.points.shape[1:]) if source == "lidar" else tuple(env.depth.shape[1:])
            self.ring = torch.zeros((slots, n) + frame, dtype=torch.float32, device=dev)
            self.ring_pose = torch.zeros((slots, 7, n), dtype=torch.float32, device=dev)
            self.latency = torch.zeros(n, dtype=torch.int32, device=dev)
            self.latency_age = torch.zeros(n, dtype=torch.int32, device=dev)
            self.fused = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.latency_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        if self.follow_sensor:
            sensor = env.lidar_scanner if source == "lidar" else env.depth_camera
            self.sensor_counter, self.sensor_every = sensor.counter, int(sensor.config.every)
            check(self._lib.pgtt_elevation_bind_rate(self._h, self.sensor_counter.data_ptr(), self.sensor_every))
        self.bind()

    def bind(self) -> None:
        """(re)bind: the env's state (with odometry: the pose estimate), image or points, observation and done flags, this object's outputs"""
        b = PgttElevationBuffers()
        eb = self.env.buffers
        b.state, b.obs = eb["state"].data_ptr(), eb["obs_state"].data_ptr()
        if self.odometry is not None:
            b.state = self.pose_est.data_ptr()                  # rows 0..6 are all the library reads of `state`
        b.done = eb["done"].data_ptr() if eb.get("done") is not None else None
        b.map, b.origin, b.est, b.known, b.obs_out = (t.data_ptr() for t in (self.map, self.origin, self.est, self.known, self.obs))
        if self.source == "lidar":
            pts = self.env.lidar_scanner.points
            check(self._lib.pgtt_elevation_bind_points(self._h, C.byref(b), (pts if self.odometry is None else self.points_est).data_ptr(), pts.shape[1]))
        else:
            b.depth = self.env.depth.data_ptr()
            check(self._lib.pgtt_elevation_bind(self._h, C.byref(b)))
        if self.passes:
            o = PgttElevationFill()
            o.est, o.dist, o.obs_out = self.filled_est.data_ptr(), self.filled_dist.data_ptr(), self.filled_obs.data_ptr()
            if self.dense:
                o.map_out, o.dist_out = self.filled_map.data_ptr(), self.filled_dist_map.data_ptr()
            check(self._lib.pgtt_elevation_bind_fill(self._h, C.byref(o), self.passes))
        if self.variance is not None:
            v = variance_struct(**self.variance, var=self.var.data_ptr(), est_var=self.est_var.data_ptr())
            check(self._lib.pgtt_elevation_bind_var(self._h, C.byref(v)))
        if self.odometry is not None:
            lidar = self.source == "lidar"
            o = odometry_struct(self.env.dt, **self.odometry, env_id_offset=self.env.env_id_offset, state=eb["state"].data_ptr(), done=b.done,
                                points=self.env.lidar_scanner.points.data_ptr() if lidar else None,
                                points_est=self.points_est.data_ptr() if lidar else None, P=self.points_est.shape[1] if lidar else 0,
                                pose_est=self.pose_est.data_ptr(), odo=self.odo.data_ptr(), counter=self.odo_counter.data_ptr())
            check(self._lib.pgtt_elevation_bind_odometry(self._h, C.byref(o)))
        if self.visibility is not None:
            v = visibility_struct(**self.visibility, sensor_pos=self._sensor_pos, cleared=self.cleared.data_ptr(),
                                  bound_out=self.bound.data_ptr() if self.dense_bound else None)
            check(self._lib.pgtt_elevation_bind_visibility(self._h, C.byref(v)))
        if self.latency_cfg is not None:
            l = latency_struct(**self.latency_cfg, env_id_offset=self.env.env_id_offset, D=self.ring.shape[0],
                               ring_data=self.ring.data_ptr(), ring_pose=self.ring_pose.data_ptr(), lat=self.latency.data_ptr(),
                               age=self.latency_age.data_ptr(), fused=self.fused.data_ptr(), counter=self.latency_counter.data_ptr())
            check(self._lib.pgtt_elevation_bind_latency(self._h, C.byref(l)))

    def tick(self, clear_mask: Optional[torch.Tensor] = None, clear_all: bool = False, use_done: bool = False, force: bool = False) -> torch.Tensor:
        """integrate the env's current image (or LiDAR points) under its current pose and sample the scan: one launch on the env's current stream,
        no synchronisation.  Before integrating, the maps of the envs with clear_mask[e] != 0 ([N] uint8 / bool), of every env (clear_all) or of
        the envs whose done flag is set (use_done) are cleared.  With fill > 0 the hole filling is enqueued behind it.
        With follow_sensor (two launches, one of which returns at once) this is so on the calls behind a sensor tick that took new data - `force`
        is what that sensor tick was given; on the others the clears are made, nothing else of the map changes and the scan is sampled from it at
        the current pose.  `force` is not read without follow_sensor.
        With odometry the pose estimate is updated first (two small launches), with the same clear arguments: a cleared env's estimate is the
        truth again and its episode's scale error and gyro bias are drawn anew.
        With visibility the clean-up is enqueued behind that and in front of the tick (one launch), with the same clear arguments.
        With latency the tick is pgtt_elevation_delayed (three launches: the push into the ring, the tick on the frame that is due, the counter)."""
        mp = None
        if clear_mask is not None:
            self._mask = clear_mask.to(self.env.device, torch.uint8).contiguous()      # kept alive until the next tick: the launch is asynchronous
            assert self._mask.shape == (self.env.num_envs,)
            mp = self._mask.data_ptr()
        stream = torch.cuda.current_stream(self.env.device).cuda_stream
        if self.odometry is not None:
            check(self._lib.pgtt_elevation_odometry(self._h, mp, int(bool(clear_all)), int(bool(use_done)), stream))
        if self.visibility is not None:
            check(self._lib.pgtt_elevation_visibility(self._h, mp, int(bool(clear_all)), int(bool(use_done)), stream))
        if self.latency_cfg is not None:
            check(self._lib.pgtt_elevation_delayed(self._h, mp, int(bool(clear_all)), int(bool(use_done)), stream))
        elif self.follow_sensor:
            check(self._lib.pgtt_elevation_follow(self._h, mp, int(bool(clear_all)), int(bool(use_done)), int(bool(force)), stream))
        elif self.variance is not None:
            fn = self._lib.pgtt_elevation_var_points if self.source == "lidar" else self._lib.pgtt_elevation_var
            check(fn(self._h, mp, int(bool(clear_all)), int(bool(use_done)), stream))
        else:
            fn = self._lib.pgtt_elevation_points if self.source == "lidar" else self._lib.pgtt_elevation
            check(fn(self._h, mp, int(bool(clear_all)), int(bool(use_done)), stream))
        if self.passes:
            check(self._lib.pgtt_elevation_fill(self._h, stream))
        return self.obs

    def fill(self) -> torch.Tensor:
        """the hole filling alone, on `map`, `origin` and the env's state and observation as they are: one launch on the env's current stream, no
        synchronisation.  -> filled_obs"""
        if not self.passes:
            raise ElevationError("ElevationMap.fill(): this map was made with fill=0")
        check(self._lib.pgtt_elevation_fill(self._h, torch.cuda.current_stream(self.env.device).cuda_stream))
        return self.filled_obs

    def clean(self, clear_mask: Optional[torch.Tensor] = None, clear_all: bool = False, use_done: bool = False) -> torch.Tensor:
        """the visibility clean-up alone, on `map`, `origin` and the env's pose and image (or points) as they are: one launch on the env's current
        stream, no synchronisation; the clear arguments are those of the tick that is to follow (an env it will clear is skipped).  -> cleared"""
        if self.visibility is None:
            raise ElevationError("ElevationMap.clean(): this map was made without visibility")
        mp = None
        if clear_mask is not None:
            self._mask = clear_mask.to(self.env.device, torch.uint8).contiguous()
            assert self._mask.shape == (self.env.num_envs,)
            mp = self._mask.data_ptr()
        check(self._lib.pgtt_elevation_visibility(self._h, mp, int(bool(clear_all)), int(bool(use_done)), torch.cuda.current_stream(self.env.device).cuda_stream))
        return self.cleared

    def world_cells(self) -> torch.Tensor:
        """[N, G, G, 2] int64: the world cell (ix, iy) each slot of `map` holds under the current window"""
        g = self.grid
        s = torch.arange(g, device=self.map.device)
        lo = self.origin.long() - g // 2                                                # [N, 2]
        wx = lo[:, 0, None] + (s[None] - lo[:, 0, None]) % g
        wy = lo[:, 1, None] + (s[None] - lo[:, 1, None]) % g
        return torch.stack([wx[:, :, None].expand(-1, g, g), wy[:, None, :].expand(-1, g, g)], dim=-1)

    def set_terrain(self, terrain) -> None:
        raise AttributeError("ElevationMap has no terrain")
