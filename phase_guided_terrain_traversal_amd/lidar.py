"""Onboard LiDAR: one range and one world point per ray per env per sensor tick (libpgtt_lidar.so, include/pgtt_lidar.h).

    from phase_guided_terrain_traversal_amd.lidar import LidarScanner, spherical_pattern
    lid = LidarScanner(env, pattern=spherical_pattern(128, 16, (-180, 180), (-85, 10)), near=0.05, far=3.0, mount_pos=(0.29, 0.0, -0.04))
    lid.tick()                   # one launch pair on the env's current stream, no synchronisation
    lid.ranges                   # [N, R] float32 on the env's device: metres along the ray, `far` on a miss
    lid.points                   # [N, R, 3] float32: the world point of every return strictly inside (near, far), NaN otherwise

`Joystick(..., lidar=dict(...))` owns one and ticks it after every step (env.lidar, env.lidar_points).  The sensor only reads the env's buffers
(state, params, variant) and its terrain table.  It is not imported by env.py unless asked for.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import _sidelib, abi
from .render import PgttRenderGeom

# include/pgtt_lidar.h
MAX_RAYS = 8192
RS_LIDAR = 33
# Joystick(lidar=...) / evaluate.py --elevation_source lidar: placeholders for a chin-mounted hemispherical scanner of a Go2 - all round the
# robot, from almost straight down to a little above the horizon, 2048 rays - settings, not measured facts about a product
DEFAULTS = dict(n_az=128, n_el=16, az_deg=(-180.0, 180.0), el_deg=(-85.0, 10.0), near=0.05, far=3.0, mount_body=0, mount_pos=(0.29, 0.0, -0.04),
                mount_quat=(1.0, 0.0, 0.0, 0.0), every=1, see_robot=True, noise=None)


def spherical_pattern(n_az: int, n_el: int, az_deg=(-180.0, 180.0), el_deg=(-85.0, 10.0)) -> np.ndarray:
    """[n_az * n_el, 3] float64 unit directions in the sensor frame, d = (cos el cos az, cos el sin az, sin el); ray r = a * n_el + k.  The n_az
    azimuths are the centres of n_az equal cells of az_deg = (lo, hi) (a full turn repeats no direction), the n_el elevations are spread over the
    closed interval el_deg = (lo, hi) (n_el = 1: its middle)."""
    n_az, n_el = int(n_az), int(n_el)
    if n_az < 1 or n_el < 1:
        raise ValueError("spherical_pattern: n_az and n_el must be >= 1")
    az = np.radians(az_deg[0] + (np.arange(n_az) + 0.5) * (az_deg[1] - az_deg[0]) / n_az)
    el = np.radians(np.linspace(el_deg[0], el_deg[1], n_el) if n_el > 1 else np.array([0.5 * (el_deg[0] + el_deg[1])]))
    ce = np.cos(el)
    d = np.stack([ce[None, :] * np.cos(az)[:, None], ce[None, :] * np.sin(az)[:, None], np.broadcast_to(np.sin(el)[None, :], (n_az, n_el))], -1)
    return d.reshape(n_az * n_el, 3)


def settings(overrides: Optional[Dict] = None) -> Dict:
    """LidarScanner's keyword arguments: DEFAULTS with `overrides` on top.  A `pattern` given replaces the spherical pattern's four settings."""
    kw = {**DEFAULTS, **dict(overrides or {})}
    if kw.get("pattern") is not None:
        for k in ("n_az", "n_el", "az_deg", "el_deg"):
            if k not in (overrides or {}):
                kw.pop(k, None)
    return kw


f, i32, vp = C.c_float, C.c_int32, C.c_void_p


class PgttLidarConfig(C.Structure):
    _fields_ = [("near", f), ("far", f), ("mount_body", i32), ("mount_pos", f * 3), ("mount_quat", f * 4), ("every", i32), ("see_robot", i32),
                ("noise_sigma", f), ("dropout", f), ("seed", C.c_uint64), ("env_id_offset", C.c_int64)]


class PgttLidarBuffers(C.Structure):
    _fields_ = [("state", vp), ("params", vp), ("variant", vp), ("range", vp), ("points", vp), ("counter", vp)]


assert C.sizeof(PgttLidarConfig) == 72 and C.sizeof(PgttLidarBuffers) == 48


class LidarError(RuntimeError):
    pass


SIDE = _sidelib.SideLib("lidar", LidarError, {
    "pgtt_lidar_check": (None, [C.POINTER(PgttLidarConfig), vp, C.c_int]),
    "pgtt_lidar_create": (None, [C.POINTER(abi.PgttModel), C.POINTER(PgttLidarConfig), vp, C.c_int, C.POINTER(PgttRenderGeom), C.c_int, C.c_int,
                                 C.c_int, C.POINTER(vp)]),
    "pgtt_lidar_destroy": (None, [vp]), "pgtt_lidar_set_terrain": (None, [vp, vp, C.c_int, C.c_int]),
    "pgtt_lidar_bind": (None, [vp, C.POINTER(PgttLidarBuffers)]), "pgtt_lidar": (None, [vp, C.c_int, vp]),
}, {"pgtt_lidar_sizeof_config": PgttLidarConfig, "pgtt_lidar_sizeof_buffers": PgttLidarBuffers})
LIB_PATH, EXPORTS, lib, check, build_info = SIDE.path, SIDE.exports, SIDE.lib, SIDE.check, SIDE.build_info


def config_struct(near, far, mount_body=0, mount_pos=(0.0, 0.0, 0.0), mount_quat=(1.0, 0.0, 0.0, 0.0), every=1, see_robot=True, sigma=0.0,
                  dropout=0.0, seed=0, env_id_offset=0) -> PgttLidarConfig:
    """no checks: the library makes its own (pgtt_lidar_check)"""
    c = PgttLidarConfig()
    return _sidelib.fill_sensor_config(c, near, far, mount_body, mount_pos, mount_quat, every, see_robot, sigma, dropout, seed, env_id_offset)


def pattern_array(pattern) -> np.ndarray:
    """the pattern as the contiguous float32 [R, 3] table the library takes"""
    p = np.ascontiguousarray(pattern, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"a LiDAR pattern is an [R, 3] table of directions, not {p.shape}")
    return p


def check_settings(config: PgttLidarConfig, pattern) -> None:
    """pgtt_lidar_check: the library's own refusals of a config and a pattern, without a GPU (LidarError)"""
    p = np.ascontiguousarray(pattern, dtype=np.float32).reshape(-1, 3)
    check(lib().pgtt_lidar_check(C.byref(config), p.ctypes.data if p.size else None, p.shape[0]))


class LidarScanner(_sidelib.RaySensor):
    """A scanning range sensor rigidly mounted on body `mount_body` (0 = the torso) of every env of a Joystick, pose (mount_pos, mount_quat wxyz) in
    that body's frame.  pattern: [R, 3] ray directions in the sensor frame (normalised by the library), or n_az / n_el / az_deg / el_deg of
    spherical_pattern.  every: the sensor period in ticks; see_robot: the robot's own primitives (`geoms`, default
    render.default_robot_geoms(model)) are in the scene; noise: None or dict(sigma=relative range noise, dropout=probability of a `far` reading,
    seed=0), the draws keyed by (seed, env.env_id_offset + env, tick counter, ray) as the env's own streams are.
    The defaults of Joystick(lidar=...) (lidar.DEFAULTS) are placeholders for a chin-mounted hemispherical scanner: settings, not facts.
    Runs on the env's device and current stream; writes nothing but `ranges`, `points` and `counter`."""
    _side, _prefix, _check = SIDE, SIDE.prefix, staticmethod(check)

    def __init__(self, env, near: float, far: float, pattern=None, n_az: Optional[int] = None, n_el: Optional[int] = None, az_deg=(-180.0, 180.0),
                 el_deg=(-85.0, 10.0), mount_body: int = 0, mount_pos: Sequence[float] = (0.0, 0.0, 0.0),
                 mount_quat: Sequence[float] = (1.0, 0.0, 0.0, 0.0), every: int = 1, see_robot: bool = True, noise: Optional[Dict] = None,
                 geoms: Optional[Sequence[Dict]] = None, points: bool = True):
        import torch
        if (pattern is None) == (n_az is None or n_el is None):
            raise ValueError("LidarScanner: give pattern=[R, 3] or n_az and n_el, not both")
        self.pattern = pattern_array(spherical_pattern(n_az, n_el, az_deg, el_deg) if pattern is None else pattern)
        self.near, self.far, self.every, self.num_rays = float(near), float(far), int(every), int(self.pattern.shape[0])
        self._create(env, config_struct(near, far, mount_body, mount_pos, mount_quat, every, see_robot, *_sidelib.noise_args(noise), env.env_id_offset),
                     geoms, self.pattern.ctypes.data if self.num_rays else None, self.num_rays)
        self.ranges = torch.zeros((env.num_envs, self.num_rays), dtype=torch.float32, device=env.device)
        self.points = torch.full((env.num_envs, self.num_rays, 3), float("nan"), dtype=torch.float32, device=env.device) if points else None
        self.bind()

    def bind(self) -> None:
        """(re)bind the env's buffers (after the env replaced one of state / params / variant)"""
        b = PgttLidarBuffers()
        b.state, b.params, b.variant = _sidelib.env_pointers(self.env)
        b.range, b.counter = self.ranges.data_ptr(), self.counter.data_ptr()
        b.points = None if self.points is None else self.points.data_ptr()
        check(self._lib.pgtt_lidar_bind(self._h, C.byref(b)))

    def tick(self, force: bool = False):
        """one sensor tick: the scan is recomputed when `force` or the counter is 0 modulo `every` (decided on the device), the counter advances"""
        self._tick(force)
        return self.ranges
