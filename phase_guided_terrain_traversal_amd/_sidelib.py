"""What the modules of the six side libraries share - render.py (libpgtt_render.so), depth.py (libpgtt_depth.so), perceive.py
(libpgtt_perceive.so), elevation.py (libpgtt_elevation.so), learn.py (libpgtt_learn.so) and lidar.py (libpgtt_lidar.so): SideLib, which loads a side library through ctypes,
turns its return codes into the module's exception and parses its build info; the terrain / close methods of a handle's owner; the three env
pointers the three ray casters read; and RaySensor, what the depth camera and the LiDAR both do around their own buffers.  Imported by those
modules only: env.py does not reach it unless a depth camera, a LiDAR, a student or an elevation map is asked for."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence, Tuple, Type

import numpy as np

from . import abi


class SideLib:
    """libpgtt_<name>.so next to the package, opened when first asked for.  prototypes = {function: (restype or None to keep int, argtypes or
    None)}, sizeofs = {pgtt_<name>_sizeof_* function: the ctypes mirror it must agree with}; the two uniform exports pgtt_<name>_last_error and
    pgtt_<name>_build_info are added here.  `exports` is every function named: the module's EXPORTS.  `path` may be set before the first lib()
    (tools/gpu_ab_raycast.py loads two builds that way); `error` is the module's exception class."""

    def __init__(self, name: str, error: Type[Exception], prototypes: Dict[str, Tuple[object, Optional[Sequence]]], sizeofs: Dict[str, type]):
        self.prefix = "pgtt_" + name
        self.path = os.path.join(os.path.dirname(os.path.abspath(__file__)), f"lib{self.prefix}.so")
        self.error, self.sizeofs = error, sizeofs
        self.prototypes = {**prototypes, self.prefix + "_last_error": (C.c_char_p, None), self.prefix + "_build_info": (C.c_char_p, None)}
        self.exports = list(self.prototypes) + list(sizeofs)
        self._lib: Optional[C.CDLL] = None

    def lib(self) -> C.CDLL:
        """the library at `path`, as it is when it is first asked for"""
        if self._lib is None:
            if not os.path.exists(self.path):
                raise self.error(f"{self.path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                 "(hipcc --offload-arch=gfx950); there is no CPU fallback")
            # torch's own HIP runtime first, as native.lib() does for libpgtt.so
            import torch  # noqa: F401
            L = C.CDLL(self.path)
            for name, (restype, argtypes) in self.prototypes.items():
                fn = getattr(L, name)
                if restype is not None:
                    fn.restype = restype
                if argtypes is not None:
                    fn.argtypes = list(argtypes)
            for name, mirror in self.sizeofs.items():
                assert getattr(L, name)() == C.sizeof(mirror), name
            self._lib = L
        return self._lib

    def check(self, rc: int) -> None:
        if rc != 0:
            raise self.error(f"lib{self.prefix} error {rc}: {getattr(self.lib(), self.prefix + '_last_error')().decode()}")

    def build_info(self) -> dict:
        """{"src": srchash.side_sha256(name) when the library was built, "flavor": "product" or an experiment's name}"""
        return dict(kv.split("=", 1) for kv in getattr(self.lib(), self.prefix + "_build_info")().decode().split(";"))


def env_pointers(env):
    """-> (state, params, variant): device pointers of a Joystick's buffers, None for one the env does not have"""
    b = env.buffers
    return (b["state"].data_ptr(), b["params"].data_ptr() if "params" in b else None, b["variant"].data_ptr() if "variant" in b else None)


class Handle:
    """owner of one library handle `_h` of `_lib`: the subclass sets _prefix and _check (its module's check)"""
    _prefix = ""
    _check = staticmethod(lambda rc: None)

    def set_terrain(self, terrain) -> None:
        fn = getattr(self._lib, self._prefix + "_set_terrain")
        if terrain is None:
            self._check(fn(self._h, None, 0, 0))
            return
        t = np.ascontiguousarray(terrain, dtype=np.float32)
        assert t.ndim == 3 and t.shape[2] == 10 and t.shape[1] <= abi.MAX_BOX
        self._check(fn(self._h, t.ctypes.data, t.shape[0], t.shape[1]))

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(self._lib, self._prefix + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fill_sensor_config(c, near, far, mount_body, mount_pos, mount_quat, every, see_robot, sigma, dropout, seed, env_id_offset):
    """the fields PgttDepthConfig and PgttLidarConfig both have, set on `c`; no checks: the library makes its own"""
    c.near, c.far, c.mount_body, c.every, c.see_robot = float(near), float(far), int(mount_body), int(every), int(bool(see_robot))
    c.mount_pos[:] = [float(x) for x in mount_pos]
    c.mount_quat[:] = [float(x) for x in mount_quat]
    c.noise_sigma, c.dropout, c.seed, c.env_id_offset = float(sigma), float(dropout), int(seed) & (2 ** 64 - 1), int(env_id_offset)
    return c


def noise_args(noise: Optional[Dict]):
    """-> (sigma, dropout, seed) of a sensor's `noise` setting, None or a dict"""
    noise = dict(noise or {})
    return noise.get("sigma", 0.0), noise.get("dropout", 0.0), noise.get("seed", 0)


class RaySensor(Handle):
    """a sensor mounted on every env of a Joystick, DepthCamera or LidarScanner: the subclass also sets _side (its module's SideLib), owns its
    output buffers and binds them"""
    _side: Optional[SideLib] = None

    def _create(self, env, config, geoms, *pattern) -> None:
        """pgtt_<x>_create(model, config, *pattern, geoms, ngeom, device, num_envs, &handle), the env's terrain, the tick counter"""
        import torch
        from . import render
        self.env, self.config = env, config
        self.geoms = list(render.default_robot_geoms(env.model) if geoms is None else geoms)
        self._lib = self._side.lib()
        self._ms = abi.model_struct(env.model)
        self._h = C.c_void_p()
        self._check(getattr(self._lib, self._prefix + "_create")(C.byref(self._ms), C.byref(config), *pattern, render.geom_array(self.geoms),
                                                                 len(self.geoms), env.device.index or 0, env.num_envs, C.byref(self._h)))
        self.set_terrain(env.terrain)
        self.counter = torch.zeros(1, dtype=torch.int64, device=env.device)

    def _tick(self, force: bool) -> None:
        """pgtt_<x>(handle, force, stream) on the env's current stream"""
        import torch
        self._check(getattr(self._lib, self._prefix)(self._h, int(bool(force)), torch.cuda.current_stream(self.env.device).cuda_stream))
