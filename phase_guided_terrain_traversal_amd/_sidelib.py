"""What render.py (libpgtt_render.so), depth.py (libpgtt_depth.so) and perceive.py (libpgtt_perceive.so) share: loading a side library through
ctypes, turning its return codes into the module's exception, parsing its build info, the terrain / close methods of a handle's owner, and the three
env pointers the two ray casters read.  Imported by those modules only: env.py does not reach it unless a depth camera or a student is asked for."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Sequence, Tuple, Type

import numpy as np

from . import abi


def load(path: str, error: Type[Exception], prototypes: Dict[str, Tuple[object, Sequence]], sizeofs: Dict[str, type]) -> C.CDLL:
    """open the library at `path`: prototypes = {function: (restype or None to keep int, argtypes or None)}, sizeofs = {function: ctypes mirror}"""
    if not os.path.exists(path):
        raise error(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # torch's own HIP runtime first, as native.lib() does for libpgtt.so
    import torch  # noqa: F401
    L = C.CDLL(path)
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(L, name)
        if restype is not None:
            fn.restype = restype
        if argtypes is not None:
            fn.argtypes = list(argtypes)
    for name, mirror in sizeofs.items():
        assert getattr(L, name)() == C.sizeof(mirror), name
    return L


def check(rc: int, L: C.CDLL, prefix: str, error: Type[Exception]) -> None:
    """prefix: "pgtt_render" / "pgtt_depth", the functions' common beginning; the library is lib<prefix>.so"""
    if rc != 0:
        raise error(f"lib{prefix} error {rc}: {getattr(L, prefix + '_last_error')().decode()}")


def build_info(L: C.CDLL, prefix: str) -> dict:
    return dict(kv.split("=", 1) for kv in getattr(L, prefix + "_build_info")().decode().split(";"))


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
