"""Batched ray-cast renderer for env frames and rollout videos (libpgtt_render.so, include/pgtt_render.h).

    from phase_guided_terrain_traversal_amd.render import Camera, Renderer, save_gif, scan_points
    r = Renderer(env, 320, 240)                                  # env: a Joystick
    out = r.render([0, 1, 2], camera=Camera("track", distance=2.0, azimuth=120, elevation=-25))
    out["rgb"]                                                   # [3, 240, 320, 3] uint8 on the env's device

The renderer only reads the env's buffers (state, params, variant) and its terrain table; it enqueues two HIP kernels on the env's current
stream and never synchronises.  It is not imported by env.py: nothing on the step path depends on it.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from . import _sidelib, abi

# include/pgtt_render.h
MAX_GEOM, MAX_MARKER, MAX_DIM, MAX_VIEWS = 32, 128, 4096, 16384
SPHERE, CAPSULE, BOX = 0, 1, 2
CAM_MODES = {"fixed": 0, "track": 1, "track_yaw": 2}
SHADOWS = 1
SEG_SKY, SEG_PLANE, SEG_BOX, SEG_GEOM, SEG_MARKER = -1, 0, 1, 1000, 2000
SEG_CELL = 10000                     # + a * G + b, the window cell (a, b) of a map call
MAP_MAX_GRID, MAP_TERRAIN = 96, 1
MAP_COLD, MAP_HOT, MAP_NOVALUE = (0.15, 0.35, 0.85), (0.95, 0.25, 0.10), (0.45, 0.45, 0.45)
MAP_FLOOR_Z, MAP_HEIGHT_RANGE, MAP_OVERLAY_LIFT = -0.05, (-0.1, 1.0), 0.01      # render_map's defaults

f, i32 = C.c_float, C.c_int32


class PgttRenderGeom(C.Structure):
    _fields_ = [("body", i32), ("type", i32), ("pos", f * 3), ("quat", f * 4), ("size", f * 3), ("rgb", f * 3)]


class PgttRenderCamera(C.Structure):
    _fields_ = [("mode", i32), ("target", f * 3), ("distance", f), ("azimuth_deg", f), ("elevation_deg", f), ("fovy_deg", f)]


class PgttRenderViews(C.Structure):
    _fields_ = [("state", C.c_void_p), ("params", C.c_void_p), ("variant", C.c_void_p), ("num_envs", i32), ("num_views", i32),
                ("env_ids", C.POINTER(i32)), ("cameras", C.POINTER(PgttRenderCamera)), ("markers", C.c_void_p), ("num_markers", i32),
                ("width", i32), ("height", i32), ("flags", i32), ("rgba", C.c_void_p), ("depth", C.c_void_p), ("segmentation", C.c_void_p),
                ("body_pose", C.c_void_p), ("workspace", C.c_void_p)]


class PgttRenderMap(C.Structure):
    _fields_ = [("map", C.c_void_p), ("origin", C.c_void_p), ("tint", C.c_void_p), ("grid", i32), ("res", f), ("floor_z", f), ("lift", f),
                ("tint_lo", f), ("tint_hi", f), ("flags", i32)]


assert C.sizeof(PgttRenderGeom) == 60 and C.sizeof(PgttRenderCamera) == 32 and C.sizeof(PgttRenderMap) == 3 * C.sizeof(C.c_void_p) + 7 * 4 + 4


class RenderError(RuntimeError):
    pass


vp = C.c_void_p
SIDE = _sidelib.SideLib("render", RenderError, {
    "pgtt_render_create": (None, [C.POINTER(abi.PgttModel), C.POINTER(PgttRenderGeom), C.c_int, C.c_int, C.POINTER(vp)]),
    "pgtt_render_destroy": (None, [vp]), "pgtt_render_set_terrain": (None, [vp, vp, C.c_int, C.c_int]),
    "pgtt_render_workspace_bytes": (C.c_int64, [C.c_int]), "pgtt_render": (None, [vp, C.POINTER(PgttRenderViews), vp]),
    "pgtt_render_map": (None, [vp, C.POINTER(PgttRenderViews), C.POINTER(PgttRenderMap), vp]),
}, {"pgtt_render_sizeof_geom": PgttRenderGeom, "pgtt_render_sizeof_camera": PgttRenderCamera, "pgtt_render_sizeof_views": PgttRenderViews,
    "pgtt_render_sizeof_map": PgttRenderMap})
LIB_PATH, EXPORTS, lib, check, build_info = SIDE.path, SIDE.exports, SIDE.lib, SIDE.check, SIDE.build_info


# ---------------------------------------------------------------- robot primitives
def _quat_z_to(u: np.ndarray) -> np.ndarray:
    """unit quaternion (wxyz) turning +z onto the unit vector u"""
    z = np.array([0.0, 0.0, 1.0])
    c = float(np.dot(z, u))
    if c < -1.0 + 1e-12:
        return np.array([0.0, 1.0, 0.0, 0.0])
    q = np.concatenate([[1.0 + c], np.cross(z, u)])
    return q / np.linalg.norm(q)


def _capsule(body: int, a, b, radius: float, rgb) -> Dict:
    a, b = np.asarray(a, float), np.asarray(b, float)
    L = float(np.linalg.norm(b - a))
    return dict(body=body, type=CAPSULE, pos=(a + b) / 2, quat=_quat_z_to((b - a) / L), size=np.array([radius, L / 2, 0.0]), rgb=np.asarray(rgb, float))


BASE_RGB, LINK_RGB, CALF_RGB, FOOT_RGB = (0.22, 0.24, 0.28), (0.85, 0.45, 0.12), (0.30, 0.30, 0.32), (0.10, 0.10, 0.10)


def default_robot_geoms(model: Dict) -> List[Dict]:
    """A stick-figure Go2 built from the shipped model constants alone (mjcf.load_model): a base box spanning the hip origins, capsules
    hip -> thigh -> calf -> foot centre along the body chain, and the foot spheres at foot_geom_pos with foot_radius.  Bodies are numbered
    as PgttModel's (0 base, 1 + 3 * leg + {0 hip, 1 thigh, 2 calf}; legs FL, FR, RL, RR).  -> list of dicts (body, type, pos, quat, size, rgb)."""
    bp = np.asarray(model["body_pos"], float)
    hips = bp[[1 + 3 * leg for leg in range(abi.NLEG)]]
    lo, hi = hips.min(0), hips.max(0)
    ident = np.array([1.0, 0.0, 0.0, 0.0])
    geoms = [dict(body=0, type=BOX, pos=(lo + hi) / 2, quat=ident, size=np.array([(hi[0] - lo[0]) / 2, max((hi[1] - lo[1]) / 2, 0.05), 0.045]),
                  rgb=np.asarray(BASE_RGB, float))]
    foot = np.asarray(model["foot_geom_pos"], float)
    radius = np.asarray(model["foot_radius"], float)
    for leg in range(abi.NLEG):
        hip, thigh, calf = 1 + 3 * leg, 2 + 3 * leg, 3 + 3 * leg
        geoms.append(_capsule(hip, np.zeros(3), bp[thigh], 0.022, LINK_RGB))          # body_pos[child] is in the parent's (moving) frame
        geoms.append(_capsule(thigh, np.zeros(3), bp[calf], 0.022, LINK_RGB))
        geoms.append(_capsule(calf, np.zeros(3), foot[leg], 0.013, CALF_RGB))
    for leg in range(abi.NLEG):
        geoms.append(dict(body=3 + 3 * leg, type=SPHERE, pos=foot[leg].copy(), quat=ident, size=np.array([radius[leg], 0.0, 0.0]),
                          rgb=np.asarray(FOOT_RGB, float)))
    return geoms


def geom_array(geoms: Sequence[Dict]):
    arr = (PgttRenderGeom * max(1, len(geoms)))()
    for g, s in zip(geoms, arr):
        s.body, s.type = int(g["body"]), int(g["type"])
        for name, n in (("pos", 3), ("quat", 4), ("size", 3), ("rgb", 3)):
            getattr(s, name)[:] = [float(x) for x in np.asarray(g[name], float).reshape(n)]
    return arr


# ---------------------------------------------------------------- cameras
@dataclass
class Camera:
    """MuJoCo free-camera convention (include/pgtt_render.h).  mode: "fixed" (look at `target`), "track" (look at base position + target),
    "track_yaw" (as track, azimuth measured from the base's heading)."""
    mode: str = "track"
    target: Sequence[float] = (0.0, 0.0, 0.0)
    distance: float = 2.2
    azimuth: float = 120.0
    elevation: float = -25.0
    fovy: float = 45.0

    def struct(self) -> PgttRenderCamera:
        c = PgttRenderCamera()
        c.mode = CAM_MODES[self.mode]
        c.target[:] = [float(x) for x in self.target]
        c.distance, c.azimuth_deg, c.elevation_deg, c.fovy_deg = float(self.distance), float(self.azimuth), float(self.elevation), float(self.fovy)
        return c


def base_yaw(quat) -> float:
    w, x, y, z = np.asarray(quat, float) / np.linalg.norm(quat)
    return float(np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z)))


def camera_basis(cam: Camera, base_pos=None, base_quat=None):
    """fp64 statement of the setup kernel's camera: -> (pos, fwd, right, up)"""
    look = np.asarray(cam.target, float).copy()
    az = float(cam.azimuth)
    if cam.mode != "fixed":
        look = look + np.asarray(base_pos, float)
    if cam.mode == "track_yaw":
        az += np.degrees(base_yaw(base_quat))
    a, e = np.radians(az), np.radians(float(cam.elevation))
    fwd = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    up = np.array([-np.sin(e) * np.cos(a), -np.sin(e) * np.sin(a), np.cos(e)])
    return look - float(cam.distance) * fwd, fwd, np.cross(fwd, up), up


def camera_rays(cam: Camera, width: int, height: int, base_pos=None, base_quat=None, offset=(0.0, 0.0)):
    """fp64 unit ray directions [H, W, 3] through the pixel centres (+ offset in pixels), and the camera origin"""
    pos, fwd, right, up = camera_basis(cam, base_pos, base_quat)
    th = np.tan(np.radians(float(cam.fovy)) / 2)
    px = np.arange(width) + 0.5 + offset[0]
    py = np.arange(height) + 0.5 + offset[1]
    u = (2 * px / width - 1) * th * width / height
    v = (1 - 2 * py / height) * th
    d = fwd[None, None] + u[None, :, None] * right[None, None] + v[:, None, None] * up[None, None]
    return pos, d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---------------------------------------------------------------- height-scan overlay
def scan_grid_xy(base_xy, yaw, scan_dist_x: float = 0.1, scan_dist_y: float = 0.1):
    """world xy of the 13 x 9 scan origins (rows front -> back, cols left -> right; the centre cell at the base itself), as the observe
    kernel forms them.  base_xy [..., 2], yaw [...] (torch or numpy) -> [..., 117, 2]"""
    try:
        import torch
        is_t = isinstance(base_xy, torch.Tensor)
    except ImportError:                                       # pragma: no cover
        is_t = False
    xp = torch if is_t else np
    r = np.repeat(np.arange(abi.SCAN_H), abi.SCAN_W)
    c = np.tile(np.arange(abi.SCAN_W), abi.SCAN_H)
    ox = ((abi.SCAN_H - 1) * 0.5 - r) * scan_dist_x
    oy = ((abi.SCAN_W - 1) * 0.5 - c) * scan_dist_y
    if is_t:
        ox = torch.as_tensor(ox, dtype=base_xy.dtype, device=base_xy.device)
        oy = torch.as_tensor(oy, dtype=base_xy.dtype, device=base_xy.device)
    cy, sy = xp.cos(yaw)[..., None], xp.sin(yaw)[..., None]
    x = base_xy[..., 0:1] + ox * cy - oy * sy
    y = base_xy[..., 1:2] + ox * sy + oy * cy
    return xp.stack([x, y], -1)


def scan_points(env, env_ids=None):
    """world positions [N or len(env_ids), 117, 3] of the height-scan hits: the grid origins at each env's base xy and yaw, z from
    buffers["scan_z"].  Marker overlays for Renderer.render (radius column added by the caller)."""
    import torch
    S = env.buffers["state"]
    q = S[abi.S_QPOS + 3:abi.S_QPOS + 7].T
    xy = S[abi.S_QPOS:abi.S_QPOS + 2].T
    z = env.buffers["scan_z"]
    if env_ids is not None:
        idx = torch.as_tensor(env_ids, dtype=torch.long, device=S.device)
        q, xy, z = q[idx], xy[idx], z[idx]
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, zz = q.unbind(-1)
    yaw = torch.atan2(2 * (w * zz + x * y), 1 - 2 * (y * y + zz * zz))
    cfg = env.config
    g = scan_grid_xy(xy, yaw, cfg.get("scan_dist_x", 0.1), cfg.get("scan_dist_y", 0.1))
    return torch.cat([g, z[..., None]], -1)


# ---------------------------------------------------------------- renderer
class Renderer(_sidelib.Handle):
    """Renders views of a Joystick's envs (state, params, variant and terrain table taken from the env) on the env's device and current
    stream.  Never writes an env buffer."""
    _prefix, _check = "pgtt_render", staticmethod(check)

    def __init__(self, env, width: int, height: int, shadows: bool = True, geoms: Optional[Sequence[Dict]] = None):
        import torch
        self.env, self.width, self.height, self.shadows = env, int(width), int(height), bool(shadows)
        self.geoms = list(default_robot_geoms(env.model) if geoms is None else geoms)
        self._lib = lib()
        self._ms = abi.model_struct(env.model)
        ga = geom_array(self.geoms)
        self._h = C.c_void_p()
        check(self._lib.pgtt_render_create(C.byref(self._ms), ga, len(self.geoms), env.device.index or 0, C.byref(self._h)))
        self.set_terrain(env.terrain)
        self._ws: Dict[int, "torch.Tensor"] = {}

    def _workspace(self, nv: int):
        import torch
        if nv not in self._ws:
            nb = int(self._lib.pgtt_render_workspace_bytes(nv))
            if nb <= 0:
                raise RenderError(f"render: {nv} views (1 .. {MAX_VIEWS} per call)")
            self._ws[nv] = torch.empty(nb, dtype=torch.uint8, device=self.env.device)
        return self._ws[nv]

    def render(self, env_ids, camera: Union[Camera, Sequence[Camera], None] = None, markers=None, depth: bool = False,
               segmentation: bool = False, body_pose: bool = False, outputs: Optional[Dict] = None) -> Dict:
        """env_ids: sequence of V env indices; camera: one Camera for every view or one per view; markers: [V, M, 4] (centre xyz, radius).
        -> {"rgba": [V, H, W, 4] uint8, "rgb": its first three channels, "depth": [V, H, W] float32, "segmentation": [V, H, W] int32,
        "body_pose": [V, 13, 7] float32} (the last three when asked for).  `outputs` may hold preallocated tensors under the same keys."""
        import torch
        v, out, keep = self._views(env_ids, camera, markers, depth, segmentation, body_pose, outputs)
        check(self._lib.pgtt_render(self._h, C.byref(v), torch.cuda.current_stream(self.env.device).cuda_stream))
        out["rgb"] = out["rgba"][..., :3]
        return out

    def _views(self, env_ids, camera, markers, depth, segmentation, body_pose, outputs):
        """the PgttRenderViews of a call, its output dict and what has to outlive the call (host arrays, the converted markers)"""
        import torch
        env = self.env
        ids = [int(i) for i in (env_ids.tolist() if hasattr(env_ids, "tolist") else env_ids)]
        V, H, W = len(ids), self.height, self.width
        cams = [camera or Camera()] * V if camera is None or isinstance(camera, Camera) else list(camera)
        if len(cams) != V:
            raise ValueError("render: one camera, or one per view")
        dev = env.device
        out = dict(outputs or {})
        if "rgba" not in out:
            out["rgba"] = torch.empty((V, H, W, 4), dtype=torch.uint8, device=dev)
        if depth and "depth" not in out:
            out["depth"] = torch.empty((V, H, W), dtype=torch.float32, device=dev)
        if segmentation and "segmentation" not in out:
            out["segmentation"] = torch.empty((V, H, W), dtype=torch.int32, device=dev)
        if body_pose and "body_pose" not in out:
            out["body_pose"] = torch.empty((V, abi.NBODY, 7), dtype=torch.float32, device=dev)
        v = PgttRenderViews()
        v.state, v.params, v.variant = _sidelib.env_pointers(env)
        v.num_envs, v.num_views = env.num_envs, V
        id_arr = (i32 * max(1, V))(*ids)
        cam_arr = (PgttRenderCamera * max(1, V))(*[c.struct() for c in cams])
        v.env_ids, v.cameras = id_arr, cam_arr
        mk = None
        if markers is not None:
            mk = markers.to(dev, torch.float32).contiguous()
            if mk.dim() != 3 or mk.shape[0] != V or mk.shape[2] != 4:
                raise ValueError("render: markers must be [V, M, 4]")
            v.markers, v.num_markers = mk.data_ptr(), mk.shape[1]
        v.width, v.height, v.flags = W, H, SHADOWS if self.shadows else 0
        v.rgba = out["rgba"].data_ptr()
        for k in ("depth", "segmentation", "body_pose"):
            setattr(v, k, out[k].data_ptr() if k in out else None)
        v.workspace = self._workspace(V).data_ptr() if 1 <= V <= MAX_VIEWS else None
        return v, out, (id_arr, cam_arr, mk)

    def render_map(self, env_ids, map, camera: Union[Camera, Sequence[Camera], None] = None, markers=None, depth: bool = False,
                   segmentation: bool = False, outputs: Optional[Dict] = None, terrain: bool = False, lift: Optional[float] = None,
                   floor_z: Optional[float] = None, tint=None, tint_range=None) -> Dict:
        """The views of render() with an elevation map drawn as a height field of cell columns (pgtt_render_map, include/pgtt_render.h): the
        belief view, or with terrain=True the map lifted over the true scene.
        map: an elevation.ElevationMap (its map, origin, grid and res), or dict(map=[N, G, G] float32, origin=[N, 2] int32, grid=G, res=) of
        tensors on the env's device, in the map's slot layout; NaN = not drawn.
        tint: None / "height" (the colour follows the height, over tint_range or (-0.1, 1.0)), "var" (an ElevationMap's variance layer, over
        (0, var_max)), "dist" (a dense fill's distance layer over (0, passes), with the FILLED map as the heights), or any [N, G, G] float32
        tensor in the same layout (over tint_range, or (0, 1)); a NaN tint shows MAP_NOVALUE.
        floor_z: the plane every column stands on (-0.05 unless given); lift: added to every height when drawn (0, or 0.01 with terrain=True).
        -> the dict render() returns."""
        import torch
        dev = self.env.device
        if isinstance(map, dict):
            missing = [k for k in ("map", "origin", "grid", "res") if k not in map]
            if missing:
                raise ValueError(f"render_map: the map dict lacks {missing}")
            hmap, origin, G, res, emap = map["map"], map["origin"], int(map["grid"]), float(map["res"]), None
        else:
            hmap, origin, G, res, emap = map.map, map.origin, int(map.grid), float(map.res), map
        lo_hi = None
        if tint is None or (isinstance(tint, str) and tint == "height"):
            layer, lo_hi = None, MAP_HEIGHT_RANGE
        elif isinstance(tint, str):
            if emap is None:
                raise ValueError(f"render_map: tint={tint!r} names a layer of an ElevationMap; with a dict give the layer itself")
            if tint == "var":
                if getattr(emap, "variance", None) is None:
                    raise ValueError("render_map: tint='var' needs a map made with variance=")
                layer, lo_hi = emap.var, (0.0, float(emap.variance["var_max"]))
            elif tint == "dist":
                if not getattr(emap, "dense", False):
                    raise ValueError("render_map: tint='dist' needs a map made with fill > 0 and dense=True")
                hmap, layer, lo_hi = emap.filled_map, emap.filled_dist_map.to(torch.float32), (0.0, float(emap.passes))
            else:
                raise ValueError(f"render_map: tint must be None, 'height', 'var', 'dist' or a tensor, not {tint!r}")
        else:
            layer, lo_hi = tint, (0.0, 1.0)
        if tint_range is not None:
            lo_hi = (float(tint_range[0]), float(tint_range[1]))
        if not 1 <= G <= MAP_MAX_GRID:
            raise ValueError(f"render_map: grid must be in [1, {MAP_MAX_GRID}], not {G}")
        n = self.env.num_envs
        for name, t, shape, dtype in (("map", hmap, (n, G, G), torch.float32), ("origin", origin, (n, 2), torch.int32), ("tint", layer, (n, G, G), torch.float32)):
            if t is None and name == "tint":
                continue
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"render_map: {name} must be a tensor")
            if tuple(t.shape) != shape or t.dtype != dtype:
                raise ValueError(f"render_map: {name} must be {list(shape)} {dtype}, not {list(t.shape)} {t.dtype}")
            if t.device != dev:
                raise ValueError(f"render_map: {name} is on {t.device}, the env on {dev}")
            if not t.is_contiguous():
                raise ValueError(f"render_map: {name} must be contiguous")
        v, out, keep = self._views(env_ids, camera, markers, depth, segmentation, False, outputs)
        m = PgttRenderMap()
        m.map, m.origin, m.tint = hmap.data_ptr(), origin.data_ptr(), None if layer is None else layer.data_ptr()
        m.grid, m.res = G, res
        m.floor_z = MAP_FLOOR_Z if floor_z is None else float(floor_z)
        m.lift = (MAP_OVERLAY_LIFT if terrain else 0.0) if lift is None else float(lift)
        m.tint_lo, m.tint_hi = lo_hi
        m.flags = MAP_TERRAIN if terrain else 0
        check(self._lib.pgtt_render_map(self._h, C.byref(v), C.byref(m), torch.cuda.current_stream(dev).cuda_stream))
        out["rgb"] = out["rgba"][..., :3]
        return out


# ---------------------------------------------------------------- writers
def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(img) -> bytes:
    """8-bit RGB / RGBA / grey image [H, W(, C)] -> PNG file contents (stdlib zlib, filter 0 on every row)"""
    a = np.ascontiguousarray(np.asarray(img, dtype=np.uint8))
    if a.ndim == 2:
        a = a[..., None]
    h, w, ch = a.shape
    ctype = {1: 0, 3: 2, 4: 6}[ch]
    raw = b"".join(b"\x00" + a[y].tobytes() for y in range(h))
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
            + _png_chunk(b"IDAT", zlib.compress(raw, 6)) + _png_chunk(b"IEND", b""))


def save_png(path: str, img) -> str:
    with open(path, "wb") as fh:
        fh.write(png_bytes(img))
    return path


def save_gif(path: str, frames, fps: float = 25.0) -> str:
    """frames [T, H, W, 3] uint8 -> an animated GIF at `path` (PIL), or, where PIL cannot be imported, a PNG sequence in the directory
    `<path without extension>_frames/`.  -> what was written"""
    frames = np.asarray(frames, dtype=np.uint8)
    try:
        from PIL import Image
    except ImportError:
        out = os.path.splitext(path)[0] + "_frames"
        os.makedirs(out, exist_ok=True)
        print(f"save_gif: PIL is not available, writing {len(frames)} PNG frames to {out}/")
        for k, fr in enumerate(frames):
            save_png(os.path.join(out, f"frame_{k:05d}.png"), fr)
        return out
    ims = [Image.fromarray(fr) for fr in frames]
    ims[0].save(path, save_all=True, append_images=ims[1:], duration=max(1, int(round(1000.0 / fps))), loop=0, optimize=False)
    return path
