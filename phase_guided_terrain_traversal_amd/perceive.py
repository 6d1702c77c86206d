"""Student perception: the 117 height-scan rows of the observation estimated from the onboard depth image and the proprioceptive rows
(libpgtt_perceive.so, include/pgtt_perceive.h), so that a policy trained on the privileged scan acts on what a robot can sense.

    est = ScanEstimator(config(env.method))          # torch: Conv2d / SiLU / Linear - what train_student.py differentiates
    sp = StudentPerception(env, est)                 # the same function as two HIP launches; sp.obs is obs with the scan rows replaced
    sp.tick(); sp.est; sp.obs
    sp.load(est)                                     # repack in place after an optimiser step

`Joystick(..., depth=dict(...), student=path_or_estimator)` owns one and ticks it behind the camera (env.student_obs).  The module is not imported
by env.py unless a student is asked for.  The backward pass is torch autograd on ScanEstimator; the library is forward only.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _sidelib, abi, acting, depth as _depth

# include/pgtt_perceive.h
MAX_CONV, MAX_CH, MAX_PROP, MAX_HIDDEN, MAX_DIM, LDS_BYTES, NLAYER, OUT_PAD = 3, 64, 64, 512, 256, 61440, 5, 128
NSCAN = abi.NSCAN
SCAN_ROW0 = {"pgtt": 38, "baseline": 30}           # the scan rows sit between phase / joint_vel and gait_freq / last_act
# the scan grid is 13 rows (x, ahead first) by 9 columns: the bands train_student.py reports
BANDS = {"ahead": slice(0, 6 * abi.SCAN_W), "under": slice(6 * abi.SCAN_W, 7 * abi.SCAN_W), "behind": slice(7 * abi.SCAN_W, NSCAN)}


def config(method: str = "pgtt", **overrides) -> Dict:
    """the default net for the task definition `method`: depth.DEFAULTS' 48 x 64 image -> 16 ch k5 s2 -> 32 ch k3 s2 -> 32 ch k3 s2 (F = 768), the
    proprioceptive input = every observation row except the scan rows (54 for the PGTT task), hidden 512"""
    od, row0 = abi.obs_dims(method)[0], SCAN_ROW0[method]
    c = dict(height=_depth.DEFAULTS["height"], width=_depth.DEFAULTS["width"], near=_depth.DEFAULTS["near"], far=_depth.DEFAULTS["far"],
             conv=[(16, 5, 2), (32, 3, 2), (32, 3, 2)], prop_rows=[r for r in range(od) if not row0 <= r < row0 + NSCAN], hidden=512,
             obs_dim=od, scan_row0=row0)
    c.update(overrides)
    return c


DEFAULTS = config("pgtt")

i32, f = C.c_int32, C.c_float


class PgttPerceiveConfig(C.Structure):
    _fields_ = [("height", i32), ("width", i32), ("near", f), ("far", f), ("n_conv", i32), ("out_ch", i32 * MAX_CONV), ("kernel", i32 * MAX_CONV),
                ("stride", i32 * MAX_CONV), ("n_prop", i32), ("prop_rows", i32 * MAX_PROP), ("hidden", i32), ("obs_dim", i32), ("scan_row0", i32)]


class PgttPerceiveBuffers(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("obs", C.c_void_p), ("w", C.c_void_p * NLAYER), ("b", C.c_void_p * NLAYER), ("latent", C.c_void_p),
                ("est", C.c_void_p), ("obs_out", C.c_void_p)]


assert C.sizeof(PgttPerceiveConfig) == 328 and C.sizeof(PgttPerceiveBuffers) == 120


class PerceiveError(RuntimeError):
    pass


vp, cp = C.c_void_p, C.POINTER(PgttPerceiveConfig)
SIDE = _sidelib.SideLib("perceive", PerceiveError, {
    "pgtt_perceive_check": (None, [cp]), "pgtt_perceive_latent_dim": (None, [cp]), "pgtt_perceive_packed_floats": (None, [cp, C.c_int]),
    "pgtt_perceive_create": (None, [cp, C.c_int, C.c_int, C.POINTER(vp)]), "pgtt_perceive_destroy": (None, [vp]),
    "pgtt_perceive_bind": (None, [vp, C.POINTER(PgttPerceiveBuffers)]), "pgtt_perceive": (None, [vp, vp]),
}, {"pgtt_perceive_sizeof_config": PgttPerceiveConfig, "pgtt_perceive_sizeof_buffers": PgttPerceiveBuffers})
LIB_PATH, EXPORTS, lib, check, build_info = SIDE.path, SIDE.exports, SIDE.lib, SIDE.check, SIDE.build_info


def conv_shapes(cfg: Dict) -> List[Tuple[int, int, int]]:
    """[(channels, height, width)] of the input and of every conv's output; no padding, no dilation"""
    shapes = [(1, int(cfg["height"]), int(cfg["width"]))]
    for co, k, s in cfg["conv"]:
        _, h, w = shapes[-1]
        shapes.append((int(co), (h - k) // s + 1 if h >= k else 0, (w - k) // s + 1 if w >= k else 0))
    return shapes


def lds_bytes(cfg: Dict) -> int:
    """the kernel's LDS budget formula (pgtt_perceive.h): 4 * (max(a_0, a_2) + a_1) with a_l the floats of the image and of every conv output
    but the last, which goes to the latent"""
    a = [c * h * w for c, h, w in conv_shapes(cfg)][:-1] + [0, 0]
    return 4 * (max(a[0], a[2]) + a[1])


def check_config(cfg: Dict) -> None:
    """the refusals of pgtt_perceive_check, on the host and without the library: ValueError"""
    def no(msg):
        raise ValueError("perceive config: " + msg)
    if not (1 <= cfg["height"] <= MAX_DIM and 1 <= cfg["width"] <= MAX_DIM):
        no("height and width must be in [1, 256]")
    if not (np.isfinite(cfg["near"]) and np.isfinite(cfg["far"]) and cfg["near"] < cfg["far"]):
        no("need near < far, finite")
    if not 1 <= len(cfg["conv"]) <= MAX_CONV:
        no("1 to 3 conv layers")
    if cfg["hidden"] % 16 or not 16 <= cfg["hidden"] <= MAX_HIDDEN:
        no("hidden must be a multiple of 16 in [16, 512]")
    if cfg["obs_dim"] < 1 or cfg["scan_row0"] < 0 or cfg["scan_row0"] + NSCAN > cfg["obs_dim"]:
        no("need 0 <= scan_row0 and scan_row0 + 117 <= obs_dim")
    if len(cfg["prop_rows"]) > MAX_PROP:
        no("at most 64 prop_rows")
    if any(not 0 <= int(r) < cfg["obs_dim"] for r in cfg["prop_rows"]):
        no("prop_rows entry outside [0, obs_dim)")
    for (co, k, s), (_, h, w) in zip(cfg["conv"], conv_shapes(cfg)):
        if co % 16 or not 16 <= co <= MAX_CH:
            no("out_ch must be a multiple of 16 in [16, 64]")
        if k not in (3, 5) or s not in (1, 2):
            no("kernel must be 3 or 5, stride 1 or 2")
        if h < k or w < k:
            no("a conv layer's output would be empty")
    if lds_bytes(cfg) > LDS_BYTES:
        no(f"the activations ({lds_bytes(cfg)} bytes) do not fit the LDS budget of {LDS_BYTES}")


def config_struct(cfg: Dict) -> PgttPerceiveConfig:
    """no checks: the library makes its own"""
    c = PgttPerceiveConfig()
    c.height, c.width, c.near, c.far = int(cfg["height"]), int(cfg["width"]), float(cfg["near"]), float(cfg["far"])
    c.n_conv = len(cfg["conv"])
    for l, (co, k, s) in enumerate(cfg["conv"][:MAX_CONV]):
        c.out_ch[l], c.kernel[l], c.stride[l] = int(co), int(k), int(s)
    c.n_prop = len(cfg["prop_rows"])
    for j, r in enumerate(cfg["prop_rows"][:MAX_PROP]):
        c.prop_rows[j] = int(r)
    c.hidden, c.obs_dim, c.scan_row0 = int(cfg["hidden"]), int(cfg["obs_dim"]), int(cfg["scan_row0"])
    return c


def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [O, C, k, k] -> the tile order of pgtt_perceive.h: the matrix [O][K = C k k], K zero-padded to a multiple of 4,
    packed[mt][ks][g][i] = W[16 mt + i][4 ks + g]"""
    o = w.shape[0]
    m = w.detach().reshape(o, -1)
    kp = -(-m.shape[1] // 4) * 4
    m = torch.nn.functional.pad(m, (0, kp - m.shape[1]))
    return m.view(o // 16, 16, kp // 4, 4).permute(0, 2, 3, 1).contiguous().reshape(-1)


def unpack_conv(p: torch.Tensor, o: int, c: int, k: int) -> torch.Tensor:
    kp = -(-(c * k * k) // 4) * 4
    m = p.view(o // 16, kp // 4, 4, 16).permute(0, 3, 1, 2).reshape(o, kp)
    return m[:, :c * k * k].reshape(o, c, k, k).contiguous()


def unpack_linear(p: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """inverse of acting.pack_linear"""
    npad, kpad = -(-n // 16) * 16, -(-k // 16) * 16
    return p.view(npad // 16, kpad // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(npad, kpad)[:n, :k].contiguous()


def preprocess(d: torch.Tensor, near: float, far: float) -> torch.Tensor:
    """depth in metres -> [-0.5, 0.5]: clamp to [near, far], a NaN reads as far"""
    d = torch.where(torch.isnan(d), torch.full_like(d, far), d)
    return (torch.clamp(d, near, far) - near) / (far - near) - 0.5


class ScanEstimator(torch.nn.Module):
    """The function of pgtt_perceive.h in torch, built from the same config dict (perceive.config): what distillation differentiates."""

    def __init__(self, cfg: Optional[Dict] = None):
        super().__init__()
        cfg = dict(DEFAULTS if cfg is None else cfg)
        cfg["conv"] = [tuple(int(v) for v in l) for l in cfg["conv"]]
        cfg["prop_rows"] = [int(r) for r in cfg["prop_rows"]]
        check_config(cfg)
        self.cfg = cfg
        shapes = conv_shapes(cfg)
        self.convs = torch.nn.ModuleList(torch.nn.Conv2d(shapes[l][0], co, k, s) for l, (co, k, s) in enumerate(cfg["conv"]))
        self.latent_dim = shapes[-1][0] * shapes[-1][1] * shapes[-1][2]
        self.fc1 = torch.nn.Linear(self.latent_dim + len(cfg["prop_rows"]), cfg["hidden"])
        self.fc2 = torch.nn.Linear(cfg["hidden"], NSCAN)
        self.register_buffer("prop_index", torch.tensor(cfg["prop_rows"], dtype=torch.long), persistent=False)

    def latent(self, depth: torch.Tensor) -> torch.Tensor:
        x = preprocess(depth, self.cfg["near"], self.cfg["far"]).unsqueeze(1)
        for conv in self.convs:
            x = torch.nn.functional.silu(conv(x))
        return x.flatten(1)

    def forward(self, depth: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
        """depth [N, H, W], obs [N, obs_dim] -> est [N, 117]"""
        z = torch.cat([self.latent(depth), obs[:, self.prop_index]], dim=1)
        return self.fc2(torch.nn.functional.silu(self.fc1(z)))

    def assemble(self, obs: torch.Tensor, est: torch.Tensor) -> torch.Tensor:
        """obs with the scan rows replaced by est: obs_out as torch ops"""
        r0 = self.cfg["scan_row0"]
        return torch.cat([obs[:, :r0], est, obs[:, r0 + NSCAN:]], dim=1)

    def layers(self):
        return list(self.convs) + [self.fc1, self.fc2]

    @torch.no_grad()
    def pack(self) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        """-> (weights, biases) in the kernel's layouts, fp32, one entry per layer of the net (the convs, fc1, fc2)"""
        ws = [pack_conv(c.weight.float()) for c in self.convs]
        bs = [c.bias.detach().float().clone() for c in self.convs]
        for lin in (self.fc1, self.fc2):
            w, b = acting.pack_linear(lin.weight, lin.bias)
            ws.append(w); bs.append(b)
        return ws, bs

    @torch.no_grad()
    def unpack(self, ws: Sequence[torch.Tensor], bs: Sequence[torch.Tensor]) -> None:
        """the inverse of pack(): fills this module's parameters"""
        n = len(self.convs)
        for l, c in enumerate(self.convs):
            c.weight.copy_(unpack_conv(ws[l], c.out_channels, c.in_channels, c.kernel_size[0])); c.bias.copy_(bs[l])
        for lin, w, b in ((self.fc1, ws[n], bs[n]), (self.fc2, ws[n + 1], bs[n + 1])):
            lin.weight.copy_(unpack_linear(w, lin.out_features, lin.in_features)); lin.bias.copy_(b[:lin.out_features])

    def save(self, path: str) -> None:
        """.npz: the config (JSON) and every parameter"""
        arrays = {k: v.detach().cpu().numpy() for k, v in self.state_dict().items()}
        np.savez(path, config=np.array(json.dumps(self.cfg)), **arrays)

    @classmethod
    def load(cls, path: str) -> "ScanEstimator":
        with np.load(path, allow_pickle=False) as z:
            est = cls(json.loads(str(z["config"])))
            est.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files if k != "config"})
        return est


def scan_target(env) -> torch.Tensor:
    """[N, 117]: scan_z[e] - min(scan_z[e]), the noise-free value of the observation's scan rows (heights above the lowest scan point)"""
    z = env.buffers["scan_z"]
    return z - z.min(dim=1, keepdim=True).values


class StudentPerception(_sidelib.Handle):
    """The estimator of one Joystick with a depth camera, as libpgtt_perceive.so runs it: owns the handle, the packed weights, `latent` [N, F],
    `est` [N, 117] and `obs` [N, obs_dim] (the obs_out buffer: the env's observation with the scan rows replaced by est).
    Runs on the env's device and current stream; reads env.depth and env.buffers["obs_state"] and writes nothing but its own tensors."""
    _prefix, _check = "pgtt_perceive", staticmethod(check)

    def __init__(self, env, estimator: ScanEstimator):
        if env.depth is None:
            raise ValueError("StudentPerception needs an env with a depth camera: Joystick(..., depth=dict(...))")
        cfg = estimator.cfg
        cam = env.depth_camera
        if (cfg["height"], cfg["width"]) != (cam.height, cam.width) or cfg["obs_dim"] != env.observation_size["state"]:
            raise ValueError(f"the estimator is for {cfg['height']}x{cfg['width']} images and {cfg['obs_dim']} observation rows; the env has "
                             f"{cam.height}x{cam.width} and {env.observation_size['state']}")
        self.env, self.cfg = env, cfg
        self._lib = lib()
        self.config = config_struct(cfg)
        self._h = C.c_void_p()
        check(self._lib.pgtt_perceive_create(C.byref(self.config), env.device.index or 0, env.num_envs, C.byref(self._h)))
        dev, n = env.device, env.num_envs
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)
        self.latent, self.est, self.obs = z(n, estimator.latent_dim), z(n, NSCAN), z(n, cfg["obs_dim"])
        nc = len(cfg["conv"])
        self._layers = list(range(nc)) + [3, 4]
        self._w = [z(self._lib.pgtt_perceive_packed_floats(C.byref(self.config), l)) for l in self._layers]
        self._b = [z(co) for co, _, _ in cfg["conv"]] + [z(cfg["hidden"]), z(OUT_PAD)]
        assert self._lib.pgtt_perceive_latent_dim(C.byref(self.config)) == estimator.latent_dim
        self.load(estimator)
        self.bind()

    def bind(self) -> None:
        """(re)bind: the env's image and observation, this object's weights and outputs"""
        b = PgttPerceiveBuffers()
        b.depth, b.obs = self.env.depth.data_ptr(), self.env.buffers["obs_state"].data_ptr()
        for l, w, bias in zip(self._layers, self._w, self._b):
            b.w[l], b.b[l] = w.data_ptr(), bias.data_ptr()
        b.latent, b.est, b.obs_out = self.latent.data_ptr(), self.est.data_ptr(), self.obs.data_ptr()
        check(self._lib.pgtt_perceive_bind(self._h, C.byref(b)))

    @torch.no_grad()
    def load(self, estimator: ScanEstimator) -> None:
        """repack the estimator's parameters in place: a captured graph keeps reading the same addresses"""
        ws, bs = estimator.pack()
        for dst, src in zip(self._w + self._b, ws + bs):
            assert dst.numel() == src.numel(), (dst.shape, src.shape)
            dst.copy_(src.to(dst.device))

    def tick(self) -> torch.Tensor:
        """one estimate for every env: two launches on the env's current stream, no synchronisation"""
        check(self._lib.pgtt_perceive(self._h, torch.cuda.current_stream(self.env.device).cuda_stream))
        return self.obs

    def set_terrain(self, terrain) -> None:
        raise AttributeError("StudentPerception has no terrain")
