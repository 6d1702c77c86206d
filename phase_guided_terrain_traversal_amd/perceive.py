"""Student perception: the 117 height-scan rows of the observation estimated from the onboard depth image and the proprioceptive rows
(libpgtt_perceive.so, include/pgtt_perceive.h), so that a policy trained on the privileged scan acts on what a robot can sense.

    est = ScanEstimator(config(env.method))          # torch: Conv2d / SiLU / Linear - what train_student.py differentiates
    sp = StudentPerception(env, est)                 # the same function as two HIP launches; sp.obs is obs with the scan rows replaced
    sp.tick(); sp.est; sp.obs
    sp.load(est)                                     # repack in place after an optimiser step

config(memory=R) puts a GRU cell of R values per env between the hidden layer and the scan rows (the recurrent form of pgtt_perceive.h):
ScanEstimator.step / .sequence in torch, StudentPerception.mem and tick(clear_mask, clear_all, use_done) on the device.

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
MAX_MEMORY = 256
NSCAN = abi.NSCAN
SCAN_ROW0 = {"pgtt": 38, "baseline": 30}           # the scan rows sit between phase / joint_vel and gait_freq / last_act
# the scan grid is 13 rows (x, ahead first) by 9 columns: the bands train_student.py reports
BANDS = {"ahead": slice(0, 6 * abi.SCAN_W), "under": slice(6 * abi.SCAN_W, 7 * abi.SCAN_W), "behind": slice(7 * abi.SCAN_W, NSCAN)}


def config(method: str = "pgtt", memory: int = 0, **overrides) -> Dict:
    """the default net for the task definition `method`: depth.DEFAULTS' 48 x 64 image -> 16 ch k5 s2 -> 32 ch k3 s2 -> 32 ch k3 s2 (F = 768), the
    proprioceptive input = every observation row except the scan rows (54 for the PGTT task), hidden 512, memory 0 (feed-forward; R > 0: a GRU cell
    of R values per env behind the hidden layer).  A config dict without "memory" means 0, and memory = 0 leaves the key out: a feed-forward
    student's saved config is what it always was."""
    od, row0 = abi.obs_dims(method)[0], SCAN_ROW0[method]
    c = dict(height=_depth.DEFAULTS["height"], width=_depth.DEFAULTS["width"], near=_depth.DEFAULTS["near"], far=_depth.DEFAULTS["far"],
             conv=[(16, 5, 2), (32, 3, 2), (32, 3, 2)], prop_rows=[r for r in range(od) if not row0 <= r < row0 + NSCAN], hidden=512,
             obs_dim=od, scan_row0=row0)
    if memory:
        c["memory"] = memory
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


class PgttPerceiveMemory(C.Structure):
    _fields_ = [("memory", i32), ("w_ih", C.c_void_p), ("w_hh", C.c_void_p), ("w_out", C.c_void_p), ("b_ih", C.c_void_p), ("b_hh", C.c_void_p),
                ("b_out", C.c_void_p), ("done", C.c_void_p), ("mem", C.c_void_p)]


assert C.sizeof(PgttPerceiveConfig) == 328 and C.sizeof(PgttPerceiveBuffers) == 120 and C.sizeof(PgttPerceiveMemory) == 72


class PerceiveError(RuntimeError):
    pass


vp, cp = C.c_void_p, C.POINTER(PgttPerceiveConfig)
SIDE = _sidelib.SideLib("perceive", PerceiveError, {
    "pgtt_perceive_check": (None, [cp]), "pgtt_perceive_latent_dim": (None, [cp]), "pgtt_perceive_packed_floats": (None, [cp, C.c_int]),
    "pgtt_perceive_create": (None, [cp, C.c_int, C.c_int, C.POINTER(vp)]), "pgtt_perceive_destroy": (None, [vp]),
    "pgtt_perceive_bind": (None, [vp, C.POINTER(PgttPerceiveBuffers)]), "pgtt_perceive": (None, [vp, vp]),
    "pgtt_perceive_memory_check": (None, [cp, C.c_int]), "pgtt_perceive_memory_packed_floats": (None, [cp, C.c_int, C.c_int]),
    "pgtt_perceive_set_memory": (None, [vp, C.POINTER(PgttPerceiveMemory)]), "pgtt_perceive_recurrent": (None, [vp, vp, C.c_int, C.c_int, vp]),
}, {"pgtt_perceive_sizeof_config": PgttPerceiveConfig, "pgtt_perceive_sizeof_buffers": PgttPerceiveBuffers,
    "pgtt_perceive_sizeof_memory": PgttPerceiveMemory})
LIB_PATH, EXPORTS, lib, check, build_info = SIDE.path, SIDE.exports, SIDE.lib, SIDE.check, SIDE.build_info


def conv_shapes(cfg: Dict) -> List[Tuple[int, int, int]]:
    """[(channels, height, width)] of the input and of every conv's output; no padding, no dilation.  An output is 0 x 0 where the kernel does
    not fit or the stride is not positive: check_config refuses such a layer"""
    shapes = [(1, int(cfg["height"]), int(cfg["width"]))]
    for co, k, s in cfg["conv"]:
        _, h, w = shapes[-1]
        shapes.append((int(co), (h - k) // s + 1 if h >= k and s > 0 else 0, (w - k) // s + 1 if w >= k and s > 0 else 0))
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
    m = cfg.get("memory", 0)
    if m != 0 and (m != int(m) or m % 16 or not 16 <= m <= MAX_MEMORY):
        no("memory must be 0 or a multiple of 16 in [16, 256]")


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
        if "memory" in cfg:
            cfg["memory"] = int(cfg["memory"])
        self.cfg = cfg
        self.memory = cfg.get("memory", 0)
        shapes = conv_shapes(cfg)
        self.convs = torch.nn.ModuleList(torch.nn.Conv2d(shapes[l][0], co, k, s) for l, (co, k, s) in enumerate(cfg["conv"]))
        self.latent_dim = shapes[-1][0] * shapes[-1][1] * shapes[-1][2]
        self.fc1 = torch.nn.Linear(self.latent_dim + len(cfg["prop_rows"]), cfg["hidden"])
        if self.memory:
            self.gru = torch.nn.GRUCell(cfg["hidden"], self.memory)
        self.fc2 = torch.nn.Linear(self.memory or cfg["hidden"], NSCAN)
        self.register_buffer("prop_index", torch.tensor(cfg["prop_rows"], dtype=torch.long), persistent=False)

    def latent(self, depth: torch.Tensor) -> torch.Tensor:
        x = preprocess(depth, self.cfg["near"], self.cfg["far"]).unsqueeze(1)
        for conv in self.convs:
            x = torch.nn.functional.silu(conv(x))
        return x.flatten(1)

    def forward(self, depth: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
        """depth [N, H, W], obs [N, obs_dim] -> est [N, 117]"""
        if self.memory:
            raise RuntimeError(f"this ScanEstimator is recurrent (memory = {self.memory}): call step(depth, obs, mem) or sequence(...), "
                               "forward() has no memory to read")
        return self.fc2(self.hidden(depth, obs))

    def hidden(self, depth: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
        """h = silu(W1 z + b1) [N, hidden]"""
        z = torch.cat([self.latent(depth), obs[:, self.prop_index]], dim=1)
        return torch.nn.functional.silu(self.fc1(z))

    def step(self, depth: torch.Tensor, obs: torch.Tensor, mem: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """one recurrent tick: depth [N, H, W], obs [N, obs_dim], mem [N, R] -> (est [N, 117], mem1 [N, R])"""
        if not self.memory:
            raise RuntimeError("this ScanEstimator is feed-forward (memory = 0): call it, step() is the recurrent form's")
        m1 = self.gru(self.hidden(depth, obs), mem)
        return self.fc2(m1), m1

    def sequence(self, depth: torch.Tensor, obs: torch.Tensor, mem0: torch.Tensor, clear: Optional[torch.Tensor] = None,
                 detach_every: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """T ticks: depth [T, N, H, W], obs [T, N, obs_dim], mem0 [N, R], clear [T, N] (non-zero: the env's memory is zeroed before tick t)
        -> (est [T, N, 117], memT [N, R]).  The trunk and the hidden layer run once over all T N images.  detach_every = L > 0 cuts the
        gradient through the memory before ticks L, 2 L, ... (truncated back-propagation through time)."""
        if not self.memory:
            raise RuntimeError("this ScanEstimator is feed-forward (memory = 0): sequence() is the recurrent form's")
        T, N = depth.shape[:2]
        h = self.hidden(depth.flatten(0, 1), obs.flatten(0, 1)).view(T, N, -1)
        mem, ms = mem0, []
        for t in range(T):
            if detach_every and t and t % detach_every == 0:
                mem = mem.detach()
            if clear is not None:
                mem = torch.where(clear[t].bool()[:, None], torch.zeros_like(mem), mem)
            mem = self.gru(h[t], mem)
            ms.append(mem)
        return self.fc2(torch.stack(ms)), mem

    def assemble(self, obs: torch.Tensor, est: torch.Tensor) -> torch.Tensor:
        """obs with the scan rows replaced by est: obs_out as torch ops"""
        r0 = self.cfg["scan_row0"]
        return torch.cat([obs[:, :r0], est, obs[:, r0 + NSCAN:]], dim=1)

    def layers(self):
        """the modules with a `weight` and a `bias` (a recurrent estimator's GRUCell is not one: weight_ih / weight_hh)"""
        return list(self.convs) + [self.fc1, self.fc2]

    @torch.no_grad()
    def pack(self) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        """-> (weights, biases) in the kernel's layouts, fp32, one entry per layer of the net: the convs, fc1, fc2; a recurrent estimator's are
        the convs, fc1, w_ih / b_ih, w_hh / b_hh, w_out / b_out (PgttPerceiveMemory)"""
        ws = [pack_conv(c.weight.float()) for c in self.convs]
        bs = [c.bias.detach().float().clone() for c in self.convs]
        for w, b in self._linears():
            w, b = acting.pack_linear(w, b)
            ws.append(w); bs.append(b)
        return ws, bs

    def _linears(self):
        """[(weight, bias)] of the layers packed in the linear tile order"""
        if self.memory:
            return [(self.fc1.weight, self.fc1.bias), (self.gru.weight_ih, self.gru.bias_ih), (self.gru.weight_hh, self.gru.bias_hh),
                    (self.fc2.weight, self.fc2.bias)]
        return [(self.fc1.weight, self.fc1.bias), (self.fc2.weight, self.fc2.bias)]

    @torch.no_grad()
    def unpack(self, ws: Sequence[torch.Tensor], bs: Sequence[torch.Tensor]) -> None:
        """the inverse of pack(): fills this module's parameters"""
        n = len(self.convs)
        for l, c in enumerate(self.convs):
            c.weight.copy_(unpack_conv(ws[l], c.out_channels, c.in_channels, c.kernel_size[0])); c.bias.copy_(bs[l])
        for (weight, bias), w, b in zip(self._linears(), ws[n:], bs[n:]):
            weight.copy_(unpack_linear(w, weight.shape[0], weight.shape[1])); bias.copy_(b[:bias.shape[0]])

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
    `est` [N, 117] and `obs` [N, obs_dim] (the obs_out buffer: the env's observation with the scan rows replaced by est).  With a recurrent
    estimator also `mem` [N, R], zeros at creation: the GRU state, read and written by every tick and cleared by its arguments.
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
        self.memory, self.mem, self._mask = estimator.memory, None, None
        if self.memory:
            # layer 4 of the feed-forward form stays a zero buffer the recurrent call never reads; the cell's own layers follow it
            r = self.memory
            check(self._lib.pgtt_perceive_memory_check(C.byref(self.config), r))
            self._mw = [z(self._lib.pgtt_perceive_memory_packed_floats(C.byref(self.config), r, which)) for which in range(3)]
            self._mb = [z(3 * r), z(3 * r), z(OUT_PAD)]
            self.mem = z(n, r)
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
        if self.memory:
            check(self._lib.pgtt_perceive_set_memory(self._h, C.byref(self.memory_struct())))

    def memory_struct(self) -> PgttPerceiveMemory:
        """the recurrent form's pointers: this object's packed cell, its `mem` and the env's done flags (None when the env has none)"""
        m = PgttPerceiveMemory()
        m.memory = self.memory
        m.w_ih, m.w_hh, m.w_out = (w.data_ptr() for w in self._mw)
        m.b_ih, m.b_hh, m.b_out = (b.data_ptr() for b in self._mb)
        done = self.env.buffers.get("done")
        m.done = None if done is None else done.data_ptr()
        m.mem = self.mem.data_ptr()
        return m

    @torch.no_grad()
    def load(self, estimator: ScanEstimator) -> None:
        """repack the estimator's parameters in place: a captured graph keeps reading the same addresses"""
        ws, bs = estimator.pack()
        if estimator.memory != self.memory:
            raise ValueError(f"this StudentPerception was made for memory = {self.memory}, the estimator has {estimator.memory}")
        dw, db = (self._w[:-1] + self._mw, self._b[:-1] + self._mb) if self.memory else (self._w, self._b)
        for dst, src in zip(dw + db, ws + bs):
            assert dst.numel() == src.numel(), (dst.shape, src.shape)
            dst.copy_(src.to(dst.device))

    def tick(self, clear_mask: Optional[torch.Tensor] = None, clear_all: bool = False, use_done: bool = False) -> torch.Tensor:
        """one estimate for every env: two launches on the env's current stream, no synchronisation.  A recurrent estimator's tick reads and writes
        `mem`; before it does, the memory of the envs with clear_mask[e] != 0 ([N] uint8 / bool), of every env (clear_all) or of the envs whose done
        flag is set (use_done) reads as zero.  A feed-forward estimator has nothing to clear and refuses the arguments."""
        stream = torch.cuda.current_stream(self.env.device).cuda_stream
        if not self.memory:
            if clear_mask is not None or clear_all or use_done:
                raise ValueError("tick(clear_mask / clear_all / use_done) is the recurrent student's: this estimator has no memory")
            check(self._lib.pgtt_perceive(self._h, stream))
            return self.obs
        mp = None
        if clear_mask is not None:
            self._mask = clear_mask.to(self.env.device, torch.uint8).contiguous()      # kept alive until the next tick: the launch is asynchronous
            assert self._mask.shape == (self.env.num_envs,)
            mp = self._mask.data_ptr()
        check(self._lib.pgtt_perceive_recurrent(self._h, mp, int(bool(clear_all)), int(bool(use_done)), stream))
        return self.obs

    def set_terrain(self, terrain) -> None:
        raise AttributeError("StudentPerception has no terrain")
