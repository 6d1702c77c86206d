"""Teacher-student policy distillation on perceived observations: a privileged teacher policy that reads the true height scan
labels the states of a roll-out, and a student policy that reads only what the sensors deliver - env.elevation_obs, env.elevation_filled_obs,
env.student_obs or any [N, obs_dim] tensor - learns to imitate it (DAgger: the student drives a growing share of the envs, the teacher labels all).

    student = distill(env, "policy177", DistillConfig(iterations=50), obs="elevation")
    student.save("student_policy.npz")          # the layout of ppo.export_policy_npz: policy.PolicyMLP, FusedActor.load and evaluate.py read it

One roll-out step is two launches of pgtt_policy_act (acting.FusedActor: the teacher on the true observation, deterministic, its raw head kept as
the label; the student on the perceived one) around env.step; one update is hand-written HIP on one stream - pgtt_learn_gather_rows, four
pgtt_learn_linear_forward, pgtt_learn_distill_loss (KL(teacher || student) of the two heads and its gradient), per layer pgtt_ppo_linear_backward
and pgtt_learn_linear_backward_data, pgtt_learn_clip_adam - replayed from one graph after two eager calls.  The student keeps the teacher's
normaliser.  GPU only, one process: there is no CPU form, no fall-back to PyTorch ops and no data parallel.

With DistillConfig(memory=R), R > 0, the student is a recurrent_policy.RecurrentPolicy - the teacher's layers, a GRU memory of R
values per env and a read-out of it added to the head - acted by recurrent_policy.RecurrentActor (pgtt_learn_recurrent_act) and trained by
recurrent_policy.SequenceLearner (truncated BPTT over whole unrolls); save() then writes the recurrent layout.  memory = 0 is the path above.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import abi, learn, native
from .learn import FlatParams, PgttLearnAdamArgs, _Layer, _stream
from .policy import PolicyMLP, _DIR as POLICY_DIR

OBS_NAMES = {"elevation": "elevation_obs", "elevation_filled": "elevation_filled_obs", "student": "student_obs"}


class DistillError(RuntimeError):
    pass


@dataclass
class DistillConfig:
    iterations: int = 20
    unroll_length: int = 20
    epochs: int = 1                          # passes over an iteration's rows
    batch_size: int = 1024                   # minibatch rows
    learning_rate: float = 1e-4
    max_grad_norm: float = 1.0
    beta: Tuple[float, float] = (1.0, 0.0)   # share of the envs the teacher drives in the first and the last iteration, linear in between
    student_noise: bool = False              # False: the student acts on its mean
    seed: int = 0
    memory: int = 0                          # R > 0: the student is a recurrent_policy.RecurrentPolicy with a GRU memory of R values

    def __post_init__(self):
        _check_memory(self)


def _check_memory(cfg) -> None:
    if cfg.memory == 0:
        return
    if not (isinstance(cfg.memory, int) and 16 <= cfg.memory <= 256 and cfg.memory % 16 == 0):
        raise DistillError(f"memory must be 0 (a feed-forward student) or a multiple of 16 in [16, 256], not {cfg.memory!r}")
    if cfg.student_noise:
        raise DistillError("student_noise=True with a memory is not built: the recurrent actor is deterministic (no draws, no log-probabilities)")


def _refuse(env) -> None:
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise DistillError(f"distillation runs in one process: this process group has {dist.get_world_size()} ranks and data parallel is not built")
    if torch.device(env.device).type != "cuda":
        raise DistillError("distillation runs on a GPU only: the env is on a CPU device and there is no CPU form")
    if getattr(env, "curriculum", None) is not None:
        raise DistillError("distillation on an env with a terrain curriculum is not built: the curriculum's restart has to follow the record")


def load_teacher(teacher: Union[PolicyMLP, str], device) -> PolicyMLP:
    if isinstance(teacher, PolicyMLP):
        return teacher.to(device)
    p = teacher if os.path.exists(teacher) else os.path.join(POLICY_DIR, str(teacher).replace(".npz", "") + ".npz")
    return PolicyMLP(p).to(device)


def perceived(env, obs) -> torch.Tensor:
    """the tensor the student reads: one of the env's perceived observations by name, or the caller's own"""
    if isinstance(obs, torch.Tensor):
        return obs
    if obs not in OBS_NAMES:
        raise DistillError(f"obs must be one of {sorted(OBS_NAMES)} or a tensor, not {obs!r}")
    t = getattr(env, OBS_NAMES[obs], None)
    if t is None:
        raise DistillError(f"obs={obs!r}: the env has no {OBS_NAMES[obs]} (build it with the sensor that delivers it)")
    return t


def student_net(teacher: PolicyMLP, device) -> nn.Sequential:
    """the teacher's layers as a module of its own: Linear, SiLU, ..., Linear"""
    mods: List[nn.Module] = []
    for i, lin in enumerate(teacher.layers):
        new = nn.Linear(lin.in_features, lin.out_features)
        with torch.no_grad():
            new.weight.copy_(lin.weight); new.bias.copy_(lin.bias)
        mods.append(new)
        if i + 1 < len(teacher.layers):
            mods.append(nn.SiLU())
    return nn.Sequential(*mods).to(device)


class Rollout:
    """T steps of the env under a mix of the two drivers.  Per step: the teacher acts deterministically on the true observation (nothing stored, its
    raw head into `head`), `head` goes to row t of `labels` through the student's device-side row counter, the student acts on `obs` (its storage's
    "obs" rows record what it saw), the env gets the teacher's tanh(loc) where `mask` is set and the student's action elsewhere, the student
    records.  No host read-back.  The steps are plain launches; that env.step with its sensors' ticks, captured in a graph, replays the eager bits
    is held by tests/test_gpu_stack.py (test_the_captured_step_is_the_eager_step)."""

    def __init__(self, env, teacher: PolicyMLP, obs: torch.Tensor, T: int, seed: int = 0, student_noise: bool = False, memory: int = 0):
        """memory = R > 0: the student is a recurrent_policy.RecurrentActor (the caller loads its weights); its storage has "obs", "mem0" and
        "clear" rows, written at the host's step index, and the labels go to the same row"""
        from .acting import FusedActor
        _refuse(env)
        self.env, self.T, self.noise, self.memory = env, int(T), bool(student_noise), int(memory)
        dev, n = env.device, env.num_envs
        self.teacher = FusedActor(env, 1, seed=seed)
        layers = [(m.weight, m.bias) for m in teacher.layers]
        self.teacher.load(layers, teacher.mean, teacher.std)
        if self.memory:
            from .recurrent_policy import RecurrentActor
            self.student = RecurrentActor(env, self.T, self.memory, obs=obs)
        else:
            self.student = FusedActor(env, self.T, seed=seed + 1, obs=obs)
            self.student.load(layers, teacher.mean, teacher.std)
        self.head = torch.zeros(n, 2 * abi.NU, device=dev)
        self.labels = torch.zeros(self.T, n, 2 * abi.NU, device=dev)
        self.mask = torch.ones(n, dtype=torch.bool, device=dev)
        self.action = torch.zeros(n, abi.NU, device=dev)
        self._last = torch.tensor([self.T - 1], dtype=torch.int64, device=dev)

    @torch.no_grad()
    def draw_mask(self, beta: float, generator: torch.Generator) -> float:
        """the teacher drives round(beta N) envs, drawn without replacement from `generator` (on the env's device); -> the share it drives"""
        n = self.env.num_envs
        k = max(0, min(n, int(round(float(beta) * n))))
        perm = torch.randperm(n, device=self.mask.device, generator=generator)
        self.mask.zero_()
        self.mask[perm[:k]] = True
        return k / n

    @torch.no_grad()
    def step(self) -> None:
        env = self.env
        self.teacher.act(deterministic=True, head=self.head, store=False)
        row = torch.minimum(self.student.counters[:1], self._last)          # a caller that ran past T without a rewind overwrites the last row
        self.labels.view(self.T, -1).index_copy_(0, row, self.head.view(1, -1))
        self.student.act(deterministic=not self.noise)
        torch.where(self.mask[:, None], self.teacher.action, self.student.action, out=self.action)
        env.step(self.action)
        self.student.record()

    @torch.no_grad()
    def step_recurrent(self, t: int) -> None:
        """step() under a recurrent student: row t of the labels and of the student's storage by the host's index; the student's memory follows
        every env, whoever drives it"""
        self.teacher.act(deterministic=True, head=self.head, store=False)
        self.labels[t].copy_(self.head)
        self.student.act(t)
        torch.where(self.mask[:, None], self.teacher.action, self.student.action, out=self.action)
        self.env.step(self.action)

    def rollout(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (what the student saw [T, N, obs_dim], the teacher's heads [T, N, 24]): the storage itself, overwritten by the next roll-out"""
        if self.memory:
            for t in range(self.T):
                self.step_recurrent(t)
            return self.student.storage["obs"], self.labels
        self.student.rewind()
        for _ in range(self.T):
            self.step()
        return self.student.storage["obs"], self.labels


class DistillLearner:
    """One update over a minibatch of the flat (observation, label) rows, on the current stream: gather, four forwards, the distillation loss, per
    layer from the top the weight / bias gradient (libpgtt.so, straight into the flat gradient) and the data gradient, clip + Adam.  After two
    eager calls it is one captured graph without parallel branches.  `mean` / `std` are read in place; `loss2` = (KL, action error) of the call."""

    def __init__(self, net: nn.Sequential, flat: FlatParams, mean: torch.Tensor, std: torch.Tensor, obs_rows: torch.Tensor, label_rows: torch.Tensor,
                 mb: int, cfg: DistillConfig, use_graph: bool = True):
        dev = obs_rows.device
        if dev.type != "cuda":
            raise DistillError("the distillation learner runs on a GPU only; there is no CPU form")
        assert obs_rows.is_contiguous() and label_rows.is_contiguous() and obs_rows.shape[0] == label_rows.shape[0]
        assert obs_rows.dtype == label_rows.dtype == torch.float32 and mean.is_contiguous() and std.is_contiguous()
        self.net, self.flat, self.mean, self.std, self.obs_rows, self.label_rows, self.cfg, self.mb, self.dev = net, flat, mean, std, obs_rows, label_rows, cfg, int(mb), dev
        self.lib, self.plib = learn.lib(), native.lib()
        self.rows, self.od, self.hd = obs_rows.shape[0], obs_rows.shape[1], label_rows.shape[1]
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.idx = torch.zeros(mb, dtype=torch.long, device=dev)
        self.x, self.y = z(mb, self.od), z(mb, self.hd)
        self.loss2, self.norm = z(2), z(1)
        self.partial = z(2 * ((mb + 63) // 64))
        self.adam_partial = z(self.lib.pgtt_learn_adam_partials(flat.numel))
        self.use_graph, self.graph, self.calls = use_graph, None, 0
        lins = [m for m in net if isinstance(m, nn.Linear)]
        assert lins[0].in_features == self.od and lins[-1].out_features == self.hd and self.hd % 2 == 0
        self.layers, x, scratch = [], self.x, 1
        for i, lin in enumerate(lins):
            L = _Layer()
            L.w, L.b, L.M, L.N, L.act = lin.weight, lin.bias, lin.in_features, lin.out_features, int(i + 1 < len(lins))
            L.x = x
            L.y, L.z, L.dy = z(mb, L.N), (z(mb, L.N) if L.act else None), z(mb, L.N)
            L.dw, L.db = flat.grad_of(lin.weight), flat.grad_of(lin.bias)
            tiles = ((L.M + 63) // 64) * ((L.N + 63) // 64)
            L.S = max(1, min(64, int(os.environ.get("PGTT_PPO_SPLITK", "768")) // tiles, mb // 16))      # as learn.NativeLearner
            scratch = max(scratch, L.S * (L.N * L.M + L.N))
            x = L.y
            self.layers.append(L)
        self.lb_partial = z(scratch)

    def _ptr(self, t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _forward_backward(self):
        L, P, st, mb, p, check = self.lib, self.plib, _stream(self.dev), self.mb, self._ptr, learn.check
        check(L.pgtt_learn_gather_rows(p(self.idx), p(self.obs_rows), p(self.label_rows), p(self.mean), p(self.std), mb, self.rows, self.od, self.hd,
                                       p(self.x), p(self.y), st))
        for l in self.layers:
            check(L.pgtt_learn_linear_forward(p(l.x), p(l.w), p(l.b), mb, l.M, l.N, l.act, p(l.y), p(l.z), st))
        top = self.layers[-1]
        check(L.pgtt_learn_distill_loss(p(top.y), p(self.y), mb, self.hd // 2, p(self.partial), p(self.loss2), p(top.dy), st))
        for i in range(len(self.layers) - 1, -1, -1):
            l = self.layers[i]
            native.check(P.pgtt_ppo_linear_backward(p(l.x), p(l.dy), C.c_int(mb), C.c_int(l.M), C.c_int(l.N), C.c_int(l.S), p(self.lb_partial),
                                                    p(l.dw), p(l.db), st))
            if i > 0:                       # the first layer's input needs no gradient
                check(L.pgtt_learn_linear_backward_data(p(l.dy), p(l.w), p(self.layers[i - 1].z), mb, l.M, l.N, p(self.layers[i - 1].dy), st))

    def _apply(self):
        f, cfg = self.flat, self.cfg
        a = PgttLearnAdamArgs()
        a.p, a.g, a.m, a.v, a.t = f.flat.data_ptr(), f.grad.data_ptr(), f.m.data_ptr(), f.v.data_ptr(), f.t.data_ptr()
        a.partial, a.norm_1, a.P = self.adam_partial.data_ptr(), self.norm.data_ptr(), f.numel
        a.lr, a.beta1, a.beta2, a.eps = float(cfg.learning_rate), 0.9, 0.999, 1e-8
        a.max_norm, a.grad_scale = float(cfg.max_grad_norm), 1.0
        learn.check(self.lib.pgtt_learn_clip_adam(C.byref(a), _stream(self.dev)))

    def _eager(self):
        self._forward_backward()
        self._apply()

    @torch.no_grad()
    def update(self, idx: torch.Tensor) -> torch.Tensor:
        self.idx.copy_(idx)
        self.calls += 1
        if self.use_graph and self.graph is None and self.calls == 3:        # two eager updates warmed everything up
            try:
                torch.cuda.synchronize(self.dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._eager()
                self.graph = g
            except Exception as exc:
                print(f"[distill] HIP graph capture of the update failed ({exc}); running eagerly")
                self.use_graph = False
        if self.graph is not None:
            self.graph.replay()
        else:
            self._eager()
        return self.loss2


class Distilled:
    """what distill() returns: the student's arrays in the layout of ppo.export_policy_npz (mean, std, w{i} as [in, out], b{i}), the live
    network, and the per-iteration history; with a memory, the recurrent layout (recurrent_policy.RecurrentPolicy.arrays) and `actor`, the live
    RecurrentActor with the final weights loaded"""
    actor = None

    def __init__(self, net: nn.Module, mean: torch.Tensor, std: torch.Tensor, history: List[Dict[str, float]]):
        self.net, self.history = net, history
        if hasattr(net, "gru_w_ih"):            # a recurrent_policy.RecurrentPolicy: its own layout, the feed-forward keys plus gru_* and mem_w
            self.arrays: Dict[str, np.ndarray] = net.arrays()
            return
        self.arrays: Dict[str, np.ndarray] = {"mean": mean.detach().float().cpu().numpy(), "std": std.detach().float().cpu().numpy()}
        for i, lin in enumerate(m for m in net if isinstance(m, nn.Linear)):
            self.arrays[f"w{i}"] = lin.weight.detach().float().cpu().numpy().T.copy()
            self.arrays[f"b{i}"] = lin.bias.detach().float().cpu().numpy().copy()

    def save(self, path: str) -> None:
        np.savez_compressed(path, **self.arrays)


def distill(env, teacher: Union[PolicyMLP, str], cfg: DistillConfig, obs: Union[str, torch.Tensor] = "elevation",
            progress_fn: Optional[Callable[[int, Dict[str, float]], Optional[bool]]] = None) -> Distilled:
    """DAgger from `teacher` into a student that reads `obs`; the env is stepped from the state it is in (reset it first).  Per iteration:
    the drive mask is redrawn, T steps are rolled out, `epochs` passes of minibatch updates run over the T N rows, the new weights are packed
    into the student's acting kernel.  progress_fn(iteration, metrics) is called once per iteration; a true return stops the run."""
    _check_memory(cfg)
    _refuse(env)
    dev = env.device
    teacher = load_teacher(teacher, dev)
    if teacher.mean.shape[0] != env.observation_size["state"]:
        raise DistillError(f"the teacher reads {teacher.mean.shape[0]} observations, the env gives {env.observation_size['state']}")
    seen = perceived(env, obs)
    T, n = int(cfg.unroll_length), env.num_envs
    if cfg.memory:
        return _distill_recurrent(env, teacher, cfg, seen, progress_fn)
    roll = Rollout(env, teacher, seen, T, seed=cfg.seed, student_noise=cfg.student_noise)
    net = student_net(teacher, dev)
    flat = FlatParams(net)
    mean, std = teacher.mean.detach().clone().contiguous(), teacher.std.detach().clone().contiguous()
    rows = T * n
    mb = min(int(cfg.batch_size), rows)
    learner = DistillLearner(net, flat, mean, std, roll.student.storage["obs"].view(rows, -1), roll.labels.view(rows, -1), mb, cfg)
    gen = torch.Generator(device=dev).manual_seed(int(cfg.seed))
    b0, b1 = (float(v) for v in cfg.beta)
    acc = torch.zeros(2, device=dev)
    history: List[Dict[str, float]] = []
    t_start = time.time()
    for it in range(int(cfg.iterations)):
        t0 = time.time()
        beta = b0 + (b1 - b0) * (it / max(1, int(cfg.iterations) - 1))
        share = roll.draw_mask(beta, gen)
        roll.rollout()
        acc.zero_()
        updates = 0
        for _ in range(int(cfg.epochs)):
            perm = torch.randperm(rows, device=dev, generator=gen)
            for k in range(rows // mb):
                acc += learner.update(perm[k * mb:(k + 1) * mb])
                updates += 1
        roll.student.load_sequential(net, mean, std)
        kl, act = (acc / max(1, updates)).tolist()                            # the iteration's one host read
        dt = time.time() - t0
        m = {"kl": kl, "action_error": act, "drive_share": share, "beta": beta, "updates": float(updates), "grad_norm": float(learner.norm),
             "env_steps_per_s": rows / dt, "seconds": time.time() - t_start}
        history.append(m)
        if progress_fn is not None and progress_fn(it, m):
            break
    return Distilled(net, mean, std, history)


def _distill_recurrent(env, teacher: PolicyMLP, cfg: DistillConfig, seen: torch.Tensor, progress_fn) -> Distilled:
    """distill() with cfg.memory = R > 0: the student is a RecurrentPolicy that starts as the teacher (W_m = 0), acts through a RecurrentActor and
    learns by SequenceLearner over minibatches of max(1, batch_size // T) whole unrolls.  Its memory is cleared here once and by `done` afterwards;
    it carries across iterations: an unroll's m_init is the roll-out's stored mem0 of row 0."""
    from .recurrent_policy import RecurrentPolicy, SequenceLearner
    dev, T, n = env.device, int(cfg.unroll_length), env.num_envs
    roll = Rollout(env, teacher, seen, T, seed=cfg.seed, memory=cfg.memory)
    policy = RecurrentPolicy.from_teacher(teacher, cfg.memory, cfg.seed).to(dev)
    flat = FlatParams(policy)
    roll.student.load(policy)
    roll.student.reset_memory()
    S = roll.student.storage
    b_env = min(n, max(1, int(cfg.batch_size) // T))
    learner = SequenceLearner(policy, flat, S["obs"], roll.labels, S["mem0"], S["clear"], b_env, cfg)
    gen = torch.Generator(device=dev).manual_seed(int(cfg.seed))
    b0, b1 = (float(v) for v in cfg.beta)
    acc = torch.zeros(2, device=dev)
    history: List[Dict[str, float]] = []
    t_start = time.time()
    for it in range(int(cfg.iterations)):
        t0 = time.time()
        beta = b0 + (b1 - b0) * (it / max(1, int(cfg.iterations) - 1))
        share = roll.draw_mask(beta, gen)
        roll.rollout()
        acc.zero_()
        updates = 0
        for _ in range(int(cfg.epochs)):
            perm = torch.randperm(n, device=dev, generator=gen)
            for k in range(n // b_env):
                acc += learner.update(perm[k * b_env:(k + 1) * b_env])
                updates += 1
        roll.student.load(policy)
        kl, act = (acc / max(1, updates)).tolist()                            # the iteration's one host read
        dt = time.time() - t0
        m = {"kl": kl, "action_error": act, "drive_share": share, "beta": beta, "updates": float(updates), "grad_norm": float(learner.norm),
             "env_steps_per_s": T * n / dt, "seconds": time.time() - t_start}
        history.append(m)
        if progress_fn is not None and progress_fn(it, m):
            break
    out = Distilled(policy, policy.mean, policy.std, history)
    out.actor = roll.student
    return out
