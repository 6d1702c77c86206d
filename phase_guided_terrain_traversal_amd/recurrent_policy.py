"""The recurrent policy (include/pgtt_learn.h): the 171-512-256-128-24 policy MLP with a GRU memory of R values per env between its
last hidden layer and its head, head = W3 h3 + b3 + W_m m1.  With W_m = 0 it is the feed-forward policy, which is how a distilled student starts.

    policy = RecurrentPolicy.from_teacher(PolicyMLP(...), memory=64, seed=0)     # plain torch ops, CPU-capable: the evaluator and the CPU tests use it
    action, head, mem = policy.step(obs, mem, clear)                             # one acting step
    heads = policy.sequence(obs_TxBxod, m_init, clear_TxB)                       # the autograd form of a whole unroll
    actor = RecurrentActor(env, T, memory=64, obs=env.elevation_obs); actor.load(policy)
    actor.act(t)                                                                 # pgtt_learn_recurrent_act: hand-written HIP, storage row t
    actor.act(t, sample=True)                                                    # pgtt_learn_recurrent_act_sample: a draw, its u and logp rows
    learner = SequenceLearner(policy, FlatParams(policy), ...); learner.update(env_idx)      # one BPTT update, hand-written HIP on one stream

The file format is that of ppo.export_policy_npz (mean, std, w{i} as [in, out], b{i}) plus gru_w_ih [3R, 128], gru_w_hh [3R, R], gru_b_ih, gru_b_hh
and mem_w [24, R]; none of the new keys starts with "w", so policy.PolicyMLP still loads the feed-forward part of such a file.  RecurrentActor and
SequenceLearner run on a GPU only: there is no CPU form of them and no fall-back to PyTorch ops.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import abi, learn, native
from .learn import FlatParams, PgttLearnAdamArgs, PgttLearnRecurrentActArgs, PgttLearnRecurrentSampleArgs, _stream

MAX_MEMORY = 256
GRU_KEYS = ("gru_w_ih", "gru_w_hh", "gru_b_ih", "gru_b_hh", "mem_w")


def memory_ok(memory) -> bool:
    """R is a multiple of 16 in [16, 256] (PGTT_LEARN_MAX_MEMORY)"""
    return isinstance(memory, int) and 16 <= memory <= MAX_MEMORY and memory % 16 == 0


class RecurrentPolicy(nn.Module):
    def __init__(self, dims=(171, 512, 256, 128, 24), memory: int = 64):
        super().__init__()
        if not memory_ok(memory):
            raise ValueError(f"memory must be a multiple of 16 in [16, {MAX_MEMORY}], not {memory!r}")
        assert len(dims) == 5 and dims[3] % 16 == 0
        self.dims, self.memory = tuple(int(d) for d in dims), int(memory)
        R, H = self.memory, self.dims[3]
        self.register_buffer("mean", torch.zeros(self.dims[0]))
        self.register_buffer("std", torch.ones(self.dims[0]))
        self.layers = nn.ModuleList(nn.Linear(self.dims[i], self.dims[i + 1]) for i in range(4))
        self.gru_w_ih, self.gru_w_hh = nn.Parameter(torch.zeros(3 * R, H)), nn.Parameter(torch.zeros(3 * R, R))
        self.gru_b_ih, self.gru_b_hh = nn.Parameter(torch.zeros(3 * R)), nn.Parameter(torch.zeros(3 * R))
        self.mem_w = nn.Parameter(torch.zeros(self.dims[4], R))

    def tensors(self) -> List[nn.Parameter]:
        """the thirteen trained tensors in the order w0, b0, .., w3, b3, gru_w_ih, gru_w_hh, gru_b_ih, gru_b_hh, mem_w"""
        return [t for lin in self.layers for t in (lin.weight, lin.bias)] + [getattr(self, k) for k in GRU_KEYS]

    @classmethod
    def from_teacher(cls, teacher, memory: int = 64, seed: int = 0) -> "RecurrentPolicy":
        """the initial state of a distilled student: the teacher's layers and statistics, torch's GRUCell initialisation under `seed`, W_m = 0"""
        lins = list(teacher.layers)
        dims = (lins[0].in_features,) + tuple(l.out_features for l in lins)
        pi = cls(dims, memory)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            cell = nn.GRUCell(dims[3], memory)
        with torch.no_grad():
            pi.mean.copy_(teacher.mean); pi.std.copy_(teacher.std)
            for new, old in zip(pi.layers, lins):
                new.weight.copy_(old.weight); new.bias.copy_(old.bias)
            pi.gru_w_ih.copy_(cell.weight_ih); pi.gru_w_hh.copy_(cell.weight_hh)
            pi.gru_b_ih.copy_(cell.bias_ih); pi.gru_b_hh.copy_(cell.bias_hh)
        return pi.to(teacher.mean.device)

    def arrays(self) -> Dict[str, np.ndarray]:
        a = {"mean": self.mean.detach().float().cpu().numpy(), "std": self.std.detach().float().cpu().numpy()}
        for i, lin in enumerate(self.layers):
            a[f"w{i}"] = lin.weight.detach().float().cpu().numpy().T.copy()
            a[f"b{i}"] = lin.bias.detach().float().cpu().numpy().copy()
        for k in GRU_KEYS:
            a[k] = getattr(self, k).detach().float().cpu().numpy().copy()
        return a

    def save(self, path: str) -> None:
        np.savez_compressed(path, **self.arrays())

    @classmethod
    def load(cls, path: str) -> "RecurrentPolicy":
        d = np.load(path)
        if "gru_w_ih" not in d.files:
            raise ValueError(f"{path} holds a feed-forward policy (no gru_w_ih): load it with policy.PolicyMLP")
        ws = [d[f"w{i}"] for i in range(4)]
        pi = cls((ws[0].shape[0],) + tuple(w.shape[1] for w in ws), int(d["gru_w_hh"].shape[1]))
        with torch.no_grad():
            pi.mean.copy_(torch.from_numpy(d["mean"])); pi.std.copy_(torch.from_numpy(d["std"]))
            for i, lin in enumerate(pi.layers):
                lin.weight.copy_(torch.from_numpy(ws[i]).T); lin.bias.copy_(torch.from_numpy(d[f"b{i}"]))
            for k in GRU_KEYS:
                getattr(pi, k).copy_(torch.from_numpy(d[k]))
        return pi

    def _trunk(self, obs):
        x = (obs - self.mean) / self.std
        for lin in self.layers[:3]:
            x = F.silu(lin(x))
        return x

    def _cell(self, gi, m0):
        R = self.memory
        gh = F.linear(m0, self.gru_w_hh, self.gru_b_hh)
        r = torch.sigmoid(gi[..., :R] + gh[..., :R])
        u = torch.sigmoid(gi[..., R:2 * R] + gh[..., R:2 * R])
        n = torch.tanh(gi[..., 2 * R:] + r * gh[..., 2 * R:])
        return (1 - u) * n + u * m0

    def _head(self, h3, m1):
        return self.layers[3](h3) + F.linear(m1, self.mem_w)

    def step(self, obs: torch.Tensor, mem: torch.Tensor, clear: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """one acting step -> (action [N, 12], head [N, 24], the new memory [N, R]); a row of `mem` whose `clear` is set is not used"""
        h3 = self._trunk(obs)
        m0 = mem if clear is None else torch.where(clear.bool()[:, None], torch.zeros((), dtype=mem.dtype, device=mem.device), mem)
        m1 = self._cell(F.linear(h3, self.gru_w_ih, self.gru_b_ih), m0)
        head = self._head(h3, m1)
        return torch.tanh(head[:, :head.shape[1] // 2]), head, m1

    def sequence(self, obs: torch.Tensor, m_init: torch.Tensor, clear: torch.Tensor) -> torch.Tensor:
        """obs [T, B, od], m_init [B, R], clear [T, B] -> heads [T, B, 24]; m0_t = clear_t ? 0 : m1_{t-1}, m1_{-1} = m_init.  Differentiable."""
        h3 = self._trunk(obs)
        gi = F.linear(h3, self.gru_w_ih, self.gru_b_ih)
        zero = torch.zeros((), dtype=m_init.dtype, device=m_init.device)
        prev, heads = m_init, []
        for t in range(obs.shape[0]):
            m0 = torch.where(clear[t].bool()[:, None], zero, prev)
            prev = self._cell(gi[t], m0)
            heads.append(self._head(h3[t], prev))
        return torch.stack(heads)


class RecurrentActor:
    """The acting step of a roll-out under a RecurrentPolicy: pgtt_learn_recurrent_act on the env's observation (or `obs`), the memory [N, R] kept
    here and cleared by the env's `done` of the step before (use_done) and, on the first call and after reset_memory(), for every env.
    storage["obs" | "mem0" | "clear"] are [T, N, .] rows written by act(t).  act(t, sample=True) is pgtt_learn_recurrent_act_sample: the action is
    tanh(u) of a draw from the tanh-normal head (Philox, keyed by `seed`, the env's global id and counters[1]), and storage["u" | "logp"] receive the
    pre-tanh sample and its log-probability.  `counters` is the device int64[2] {storage row, draw counter} that pgtt_rollout_record advances; the
    acting step reads the draw counter only - its row is the `t` it is given."""

    def __init__(self, env, T: int, memory: int = 64, obs: Optional[torch.Tensor] = None, seed: int = 0, counters: Optional[torch.Tensor] = None):
        if torch.device(env.device).type != "cuda":
            raise learn.LearnError("RecurrentActor needs a Joystick on a ROCm device; there is no CPU path")
        if not memory_ok(memory):
            raise learn.LearnError(f"memory must be a multiple of 16 in [16, {MAX_MEMORY}], not {memory!r}")
        self.env, self.T, self.memory = env, int(T), int(memory)
        self._L = learn.lib()
        dev, n, od, R = env.device, env.num_envs, env.observation_size["state"], self.memory
        self.obs = env.buffers["obs_state"] if obs is None else obs
        if not (self.obs.dtype == torch.float32 and self.obs.is_contiguous() and tuple(self.obs.shape) == (n, od) and self.obs.device == env.buffers["obs_state"].device):
            raise ValueError(f"RecurrentActor: `obs` must be {n} x {od} contiguous float32 values on {dev}")
        z = lambda *sh: torch.zeros(*sh, device=dev)
        self.dims = (od, 512, 256, 128, 2 * abi.NU)
        d = self.dims
        self.mean, self.std = z(od), torch.ones(od, device=dev)
        self.w, self.b = [z(d[i + 1], d[i]) for i in range(4)], [z(d[i + 1]) for i in range(4)]
        self.gru = {"gru_w_ih": z(3 * R, d[3]), "gru_w_hh": z(3 * R, R), "gru_b_ih": z(3 * R), "gru_b_hh": z(3 * R), "mem_w": z(d[4], R)}
        self.mem, self.action = z(n, R), z(n, abi.NU)
        self.storage: Dict[str, torch.Tensor] = {"obs": z(self.T, n, od), "mem0": z(self.T, n, R),
                                                  "clear": torch.zeros(self.T, n, dtype=torch.uint8, device=dev)}
        self.work = z(int(self._L.pgtt_learn_recurrent_act_work_floats(n, od, d[1], d[2], d[3])))
        self._clear_all = True
        a = PgttLearnRecurrentActArgs()
        a.obs, a.mean, a.std = self.obs.data_ptr(), self.mean.data_ptr(), self.std.data_ptr()
        for i in range(4):
            setattr(a, f"w{i}", self.w[i].data_ptr()); setattr(a, f"b{i}", self.b[i].data_ptr())
        a.w_ih, a.w_hh, a.b_ih, a.b_hh, a.w_m = (self.gru[k].data_ptr() for k in GRU_KEYS)
        a.done, a.clear_mask = env.buffers["done"].data_ptr(), None
        a.mem, a.action, a.work = self.mem.data_ptr(), self.action.data_ptr(), self.work.data_ptr()
        a.num_envs, a.obs_dim, a.h1, a.h2, a.h3, a.memory, a.store_rows, a.use_done = n, od, d[1], d[2], d[3], R, self.T, 1
        self._args = a
        # the sampled step: its own copy of the struct above (embedded, refreshed by act), the draw counter and the two rows it adds
        self.storage["u"], self.storage["logp"] = z(self.T, n, abi.NU), z(self.T, n)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev) if counters is None else counters
        if not (self.counters.dtype == torch.int64 and self.counters.numel() == 2 and self.counters.is_contiguous()
                and self.counters.device == self.mem.device):
            raise ValueError(f"RecurrentActor: `counters` must be two contiguous int64 values on {dev}")
        s = PgttLearnRecurrentSampleArgs()
        s.counters, s.seed, s.env_id_offset = self.counters.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(getattr(env, "env_id_offset", 0))
        self._sample_args = s

    @torch.no_grad()
    def load(self, policy: RecurrentPolicy) -> None:
        """the policy's tensors into the buffers the kernel reads, in place"""
        assert policy.dims == self.dims and policy.memory == self.memory, (policy.dims, policy.memory)
        self.mean.copy_(policy.mean); self.std.copy_(policy.std)
        for i, lin in enumerate(policy.layers):
            self.w[i].copy_(lin.weight); self.b[i].copy_(lin.bias)
        for k in GRU_KEYS:
            self.gru[k].copy_(getattr(policy, k))

    def reset_memory(self) -> None:
        """the next act() starts every env from a zero memory (clear_all)"""
        self._clear_all = True

    def act(self, t: Optional[int] = None, head: Optional[torch.Tensor] = None, sample: bool = False, eps: Optional[torch.Tensor] = None,
            deterministic: bool = False) -> torch.Tensor:
        """the deterministic action tanh(loc) for the current observation -> self.action; with t, row t of the storage is written; `head` [N, 24]
        receives the raw head.  sample=True: the action is tanh(u), u = loc + scale eps with eps drawn in the kernel (or `eps` [N, 12]; deterministic:
        u = loc), and with t the rows "u" and "logp" are written too"""
        a, S = self._args, self.storage
        if not sample and (eps is not None or deterministic):
            raise ValueError("RecurrentActor.act: `eps` and `deterministic` belong to sample=True")
        a.clear_all, self._clear_all = int(self._clear_all), False
        if head is not None:
            assert head.is_contiguous() and head.dtype == torch.float32 and tuple(head.shape) == (self.env.num_envs, self.dims[4])
        a.head = None if head is None else head.data_ptr()
        a.t = 0 if t is None else int(t)
        a.store_obs, a.store_mem0, a.store_clear = (None, None, None) if t is None else (S["obs"].data_ptr(), S["mem0"].data_ptr(), S["clear"].data_ptr())
        if not sample:
            learn.check(self._L.pgtt_learn_recurrent_act(C.byref(a), _stream(self.env.device)))
            return self.action
        s = self._sample_args
        if eps is not None:
            assert eps.is_contiguous() and eps.dtype == torch.float32 and tuple(eps.shape) == (self.env.num_envs, abi.NU) and eps.device == self.mem.device
        s.act = a                                   # a copy of the struct as it stands now
        s.eps, s.deterministic = None if eps is None else eps.data_ptr(), int(bool(deterministic))
        s.store_u, s.store_logp = (None, None) if t is None else (S["u"].data_ptr(), S["logp"].data_ptr())
        learn.check(self._L.pgtt_learn_recurrent_act_sample(C.byref(s), _stream(self.env.device)))
        return self.action


class SequenceLearner:
    """One BPTT update over a minibatch of whole unrolls - B_env envs by T steps out of the roll-out's [T, N, .] rows - on the current stream:
    pgtt_learn_gather_rows with the indices t N + e (t-major: a step's rows are contiguous), the trunk over all T B rows, gi over all rows as one
    product, per step one gh product and one cell launch, the head over all rows (W3 h3 + b3, W_m m1, their sum), pgtt_learn_distill_loss, the
    backward recurrence (per step the cell's backward, dgh W_hh and an add), the weight gradients (one pgtt_ppo_linear_backward per weight tensor over
    all rows, straight into the flat gradient) and pgtt_learn_clip_adam: 24 + 5 T launches.  After two eager calls it is one captured graph without
    parallel branches.  m_init (the stored mem0 of row 0), the clear flags and the indices are filled outside the graph into fixed buffers."""

    def __init__(self, policy: RecurrentPolicy, flat: FlatParams, obs_store: torch.Tensor, label_store: torch.Tensor, mem0_store: torch.Tensor,
                 clear_store: torch.Tensor, b_env: int, cfg, use_graph: bool = True):
        dev = obs_store.device
        if dev.type != "cuda":
            raise learn.LearnError("the sequence learner runs on a GPU only; there is no CPU form")
        T, N, od = obs_store.shape
        R, d = policy.memory, policy.dims
        assert obs_store.is_contiguous() and label_store.is_contiguous() and mem0_store.is_contiguous() and clear_store.is_contiguous()
        assert tuple(label_store.shape) == (T, N, self._label_dim(d)) and tuple(mem0_store.shape)[1:] == (N, R) and tuple(clear_store.shape) == (T, N)
        assert clear_store.dtype == torch.uint8 and od == d[0] and policy.mean.is_contiguous() and policy.std.is_contiguous()
        self.policy, self.flat, self.cfg, self.dev = policy, flat, cfg, dev
        self.obs_store, self.label_store, self.mem0_store, self.clear_store = obs_store, label_store, mem0_store, clear_store
        self.T, self.N, self.B, self.R, self.dims = T, N, int(b_env), R, d
        self.lib, self.plib = learn.lib(), native.lib()
        B, TB = self.B, T * self.B
        self.rows = TB
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.idx = torch.zeros(TB, dtype=torch.long, device=dev)
        self._t_off = (torch.arange(T, device=dev) * N)[:, None]
        self.m_init, self.clear = z(B, R), torch.zeros(T, B, dtype=torch.uint8, device=dev)
        self.x, self.y = z(TB, od), z(TB, self._label_dim(d))
        self.h = [z(TB, d[i + 1]) for i in range(3)]
        self.zs = [z(TB, d[i + 1]) for i in range(3)]
        self.dz = [z(TB, d[i + 1]) for i in range(3)]
        self.dz3b = z(TB, d[3])
        self.gi, self.gh, self.gates, self.dgi, self.dgh = (z(TB, 3 * R) for _ in range(5))
        self.m0, self.m1, self.dm1_head = z(TB, R), z(TB, R), z(TB, R)
        self.dm0, self.direct, self.tmp = z(B, R), z(B, R), z(B, R)
        self.head, self.head_h, self.head_m, self.dhead = (z(TB, d[4]) for _ in range(4))
        self.zero_bias, self.db_none = z(d[4]), z(d[4])
        self.loss2, self.norm = z(2), z(1)
        self.partial = z(2 * ((TB + 63) // 64))
        self.adam_partial = z(self.lib.pgtt_learn_adam_partials(flat.numel))
        self.use_graph, self.graph, self.calls = use_graph, None, 0
        # the weight gradients: (input rows, output gradient rows, M, N, dW, db)
        L, g = policy.layers, flat.grad_of
        self.wgrads = [(self.m1, self.dhead, R, d[4], g(policy.mem_w), self.db_none),
                       (self.h[2], self.dhead, d[3], d[4], g(L[3].weight), g(L[3].bias)),
                       (self.h[2], self.dgi, d[3], 3 * R, g(policy.gru_w_ih), g(policy.gru_b_ih)),
                       (self.m0, self.dgh, R, 3 * R, g(policy.gru_w_hh), g(policy.gru_b_hh)),
                       (self.h[1], self.dz[2], d[2], d[3], g(L[2].weight), g(L[2].bias)),
                       (self.h[0], self.dz[1], d[1], d[2], g(L[1].weight), g(L[1].bias)),
                       (self.x, self.dz[0], d[0], d[1], g(L[0].weight), g(L[0].bias))]
        scratch, self.S = 1, []
        for _, _, M, Nn, _, _ in self.wgrads:
            tiles = ((M + 63) // 64) * ((Nn + 63) // 64)
            S = max(1, min(64, int(os.environ.get("PGTT_PPO_SPLITK", "768")) // tiles, TB // 16))      # as distill.DistillLearner
            self.S.append(S)
            scratch = max(scratch, S * (Nn * M + Nn))
        self.lb_partial = z(scratch)

    @staticmethod
    def _label_dim(d) -> int:
        """the width of the rows of `label_store` that the gather copies into self.y next to the normalised observation"""
        return d[4]

    def _loss(self) -> None:
        """self.head [T B, 24] and self.y -> dL/dhead into self.dhead: the one call a subclass replaces (recurrent_ppo.SequencePPOLearner)"""
        learn.check(self.lib.pgtt_learn_distill_loss(C.c_void_p(self.head.data_ptr()), C.c_void_p(self.y.data_ptr()), self.rows, self.dims[4] // 2,
                                                     C.c_void_p(self.partial.data_ptr()), C.c_void_p(self.loss2.data_ptr()),
                                                     C.c_void_p(self.dhead.data_ptr()), _stream(self.dev)))

    def _forward_backward(self):
        L, P, st, p, check = self.lib, self.plib, _stream(self.dev), (lambda t: None if t is None else C.c_void_p(t.data_ptr())), learn.check
        pi, T, B, TB, R, d = self.policy, self.T, self.B, self.rows, self.R, self.dims
        lin = pi.layers
        check(L.pgtt_learn_gather_rows(p(self.idx), p(self.obs_store), p(self.label_store), p(pi.mean), p(pi.std), TB, self.T * self.N, d[0],
                                       self.y.shape[1], p(self.x), p(self.y), st))
        x = self.x
        for i in range(3):
            check(L.pgtt_learn_linear_forward(p(x), p(lin[i].weight), p(lin[i].bias), TB, d[i], d[i + 1], 1, p(self.h[i]), p(self.zs[i]), st))
            x = self.h[i]
        h3 = self.h[2]
        check(L.pgtt_learn_linear_forward(p(h3), p(pi.gru_w_ih), p(pi.gru_b_ih), TB, d[3], 3 * R, 0, p(self.gi), None, st))
        check(L.pgtt_learn_gru_clear_rows(p(self.m_init), p(self.clear[0]), B, R, p(self.m0[:B]), st))
        rows = lambda a, t: a[t * B:(t + 1) * B]
        for t in range(T):
            check(L.pgtt_learn_linear_forward(p(rows(self.m0, t)), p(pi.gru_w_hh), p(pi.gru_b_hh), B, R, 3 * R, 0, p(rows(self.gh, t)), None, st))
            nxt = t + 1 < T
            check(L.pgtt_learn_gru_cell_forward(p(rows(self.gi, t)), p(rows(self.gh, t)), p(rows(self.m0, t)), p(self.clear[t + 1]) if nxt else None, B, R,
                                                p(rows(self.gates, t)), p(rows(self.m1, t)), p(rows(self.m0, t + 1)) if nxt else None, st))
        check(L.pgtt_learn_linear_forward(p(h3), p(lin[3].weight), p(lin[3].bias), TB, d[3], d[4], 0, p(self.head_h), None, st))
        check(L.pgtt_learn_linear_forward(p(self.m1), p(pi.mem_w), p(self.zero_bias), TB, R, d[4], 0, p(self.head_m), None, st))
        check(L.pgtt_learn_add_rows(p(self.head_h), p(self.head_m), TB * d[4], p(self.head), st))
        self._loss()
        # the backward recurrence
        check(L.pgtt_learn_linear_backward_data(p(self.dhead), p(pi.mem_w), None, TB, R, d[4], p(self.dm1_head), st))
        for t in range(T - 1, -1, -1):
            nxt = t + 1 < T
            check(L.pgtt_learn_gru_cell_backward(p(rows(self.gates, t)), p(rows(self.gh, t)), p(rows(self.m0, t)), p(rows(self.dm1_head, t)),
                                                 p(self.dm0) if nxt else None, p(self.clear[t + 1]) if nxt else None, B, R,
                                                 p(rows(self.dgi, t)), p(rows(self.dgh, t)), p(self.direct), st))
            if t > 0:                       # m_init gets no gradient: the sequence is truncated at the unroll's start
                check(L.pgtt_learn_linear_backward_data(p(rows(self.dgh, t)), p(pi.gru_w_hh), None, B, R, 3 * R, p(self.tmp), st))
                check(L.pgtt_learn_add_rows(p(self.direct), p(self.tmp), B * R, p(self.dm0), st))
        # dL/dz3: the two sources of dL/dh3, silu'(z3) applied once per addend
        check(L.pgtt_learn_linear_backward_data(p(self.dhead), p(lin[3].weight), p(self.zs[2]), TB, d[3], d[4], p(self.dz[2]), st))
        check(L.pgtt_learn_linear_backward_data(p(self.dgi), p(pi.gru_w_ih), p(self.zs[2]), TB, d[3], 3 * R, p(self.dz3b), st))
        check(L.pgtt_learn_add_rows(p(self.dz[2]), p(self.dz3b), TB * d[3], p(self.dz[2]), st))
        for i in (2, 1):
            check(L.pgtt_learn_linear_backward_data(p(self.dz[i]), p(lin[i].weight), p(self.zs[i - 1]), TB, d[i], d[i + 1], p(self.dz[i - 1]), st))
        for (xin, dy, M, Nn, dw, db), S in zip(self.wgrads, self.S):
            native.check(P.pgtt_ppo_linear_backward(p(xin), p(dy), C.c_int(TB), C.c_int(M), C.c_int(Nn), C.c_int(S), p(self.lb_partial), p(dw), p(db), st))

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
    def fill(self, env_idx: torch.Tensor) -> None:
        """the minibatch's fixed buffers, outside the graph: row indices t N + e, m_init = the stored mem0 of row 0, the clear flags"""
        e = env_idx.to(self.dev).long()
        assert e.numel() == self.B
        self.idx.copy_((self._t_off + e[None, :]).reshape(-1))
        self.m_init.copy_(self.mem0_store[0].index_select(0, e))
        self.clear.copy_(self.clear_store.index_select(1, e))

    @torch.no_grad()
    def update(self, env_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one update over the unrolls of the envs `env_idx` [B_env] (None: the fixed buffers as they stand) -> loss2 = (KL, action error)"""
        if env_idx is not None:
            self.fill(env_idx)
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
