"""The native PPO learner (libpgtt_learn.so, include/pgtt_learn.h, with the two trainer kernels of libpgtt.so): one minibatch update as ~45
hand-written HIP launches on ONE stream instead of ~150 PyTorch ops on two, and GAE as one launch instead of a loop of T.

    flat = FlatParams(model)                                   # every parameter a view of one fp32 buffer; grad, m, v, step counter next to it
    learner = NativeLearner(model, flat, norm_s, norm_p, B, mb, cfg)
    learner.refresh_stats()                                    # once per iteration: mean / std of the two RunningNorm into the learner's vectors
    loss = learner.update(idx)                                 # ppo._Learner.update: two eager calls, then captured and replayed
    adv, vs = gae(trunc, done, rew, val, boot, lam, gamma)     # ppo.compute_gae with term = done (1 - trunc)

Imported by ppo.train only with PPOConfig.learner == "native"; there is no CPU form and no fall-back to PyTorch ops.
"""
from __future__ import annotations

import ctypes as C
import os

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _sidelib, native

vp, i32 = C.c_void_p, C.c_int32


class PgttLearnGatherArgs(C.Structure):
    _fields_ = [(k, vp) for k in ("idx", "obs", "priv", "u", "logp", "adv", "ret", "mean_s", "std_s", "mean_p", "std_p",
                                  "x_s", "x_p", "u_out", "logp_out", "adv_out", "ret_out")] + \
               [(k, i32) for k in ("B", "rows", "obs_dim", "priv_dim", "act_dim")]


class PgttLearnAdamArgs(C.Structure):
    _fields_ = [(k, vp) for k in ("p", "g", "m", "v", "t", "partial", "norm_1")] + [("P", C.c_int64)] + \
               [(k, C.c_double) for k in ("lr", "beta1", "beta2", "eps")] + [("max_norm", C.c_float), ("grad_scale", C.c_float)]


class PgttLearnRecurrentActArgs(C.Structure):
    """the acting step of the recurrent policy (recurrent_policy.RecurrentActor)"""
    _fields_ = [(k, vp) for k in ("obs", "mean", "std", "w0", "w1", "w2", "w3", "b0", "b1", "b2", "b3", "w_ih", "w_hh", "b_ih", "b_hh", "w_m",
                                  "done", "clear_mask", "mem", "action", "head", "store_obs", "store_mem0", "store_clear", "work")] + \
               [(k, i32) for k in ("num_envs", "obs_dim", "h1", "h2", "h3", "memory", "t", "store_rows", "clear_all", "use_done")]


class PgttLearnRecurrentSampleArgs(C.Structure):
    """the sampled acting step (recurrent_policy.RecurrentActor.act(t, sample=True)): the struct above, embedded, and the sampling fields"""
    _fields_ = [("act", PgttLearnRecurrentActArgs)] + [(k, vp) for k in ("eps", "counters", "store_u", "store_logp")] + \
               [("seed", C.c_uint64), ("env_id_offset", C.c_int64), ("deterministic", i32)]


assert C.sizeof(PgttLearnGatherArgs) == 160 and C.sizeof(PgttLearnAdamArgs) == 104 and C.sizeof(PgttLearnRecurrentActArgs) == 240
assert C.sizeof(PgttLearnRecurrentSampleArgs) == 296


class LearnError(RuntimeError):
    pass


ci, cf = C.c_int, C.c_float
SIDE = _sidelib.SideLib("learn", LearnError, {
    "pgtt_learn_gather": (None, [C.POINTER(PgttLearnGatherArgs), vp]),
    "pgtt_learn_linear_forward": (None, [vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]),
    "pgtt_learn_linear_backward_data": (None, [vp, vp, vp, ci, ci, ci, vp, vp]),
    "pgtt_learn_value_loss": (None, [vp, vp, ci, vp, vp, vp]),
    "pgtt_learn_clip_adam": (None, [C.POINTER(PgttLearnAdamArgs), vp]),
    "pgtt_learn_adam_partials": (None, [C.c_int64]),
    "pgtt_learn_gae": (None, [vp, vp, vp, vp, vp, ci, ci, cf, cf, vp, vp, vp]),
    "pgtt_learn_distill_loss": (None, [vp, vp, ci, ci, vp, vp, vp, vp]),                       # the two entries of distill.py
    "pgtt_learn_gather_rows": (None, [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]),
    "pgtt_learn_recurrent_act": (None, [C.POINTER(PgttLearnRecurrentActArgs), vp]),             # the entries of recurrent_policy.py
    "pgtt_learn_recurrent_act_work_floats": (C.c_int64, [ci, ci, ci, ci, ci]),
    "pgtt_learn_recurrent_act_sample": (None, [C.POINTER(PgttLearnRecurrentSampleArgs), vp]),
    "pgtt_learn_gru_clear_rows": (None, [vp, vp, ci, ci, vp, vp]),
    "pgtt_learn_gru_cell_forward": (None, [vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]),
    "pgtt_learn_gru_cell_backward": (None, [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]),
    "pgtt_learn_add_rows": (None, [vp, vp, C.c_int64, vp, vp]),
}, {"pgtt_learn_sizeof_gather_args": PgttLearnGatherArgs, "pgtt_learn_sizeof_adam_args": PgttLearnAdamArgs,
    "pgtt_learn_sizeof_recurrent_act_args": PgttLearnRecurrentActArgs,
    "pgtt_learn_sizeof_recurrent_sample_args": PgttLearnRecurrentSampleArgs})
LIB_PATH, EXPORTS, lib, check, build_info = SIDE.path, SIDE.exports, SIDE.lib, SIDE.check, SIDE.build_info


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def gae(trunc: torch.Tensor, done: torch.Tensor, rew: torch.Tensor, val: torch.Tensor, boot: torch.Tensor, lambda_: float, discount: float,
        out=None):
    """pgtt_learn_gae: rows [T, N] (contiguous fp32 on one GPU), boot [N]; `done` is the raw flag, the kernel forms term = done (1 - trunc).
    Returns (advantages, value targets), written into `out` = (adv, vs) when given."""
    T, N = rew.shape
    trunc, done, rew, val, boot = (t.contiguous() for t in (trunc, done, rew, val, boot))
    adv, vs = out if out is not None else (torch.empty_like(rew), torch.empty_like(rew))
    check(lib().pgtt_learn_gae(trunc.data_ptr(), done.data_ptr(), rew.data_ptr(), val.data_ptr(), boot.data_ptr(), T, N, float(lambda_), float(discount),
                               adv.data_ptr(), vs.data_ptr(), _stream(rew.device)))
    return adv, vs


class FlatParams:
    """Every parameter of `model` in ONE flat fp32 buffer `flat` (the order of model.parameters()); the module's parameters become views of it, so
    state_dict keys, shapes and values are what they were and load_state_dict / in-place writes through the module land in the buffer.  Next to it
    `grad` (each parameter's .grad is a view of it), Adam's `m` and `v`, and the device step counter `t` (int64[1]).  Moving the module afterwards
    (model.to) would break the aliasing."""

    def __init__(self, model: nn.Module):
        self.params = [p for p in model.parameters() if p.requires_grad]
        dev = self.params[0].device
        assert all(p.dtype == torch.float32 and p.device == dev for p in self.params)
        self.sizes = [p.numel() for p in self.params]
        self.offsets = [sum(self.sizes[:i]) for i in range(len(self.sizes))]
        self.numel = sum(self.sizes)
        self.flat = torch.empty(self.numel, dtype=torch.float32, device=dev)
        self.grad, self.m, self.v = (torch.zeros(self.numel, dtype=torch.float32, device=dev) for _ in range(3))
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.offset_of = {}
        with torch.no_grad():
            for p, o, n in zip(self.params, self.offsets, self.sizes):
                view = self.flat[o:o + n].view(p.shape)
                view.copy_(p)
                p.data = view
                p.grad = self.grad[o:o + n].view(p.shape)
                self.offset_of[id(p)] = o

    def grad_of(self, p) -> torch.Tensor:
        o = self.offset_of[id(p)]
        return self.grad[o:o + p.numel()].view(p.shape)


class _Layer:
    pass


class NativeLearner:
    """ppo._Learner's constructor (with a FlatParams where it takes the optimiser) and update(idx) -> loss.  One update: gather, four forwards per
    net, the policy loss (libpgtt.so, eps from torch.randn) and the value loss, per layer from the top the weight / bias gradient (libpgtt.so,
    written straight into the flat gradient) and the data gradient, under data parallel one all-reduce of the flat gradient, clip + Adam.  All on
    the current stream.  After two eager calls it is one captured graph (two round the all-reduce under data parallel).
    `mean_s / std_s / mean_p / std_p` are the learner's own vectors: refresh_stats() copies the RunningNorm into them once per iteration."""

    def __init__(self, model, flat: FlatParams, norm_s, norm_p, B, mb, cfg, use_graph=True):
        from . import ppo
        dev = B["obs"].device
        if dev.type != "cuda":
            raise LearnError("the native learner runs on a GPU only; use learner='torch' on a CPU device")
        self.model, self.flat, self.norm_s, self.norm_p, self.B, self.cfg, self.mb, self.dev = model, flat, norm_s, norm_p, B, cfg, int(mb), dev
        self.lib, self.plib = lib(), native.lib()
        self.idx = torch.zeros(mb, dtype=torch.long, device=dev)
        self.loss = torch.zeros((), device=dev)
        self.use_graph, self.graph, self.calls = use_graph, None, 0
        self.world, self.dp = ppo._world()[0], ppo._dp()
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        od, pd, A = B["obs"].shape[1], B["priv"].shape[1], B["u"].shape[1]
        self.rows, self.od, self.pd, self.A = B["obs"].shape[0], od, pd, A
        self.mean_s, self.std_s, self.mean_p, self.std_p = z(od), torch.ones(od, device=dev), z(pd), torch.ones(pd, device=dev)
        self.refresh_stats()
        self.x_s, self.x_p, self.u, self.logp, self.adv, self.ret = z(mb, od), z(mb, pd), z(mb, A), z(mb), z(mb), z(mb)
        self.loss3, self.vloss, self.norm = z(3), z(1), z(1)
        self.pl_partial = z(2 * ((mb + 63) // 64))
        self.adam_partial = z(self.lib.pgtt_learn_adam_partials(flat.numel))
        self.nets = []
        scratch = 1
        for seq, x in ((model.policy, self.x_s), (model.value, self.x_p)):
            lins = [m for m in seq if isinstance(m, nn.Linear)]
            layers = []
            for i, lin in enumerate(lins):
                L = _Layer()
                L.w, L.b, L.M, L.N, L.act = lin.weight, lin.bias, lin.in_features, lin.out_features, int(i + 1 < len(lins))
                L.x = x
                L.y, L.z, L.dy = z(mb, L.N), (z(mb, L.N) if L.act else None), z(mb, L.N)
                L.dw, L.db = flat.grad_of(lin.weight), flat.grad_of(lin.bias)
                tiles = ((L.M + 63) // 64) * ((L.N + 63) // 64)
                L.S = max(1, min(64, int(os.environ.get("PGTT_PPO_SPLITK", "768")) // tiles, mb // 16))      # as ppo._LinearLongBatch.backward
                scratch = max(scratch, L.S * (L.N * L.M + L.N))
                x = L.y
                layers.append(L)
            self.nets.append(layers)
        assert self.nets[0][-1].N == 2 * A and self.nets[1][-1].N == 1
        self.lb_partial = z(scratch)

    @torch.no_grad()
    def refresh_stats(self):
        """the statistics do not move during the updates of one iteration: their mean / std vectors are formed once, in place (a captured graph keeps reading them)"""
        self.mean_s.copy_(self.norm_s.mean); self.std_s.copy_(self.norm_s.std)
        self.mean_p.copy_(self.norm_p.mean); self.std_p.copy_(self.norm_p.std)

    def _ptr(self, t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _forward_backward(self):
        L, P, B, st, mb, p = self.lib, self.plib, self.B, _stream(self.dev), self.mb, self._ptr
        a = PgttLearnGatherArgs()
        a.idx = self.idx.data_ptr()
        for k, key in (("obs", "obs"), ("priv", "priv"), ("u", "u"), ("logp", "logp"), ("adv", "adv"), ("ret", "ret")):
            assert B[key].is_contiguous()
            setattr(a, k, B[key].data_ptr())
        a.mean_s, a.std_s, a.mean_p, a.std_p = (t.data_ptr() for t in (self.mean_s, self.std_s, self.mean_p, self.std_p))
        a.x_s, a.x_p, a.u_out, a.logp_out, a.adv_out, a.ret_out = (t.data_ptr() for t in (self.x_s, self.x_p, self.u, self.logp, self.adv, self.ret))
        a.B, a.rows, a.obs_dim, a.priv_dim, a.act_dim = mb, self.rows, self.od, self.pd, self.A
        check(L.pgtt_learn_gather(C.byref(a), st))
        for layers in self.nets:
            for l in layers:
                check(L.pgtt_learn_linear_forward(p(l.x), p(l.w), p(l.b), mb, l.M, l.N, l.act, p(l.y), p(l.z), st))
        pol, val = self.nets
        eps = torch.randn(mb, self.A, dtype=torch.float32, device=self.dev)
        native.check(P.pgtt_ppo_policy_loss(p(pol[-1].y), p(self.u), p(self.logp), p(self.adv), p(eps), C.c_int(mb), C.c_int(self.A),
                                            C.c_float(float(self.cfg.clipping_epsilon)), C.c_float(float(self.cfg.entropy_cost)),
                                            p(self.pl_partial), p(self.loss3), p(pol[-1].dy), st))
        check(L.pgtt_learn_value_loss(p(val[-1].y), p(self.ret), mb, p(self.vloss), p(val[-1].dy), st))
        torch.add(self.loss3[0], self.vloss[0], out=self.loss)
        for layers in self.nets:
            for i in range(len(layers) - 1, -1, -1):
                l = layers[i]
                native.check(P.pgtt_ppo_linear_backward(p(l.x), p(l.dy), C.c_int(mb), C.c_int(l.M), C.c_int(l.N), C.c_int(l.S), p(self.lb_partial),
                                                        p(l.dw), p(l.db), st))
                if i > 0:                       # the first layer's input needs no gradient
                    check(L.pgtt_learn_linear_backward_data(p(l.dy), p(l.w), p(layers[i - 1].z), mb, l.M, l.N, p(layers[i - 1].dy), st))

    def _all_reduce(self):
        if self.dp:
            dist.all_reduce(self.flat.grad)     # the flat gradient IS the bucket

    def _apply(self):
        f, cfg = self.flat, self.cfg
        a = PgttLearnAdamArgs()
        a.p, a.g, a.m, a.v, a.t = f.flat.data_ptr(), f.grad.data_ptr(), f.m.data_ptr(), f.v.data_ptr(), f.t.data_ptr()
        a.partial, a.norm_1, a.P = self.adam_partial.data_ptr(), self.norm.data_ptr(), f.numel
        a.lr, a.beta1, a.beta2, a.eps = float(cfg.learning_rate), 0.9, 0.999, 1e-8
        a.max_norm, a.grad_scale = float(cfg.max_grad_norm), (1.0 / self.world if self.dp else 1.0)
        check(self.lib.pgtt_learn_clip_adam(C.byref(a), _stream(self.dev)))

    def _eager(self):
        self._forward_backward()
        self._all_reduce()
        self._apply()

    @torch.no_grad()
    def update(self, idx):
        self.idx.copy_(idx)
        self.calls += 1
        if self.use_graph and self.graph is None and self.calls == 3:        # two eager updates warmed everything up
            try:
                torch.cuda.synchronize(self.dev)
                if not self.dp:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._forward_backward()
                        self._apply()
                    self.graph = (g,)
                else:                       # the collective stays outside the captured work, as in ppo._Learner
                    ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                    with torch.cuda.graph(ga):
                        self._forward_backward()
                    with torch.cuda.graph(gb, pool=ga.pool()):
                        self._apply()
                    self.graph = (ga, gb)
            except Exception as exc:
                if self.dp:
                    raise
                print(f"[learn] HIP graph capture of the update failed ({exc}); running eagerly")
                self.use_graph = False
        if self.graph is not None:
            self.graph[0].replay()
            if self.dp:
                self._all_reduce()
                self.graph[1].replay()
        else:
            self._eager()
        return self.loss
