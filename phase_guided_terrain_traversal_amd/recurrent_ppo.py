"""PPO fine-tuning of a recurrent policy on a perceived observation: the second stage behind the distillation of distill.py.  A
recurrent_policy.RecurrentPolicy - a distilled student, or a feed-forward policy given a memory with W_m = 0 - is trained with rewards on what the
sensors deliver, next to a feed-forward critic on the privileged observation (an asymmetric critic, as ppo.ActorCritic's).

    policy = RecurrentPolicy.load("distilled.npz")
    out = finetune(env, policy, FinetuneConfig(iterations=50), obs="elevation")
    out.save("finetuned.npz")                  # the 13-tensor file of RecurrentPolicy.save: evaluate.py --policy reads it

One acting step is RecurrentActor.act(t, sample=True) (pgtt_learn_recurrent_act_sample: five launches, the draw, u, logp and tanh(u) fused into the
last), env.step and pgtt_rollout_record.  One update (SequencePPOLearner) is recurrent_policy.SequenceLearner's BPTT over B_env whole unrolls with
pgtt_ppo_policy_loss in the place of the distillation loss, the critic's gather, four forwards, value loss and seven backward launches on the same
minibatch rows, and ONE pgtt_learn_clip_adam over one flat buffer that holds both nets: 37 + 5 T launches and one torch.randn, all existing entries
of libpgtt_learn.so and libpgtt.so, on one stream, one captured graph without parallel branches after two eager calls.  The policy's observation
statistics stay the loaded policy's (frozen: a fine-tuned file acts on the same normalisation); the critic's follow a RunningNorm as in ppo.train.
GPU only, one process: there is no CPU form, no fall-back to PyTorch ops and no data parallel.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Union

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import abi, learn, native, ppo
from .learn import FlatParams, _Layer, _stream
from .recurrent_policy import RecurrentActor, RecurrentPolicy, SequenceLearner, memory_ok

HIDDEN = (512, 256, 128)


class FinetuneError(RuntimeError):
    pass


@dataclass
class FinetuneConfig(ppo.PPOConfig):
    """PPOConfig's fields with the meaning they have in ppo.train (unroll_length, num_minibatches, num_updates_per_batch, learning_rate, discounting,
    gae_lambda, entropy_cost, clipping_epsilon, max_grad_norm, reward_scaling, seed; num_timesteps, num_evals, batch_size and learner are not read:
    a minibatch is num_envs / num_minibatches whole unrolls) plus the two below.  The memory's size is the policy's."""
    learning_rate: float = 3e-5              # a tenth of ppo.train's 3e-4: the run starts from a trained policy (DESIGN.md 25 has a run at 1e-4)
    iterations: int = 20
    critic_warmup_iters: int = 50            # the first iterations update the critic only: the loaded policy has none


class RecurrentActorCritic(nn.Module):
    """the two nets of one optimiser: parameters() walks the policy's thirteen tensors first, then the value MLP's eight"""

    def __init__(self, policy: RecurrentPolicy, priv_dim: int):
        super().__init__()
        self.policy = policy
        self.value = ppo.mlp((int(priv_dim),) + HIDDEN, 1)


class SequencePPOLearner(SequenceLearner):
    """One PPO update over B_env whole unrolls of T steps out of the roll-out's [T, N, .] rows.  The policy path is SequenceLearner's forward and
    backward launch for launch, with pgtt_ppo_policy_loss where it has pgtt_learn_distill_loss; the rows the gather copies next to the normalised
    observations are the stored pre-tanh samples u.  The critic - model.value on the privileged rows of the same indices - follows on the same stream:
    pgtt_learn_gather_rows (the value targets as the one label column), four pgtt_learn_linear_forward, pgtt_learn_value_loss, three
    pgtt_learn_linear_backward_data, four pgtt_ppo_linear_backward.  Then one pgtt_learn_clip_adam over the flat buffer of both nets: the global norm is
    taken over both, as in learn.NativeLearner.  fill() runs outside the graph: besides the indices, m_init and the clear flags it selects logp_old and
    the advantages of the T B_env rows and normalises the advantages over the minibatch (mean, population standard deviation, + 1e-8).
    update(env_idx, policy=False) runs the critic's launches and the Adam step only, with the policy's segment of the flat gradient at zero: Adam on a
    zero gradient with zero moments changes nothing, so during a warm-up before the first policy update the policy keeps its bits."""

    def __init__(self, model: RecurrentActorCritic, flat: FlatParams, obs_store: torch.Tensor, u_store: torch.Tensor, logp_store: torch.Tensor,
                 mem0_store: torch.Tensor, clear_store: torch.Tensor, priv_store: torch.Tensor, adv_store: torch.Tensor, ret_store: torch.Tensor,
                 mean_p: torch.Tensor, std_p: torch.Tensor, b_env: int, cfg, use_graph: bool = True):
        super().__init__(model.policy, flat, obs_store, u_store, mem0_store, clear_store, b_env, cfg, use_graph=use_graph)
        T, N, TB, dev = self.T, self.N, self.rows, self.dev
        pd = priv_store.shape[2]
        for s, shape in ((logp_store, (T, N)), (adv_store, (T, N)), (ret_store, (T, N)), (priv_store, (T, N, pd))):
            assert s.is_contiguous() and s.dtype == torch.float32 and tuple(s.shape) == shape, (tuple(s.shape), shape)
        assert mean_p.is_contiguous() and std_p.is_contiguous() and mean_p.numel() == std_p.numel() == pd
        self.model, self.logp_store, self.adv_store, self.ret_store, self.priv_store = model, logp_store, adv_store, ret_store, priv_store
        self.mean_p, self.std_p, self.pd = mean_p, std_p, pd
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.logp_old, self.adv, self.ret, self.x_p = z(TB), z(TB), z(TB, 1), z(TB, pd)
        self.loss3, self.vloss = z(3), z(1)
        lins = [m for m in model.value if isinstance(m, nn.Linear)]
        assert lins[0].in_features == pd and lins[-1].out_features == 1
        self.vlayers, x, scratch = [], self.x_p, 1
        for i, lin in enumerate(lins):
            L = _Layer()
            L.w, L.b, L.M, L.N, L.act = lin.weight, lin.bias, lin.in_features, lin.out_features, int(i + 1 < len(lins))
            L.x = x
            L.y, L.z, L.dy = z(TB, L.N), (z(TB, L.N) if L.act else None), z(TB, L.N)
            L.dw, L.db = flat.grad_of(lin.weight), flat.grad_of(lin.bias)
            tiles = ((L.M + 63) // 64) * ((L.N + 63) // 64)
            L.S = max(1, min(64, int(os.environ.get("PGTT_PPO_SPLITK", "768")) // tiles, TB // 16))      # as learn.NativeLearner
            scratch = max(scratch, L.S * (L.N * L.M + L.N))
            x = L.y
            self.vlayers.append(L)
        self.vb_partial = z(scratch)
        # the policy's tensors are the first parameters of the module, so its gradient is the head of the flat gradient
        self.policy_numel = sum(p.numel() for p in model.policy.parameters())
        assert flat.offset_of[id(lins[0].weight)] == self.policy_numel and flat.numel == self.policy_numel + sum(p.numel() for p in model.value.parameters())
        self._policy_grad_live = False
        self.graph_critic, self.calls_critic = None, 0

    @staticmethod
    def _label_dim(d) -> int:
        return d[4] // 2                     # the gather's label rows are the pre-tanh samples u [., 12]

    def _loss(self) -> None:
        p, cfg = (lambda t: C.c_void_p(t.data_ptr())), self.cfg
        A = self.dims[4] // 2
        eps = torch.randn(self.rows, A, dtype=torch.float32, device=self.dev)
        native.check(self.plib.pgtt_ppo_policy_loss(p(self.head), p(self.y), p(self.logp_old), p(self.adv), p(eps), C.c_int(self.rows), C.c_int(A),
                                                    C.c_float(float(cfg.clipping_epsilon)), C.c_float(float(cfg.entropy_cost)),
                                                    p(self.partial), p(self.loss3), p(self.dhead), _stream(self.dev)))

    def _critic(self) -> None:
        L, P, st, TB, check = self.lib, self.plib, _stream(self.dev), self.rows, learn.check
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        check(L.pgtt_learn_gather_rows(p(self.idx), p(self.priv_store), p(self.ret_store), p(self.mean_p), p(self.std_p), TB, self.T * self.N, self.pd, 1,
                                       p(self.x_p), p(self.ret), st))
        V = self.vlayers
        for l in V:
            check(L.pgtt_learn_linear_forward(p(l.x), p(l.w), p(l.b), TB, l.M, l.N, l.act, p(l.y), p(l.z), st))
        check(L.pgtt_learn_value_loss(p(V[-1].y), p(self.ret), TB, p(self.vloss), p(V[-1].dy), st))
        for i in range(len(V) - 1, 0, -1):
            check(L.pgtt_learn_linear_backward_data(p(V[i].dy), p(V[i].w), p(V[i - 1].z), TB, V[i].M, V[i].N, p(V[i - 1].dy), st))
        for l in reversed(V):
            native.check(P.pgtt_ppo_linear_backward(p(l.x), p(l.dy), C.c_int(TB), C.c_int(l.M), C.c_int(l.N), C.c_int(l.S), p(self.vb_partial),
                                                    p(l.dw), p(l.db), st))

    def _eager(self):
        self._forward_backward()
        self._critic()
        self._apply()

    def _eager_critic(self):
        self._critic()
        self._apply()

    @torch.no_grad()
    def fill(self, env_idx: torch.Tensor) -> None:
        """the minibatch's fixed buffers, outside the graph: SequenceLearner's, and logp_old and the normalised advantages of the rows t N + e"""
        super().fill(env_idx)
        e = env_idx.to(self.dev).long()
        self.logp_old.copy_(self.logp_store.index_select(1, e).reshape(-1))
        a = self.adv_store.index_select(1, e).reshape(-1)
        self.adv.copy_((a - a.mean()) / (a.std(unbiased=False) + 1e-8))

    def _capture(self, body):
        try:
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            return g
        except Exception as exc:
            print(f"[finetune] HIP graph capture of the update failed ({exc}); running eagerly")
            self.use_graph = False
            return None

    @torch.no_grad()
    def update(self, env_idx: Optional[torch.Tensor] = None, policy: bool = True) -> torch.Tensor:
        """one update over the unrolls of the envs `env_idx` [B_env] (None: the fixed buffers as they stand) -> loss3 = (policy total, -mean surr,
        mean entropy) of pgtt_ppo_policy_loss; self.vloss holds the value loss.  policy=False: the critic alone (loss3 keeps its last values)."""
        if env_idx is not None:
            self.fill(env_idx)
        if policy:
            self._policy_grad_live = True
            self.calls += 1
            if self.use_graph and self.graph is None and self.calls == 3:            # two eager updates warmed everything up
                self.graph = self._capture(self._eager)
            if self.graph is not None:
                self.graph.replay()
            else:
                self._eager()
            return self.loss3
        if self._policy_grad_live:               # back from a policy update: its gradient must not reach this Adam step
            self.flat.grad[:self.policy_numel].zero_()
            self._policy_grad_live = False
        self.calls_critic += 1
        if self.use_graph and self.graph_critic is None and self.calls_critic == 3:
            self.graph_critic = self._capture(self._eager_critic)
        if self.graph_critic is not None:
            self.graph_critic.replay()
        else:
            self._eager_critic()
        return self.loss3


def _refuse(env, policy, cfg) -> None:
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise FinetuneError(f"fine-tuning runs in one process: this process group has {dist.get_world_size()} ranks and data parallel is not built")
    if not memory_ok(getattr(policy, "memory", None)):
        raise FinetuneError(f"the policy's memory must be a multiple of 16 in [16, 256], not {getattr(policy, 'memory', None)!r}")
    if int(cfg.num_minibatches) <= 0 or env.num_envs % int(cfg.num_minibatches) != 0:
        raise FinetuneError(f"num_minibatches = {cfg.num_minibatches} does not divide the {env.num_envs} envs: a minibatch is a set of whole unrolls")
    if torch.device(env.device).type != "cuda":
        raise FinetuneError("fine-tuning runs on a GPU only: the env is on a CPU device and there is no CPU form")
    if getattr(env, "curriculum", None) is not None:
        raise FinetuneError("fine-tuning on an env with a terrain curriculum is not built: the curriculum's restart has to follow the record")


class Finetuned:
    """what finetune() returns: the trained policy (its arrays in the layout of RecurrentPolicy.save), the value net and the per-iteration history"""

    def __init__(self, model: RecurrentActorCritic, history: List[Dict[str, float]], actor: RecurrentActor):
        self.policy, self.value, self.history, self.actor = model.policy, model.value, history, actor
        self.arrays: Dict[str, np.ndarray] = model.policy.arrays()

    def save(self, path: str) -> None:
        np.savez_compressed(path, **self.arrays)


class Rollout:
    """T sampled acting steps of the env under the policy, into the actor's storage plus "priv", "rew", "done", "trunc" rows.  Per step:
    RecurrentActor.act(t, sample=True), the privileged row copied, env.step, pgtt_rollout_record (reward, done, truncation, the finished episodes'
    sums, both counters).  No host read-back."""

    def __init__(self, env, actor: RecurrentActor, cfg):
        from .acting import PgttRolloutRecordArgs, _lib
        self.env, self.actor, self.T = env, actor, actor.T
        dev, n, pd = env.device, env.num_envs, env.observation_size["privileged_state"]
        z = lambda *sh: torch.zeros(*sh, device=dev)
        S = actor.storage
        S.update(priv=z(self.T, n, pd), rew=z(self.T, n), done=z(self.T, n), trunc=z(self.T, n))
        self.episode_sums = z(abi.NMETRIC + 3)                       # 22 metric sums, return, length, count
        self._L = _lib()
        r = PgttRolloutRecordArgs()
        r.reward, r.done = env.buffers["reward"].data_ptr(), env.buffers["done"].data_ptr()
        r.ep_steps = env.buffers["istate"][abi.I_EP_STEPS].data_ptr()
        r.up_z = env.buffers["frame"][abi.F_UPVECTOR + 2].data_ptr()
        r.ep_metrics = env.buffers["ep_metrics"].data_ptr()
        r.store_rew, r.store_done, r.store_trunc = S["rew"].data_ptr(), S["done"].data_ptr(), S["trunc"].data_ptr()
        r.counters, r.episode_sums = actor.counters.data_ptr(), self.episode_sums.data_ptr()
        r.reward_scaling, r.num_envs, r.episode_length, r.store_rows = float(cfg.reward_scaling), n, int(env.config["episode_length"]), self.T
        self._rec_args = r

    @torch.no_grad()
    def step(self, t: int) -> None:
        """acting step t of a roll-out; the record writes the row its own counter names, which rollout() keeps equal to t"""
        env, actor = self.env, self.actor
        actor.act(t, sample=True)
        actor.storage["priv"][t].copy_(env.buffers["obs_priv"])
        env.step(actor.action)
        native.check(self._L.pgtt_rollout_record(C.byref(self._rec_args), torch.cuda.current_stream(env.device).cuda_stream))

    def rollout(self) -> Dict[str, torch.Tensor]:
        self.actor.counters[0].zero_()                               # the record's row; the draw counter keeps running
        for t in range(self.T):
            self.step(t)
        return self.actor.storage


def finetune(env, policy: RecurrentPolicy, cfg: FinetuneConfig, obs: Union[str, torch.Tensor] = "elevation",
             progress_fn: Optional[Callable[[int, Dict[str, float]], Optional[bool]]] = None, use_graph: bool = True) -> Finetuned:
    """PPO on `obs` from `policy`; the env (autoreset=True) is stepped from the state it is in (reset it first).  Per iteration: T sampled acting
    steps, the critic's values of the T + 1 privileged rows and GAE, then num_updates_per_batch passes over a random partition of the envs into
    num_minibatches groups of whole unrolls - critic-only during the first critic_warmup_iters iterations.  The memory is cleared here once and by
    `done` afterwards; it carries across iterations.  progress_fn(iteration, metrics) is called once per iteration; a true return stops the run."""
    from .distill import DistillError, perceived
    _refuse(env, policy, cfg)
    dev, n, T = env.device, env.num_envs, int(cfg.unroll_length)
    try:
        seen = perceived(env, obs)
    except DistillError as exc:
        raise FinetuneError(str(exc)) from None
    if policy.dims[0] != env.observation_size["state"]:
        raise FinetuneError(f"the policy reads {policy.dims[0]} observations, the env gives {env.observation_size['state']}")
    pd = env.observation_size["privileged_state"]
    torch.manual_seed(int(cfg.seed))
    model = RecurrentActorCritic(policy, pd).to(dev)
    flat = FlatParams(model)
    actor = RecurrentActor(env, T, policy.memory, obs=seen, seed=int(cfg.seed))
    actor.load(model.policy)
    actor.reset_memory()
    roll = Rollout(env, actor, cfg)
    S = actor.storage
    norm_p = ppo.RunningNorm(pd, dev)
    mean_p, std_p = torch.zeros(pd, device=dev), torch.ones(pd, device=dev)
    adv, ret = torch.zeros(T, n, device=dev), torch.zeros(T, n, device=dev)
    b_env = n // int(cfg.num_minibatches)
    learner = SequencePPOLearner(model, flat, S["obs"], S["u"], S["logp"], S["mem0"], S["clear"], S["priv"], adv, ret, mean_p, std_p, b_env, cfg,
                                 use_graph=use_graph)
    gen = torch.Generator(device=dev).manual_seed(int(cfg.seed))
    acc = torch.zeros(5, device=dev)
    history: List[Dict[str, float]] = []
    t_start = time.time()
    for it in range(int(cfg.iterations)):
        t0 = time.time()
        with torch.no_grad():
            roll.rollout()
            norm_p.update(S["priv"])
            mean_p.copy_(norm_p.mean); std_p.copy_(norm_p.std)
            values = model.value((torch.cat([S["priv"], env.buffers["obs_priv"][None]], 0) - mean_p) / std_p).squeeze(-1)      # [T + 1, N]
            learn.gae(S["trunc"], S["done"], S["rew"], values[:-1], values[-1], cfg.gae_lambda, cfg.discounting, out=(adv, ret))
        train_policy = it >= int(cfg.critic_warmup_iters)
        acc.zero_()
        updates = 0
        for _ in range(int(cfg.num_updates_per_batch)):
            perm = torch.randperm(n, device=dev, generator=gen)
            for k in range(int(cfg.num_minibatches)):
                l3 = learner.update(perm[k * b_env:(k + 1) * b_env], policy=train_policy)
                acc[:3] += l3; acc[3] += learner.vloss[0]; acc[4] += learner.norm[0]
                updates += 1
        actor.load(model.policy)
        es = roll.episode_sums
        log = torch.cat([acc / max(1, updates), es[abi.NMETRIC:abi.NMETRIC + 3], S["rew"].mean()[None]]).tolist()      # the iteration's one host read
        es.zero_()
        dt = time.time() - t0
        c = max(log[7], 1.0)
        m = {"policy_updates": float(train_policy), "loss": log[0], "policy_loss": log[1], "entropy": log[2], "value_loss": log[3], "grad_norm": log[4],
             "episode_reward": log[5] / c, "episode_length": log[6] / c, "episodes": log[7], "mean_step_reward": log[8], "updates": float(updates),
             "env_steps_per_s": T * n / dt, "seconds": time.time() - t_start}
        history.append(m)
        if progress_fn is not None and progress_fn(it, m):
            break
    return Finetuned(model, history, actor)
