"""An fp64 statement of one recurrent PPO update, written from include/pgtt_learn.h and include/pgtt_train.h and from the three
references it composes - recurrent_policy_reference (the sequence forward with its clears), ppo_reference (log_prob, the clipped surrogate, the
entropy at a given eps, the advantage normalisation) and acting_reference (the sampled head) - and from nothing in recurrent_ppo.py.  A helper module
like them: test_recurrent_ppo_reference.py holds it to facts that do not come from the product code (CPU), test_gpu_recurrent_ppo.py holds the
product code to it.  Everything is torch.float64 on the CPU; the gradients are autograd's.

    heads  = the recurrent policy over B whole unrolls of T steps (obs [T, B, od], m_init [B, R], clear [T, B]), rows t-major: [T B, 24]
    logp   = ppo_reference.log_prob(heads, u);   ratio = exp(logp - logp_old);   a = ppo_reference.normalise_advantage(adv) over the T B rows
    policy = -mean(min(ratio a, clip(ratio, 1 - c, 1 + c) a));   entropy = mean(ppo_reference.entropy(heads, eps))
    v      = value MLP((priv - mean_p) / std_p) [T B];   value_loss = 0.25 mean((ret - v)^2)
    total  = policy - entropy_cost entropy + value_loss
    g     <- g min(1, max_norm / (|g|_2 + 1e-6)) over the thirteen policy tensors and the eight of the value net together
m_init is data: the sequence is truncated at the unroll's start.  A policy=False update is the same with the policy's gradient set to zero.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_reference as pref  # noqa: E402
import recurrent_policy_reference as rref  # noqa: E402

F64 = torch.float64
f64 = rref.f64
POLICY_NAMES = [f"{k}{i}" for i in range(4) for k in "wb"] + list(rref.KEYS)
VALUE_NAMES = [f"v{k}{i}" for i in range(4) for k in "wb"]


def policy_tensors(P):
    """the thirteen trained tensors of a parameter dict in the order of RecurrentPolicy.parameters()"""
    return [t for i in range(4) for t in (P["w"][i], P["b"][i])] + [P[k] for k in rref.KEYS]


def with_tensors(P, tensors):
    """a parameter dict with the thirteen tensors replaced (mean and std kept)"""
    out = {"mean": P["mean"], "std": P["std"], "w": [tensors[2 * i] for i in range(4)], "b": [tensors[2 * i + 1] for i in range(4)]}
    out.update({k: t for k, t in zip(rref.KEYS, tensors[8:])})
    return out


def losses(P, V, mb, clip=0.3, entropy_cost=1e-2):
    """P: fp64 parameter dict (rref.params64's layout), V: [(W, b)] x 4 of the value net, mb: fp64 dict of obs [T, B, od], m_init [B, R], clear bool
    [T, B], u [T, B, 12], logp_old [T, B], adv [T, B] (raw), eps [T B, 12], priv [T, B, pd], ret [T, B], mean_p, std_p.  Differentiable in P and V.
    -> dict(total, policy_total, policy, entropy, value_loss, heads [T B, 24], logp, mag, ratio, v)"""
    T, B = mb["obs"].shape[:2]
    heads = rref.sequence(P, mb["obs"], mb["m_init"], mb["clear"])["heads"].reshape(T * B, -1)
    u, logp_old = mb["u"].reshape(T * B, -1), mb["logp_old"].reshape(-1)
    a = pref.normalise_advantage(mb["adv"].reshape(-1))
    logp, mag = pref.log_prob(heads, u)
    ratio = torch.exp(logp - logp_old)
    surr = torch.minimum(ratio * a, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a)
    pol, ent = -surr.mean(), pref.entropy(heads, mb["eps"]).mean()
    v = pref.silu_mlp((mb["priv"].reshape(T * B, -1) - mb["mean_p"]) / mb["std_p"], V).squeeze(-1)
    v_loss = 0.25 * ((mb["ret"].reshape(-1) - v) ** 2).mean()
    ptotal = pol - entropy_cost * ent
    return {"total": ptotal + v_loss, "policy_total": ptotal, "policy": pol, "entropy": ent, "value_loss": v_loss, "heads": heads, "logp": logp,
            "mag": mag + logp_old.abs(), "ratio": ratio, "v": v, "adv": a}


def minibatch64(mb):
    out = {k: f64(v) for k, v in mb.items() if k != "clear"}
    out["clear"] = mb["clear"].to("cpu").bool()
    return out


def update(P, V, mb, clip=0.3, entropy_cost=1e-2, max_norm=1.0, policy=True):
    """one update in fp64 from parameters and rows of any dtype -> dict: loss_3 = (policy total, -mean surr, mean entropy), value_loss, total, heads,
    dhead (d total / d heads), logp, mag, ratio, grads (UNCLIPPED, the thirteen policy tensors then W0, b0, .., W3, b3 of the value net; the policy's
    are zero with policy=False), grad_norm (unclipped, over all 21), clip_coef"""
    P64 = rref.params64(P)
    pt = [t.clone().requires_grad_(True) for t in policy_tensors(P64)]
    vt = [(f64(w).clone().requires_grad_(True), f64(b).clone().requires_grad_(True)) for w, b in V]
    out = losses(with_tensors(P64, pt), vt, minibatch64(mb), clip, entropy_cost)
    params = pt + [t for wb in vt for t in wb]
    grads = list(torch.autograd.grad(out["total"], params + [out["heads"]]))
    dhead = grads.pop()
    out = {k: v.detach() for k, v in out.items()}
    if not policy:
        grads[:13] = [torch.zeros_like(g) for g in grads[:13]]
    norm = math.sqrt(sum(float((g * g).sum()) for g in grads))
    return {"loss_3": (float(out["policy_total"]), float(out["policy"]), float(out["entropy"])), "value_loss": float(out["value_loss"]),
            "total": float(out["total"]), "heads": out["heads"].detach(), "dhead": dhead, "logp": out["logp"].detach(), "mag": out["mag"],
            "ratio": out["ratio"].detach(), "grads": grads, "grad_norm": norm, "clip_coef": min(1.0, max_norm / (norm + 1e-6))}


def stored_logp(P, obs, mem0, clear, u):
    """the log-probability an acting step stored: one step from its own stored rows obs [N, od], mem0 [N, R] (the memory after clearing), u [N, 12]
    -> (logp [N], mag [N], head [N, 24], |d logp / d head| [N, 24])"""
    s = rref.step(P, obs, mem0, clear)
    head = s["head"].clone().requires_grad_(True)
    logp, mag = pref.log_prob(head, f64(u))
    (dl,) = torch.autograd.grad(logp.sum(), head)
    return logp.detach(), mag, s["head"], dl.abs()
