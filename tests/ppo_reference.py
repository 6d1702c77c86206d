"""An fp64 statement of one PPO minibatch update, written from the formulas in the header of csrc/pgtt_ppo.hip and
include/pgtt_train.h (the Brax PPO loss and update the trainer restates) and from nothing in ppo.py.  A helper module like
parity_explain.py: the trainer tests (test_ppo_reference.py on the CPU, test_gpu_ppo_kernels.py / test_gpu_ppo_update.py on the GPU)
hold the product code to it.  Everything is torch.float64 on the CPU.

    out    = MLP(normalise(obs)),   loc, raw = out[:, :A], out[:, A:],   scale = softplus(raw) + 1e-3
    logp   = sum_j -0.5 z^2 - log(scale) - 0.5 log(2 pi) - 2 (log 2 - u - softplus(-2 u)),   z = (u - loc) / scale
    ratio  = exp(logp - logp_old),   surr = min(ratio a, clip(ratio, 1 - c, 1 + c) a),   a = (adv - mean) / (population std + 1e-8)
    ent    = sum_j 0.5 + 0.5 log(2 pi) + log(scale) + 2 (log 2 - s - softplus(-2 s)),   s = loc + scale eps      (one sample)
    loss   = -mean(surr) - entropy_cost mean(ent) + 0.25 mean((ret - V(normalise(priv)))^2)
    g     <- g min(1, max_norm / (|g|_2 + 1e-6)) over every parameter;   Adam (0.9, 0.999, 1e-8) with bias correction
"""
import math

import torch

F64 = torch.float64
U32 = 2.0 ** -24          # unit roundoff of fp32
LOGP_OPS = 8              # rounded operations per term of the log-probability (see logp_error)


def f64(x):
    return x.detach().to("cpu", F64)


def softplus(x):
    """log(1 + e^x) without a threshold (fp64: exact to rounding everywhere the tests go)"""
    return torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs()))


def silu_mlp(x, layers):
    """layers = [(W [out, in], b [out]), ...]; SiLU between the layers, none after the last"""
    for i, (w, b) in enumerate(layers):
        x = x @ w.T + b
        if i + 1 < len(layers):
            x = x * torch.sigmoid(x)
    return x


def norm_std(m2, count):
    """std of the running statistics: sqrt(max(m2 / count, 1e-12)) floored at 1e-6; 1 before the first update"""
    if float(count) <= 0:
        return torch.ones_like(m2)
    return torch.sqrt(torch.clamp(m2 / float(count), min=1e-12)).clamp(min=1e-6)


def normalise(x, mean, m2, count):
    return (x - mean) / norm_std(m2, count)


def log_prob(out, u):
    """tanh-normal log-probability of the pre-tanh sample u under head output `out` = (loc | raw); returns (logp [B], mag [B]) with
    mag = sum_j of the absolute values of the terms logp is summed from (without |logp_old|, which the caller adds)"""
    A = u.shape[-1]
    loc, raw = out[..., :A], out[..., A:]
    scale = softplus(raw) + 1e-3
    z = (u - loc) / scale
    sp = softplus(-2.0 * u)
    logp = (-0.5 * z * z - torch.log(scale) - 0.5 * math.log(2 * math.pi) - 2.0 * (math.log(2.0) - u - sp)).sum(-1)
    mag = (0.5 * z * z + torch.log(scale).abs() + 0.5 * math.log(2 * math.pi) + 2.0 * math.log(2.0) + 2.0 * u.abs() + 2.0 * sp).sum(-1)
    return logp, mag.detach()


def logp_error(mag):
    """fp32 error model of logp - logp_old: every term goes through about LOGP_OPS rounded operations (subtract, divide, square, scale,
    the two or three steps of log / exp / log1p at ~2 ulp each, and its place in the running sum), each within 2^-24 of the term's size"""
    return LOGP_OPS * U32 * mag


def entropy(out, eps):
    A = eps.shape[-1]
    loc, raw = out[..., :A], out[..., A:]
    scale = softplus(raw) + 1e-3
    s = loc + scale * eps
    return (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(scale) + 2.0 * (math.log(2.0) - s - softplus(-2.0 * s))).sum(-1)


def normalise_advantage(adv):
    return (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)


def policy_loss(out, u, logp_old, adv, eps, clip, cost):
    """The policy part of the loss for head outputs `out` [B, 2A] and ALREADY normalised advantages `adv`.  Returns a dict: total, policy
    (-mean surr), entropy (mean), grad (d total / d out), and per sample logp, ratio, surr, ent, mag (incl. |logp_old|), err, edge."""
    out = f64(out).requires_grad_(True)
    u, logp_old, adv, eps = f64(u), f64(logp_old), f64(adv), f64(eps)
    logp, mag = log_prob(out, u)
    ratio = torch.exp(logp - logp_old)
    surr = torch.minimum(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv)
    ent = entropy(out, eps)
    pol, ment = -surr.mean(), ent.mean()
    total = pol - cost * ment
    (grad,) = torch.autograd.grad(total, out)
    mag = mag + logp_old.abs()
    err = logp_error(mag)
    r = ratio.detach()
    edge = ((r - (1.0 - clip)).abs() < 4.0 * err * r) | ((r - (1.0 + clip)).abs() < 4.0 * err * r)
    return {"total": float(total.detach()), "policy": float(pol.detach()), "entropy": float(ment.detach()), "grad": grad, "logp": logp.detach(), "ratio": r,
            "surr": surr.detach(), "ent": ent.detach(), "mag": mag, "err": err, "edge": edge}


def update(policy, value, stats_s, stats_p, mb, eps, clip=0.3, entropy_cost=1e-2, max_norm=1.0):
    """One minibatch: policy / value = [(W, b)] x 4 (any dtype, taken to fp64), stats_* = (mean, m2, count), mb = dict of the minibatch rows
    obs, priv, u, logp, adv (raw), ret.  Returns total / policy / entropy / value_loss, grad_out, the UNCLIPPED gradient norm, and `grads`:
    the clipped gradient of every parameter in the order W0, b0, ..., W3, b3 of the policy, then of the value net."""
    pol = [(f64(w).requires_grad_(True), f64(b).requires_grad_(True)) for w, b in policy]
    val = [(f64(w).requires_grad_(True), f64(b).requires_grad_(True)) for w, b in value]
    obs, priv, u, logp_old, adv, ret = (f64(mb[k]) for k in ("obs", "priv", "u", "logp", "adv", "ret"))
    out = silu_mlp(normalise(obs, f64(stats_s[0]), f64(stats_s[1]), stats_s[2]), pol)
    out.retain_grad()
    a = normalise_advantage(adv)
    logp, mag = log_prob(out, u)
    ratio = torch.exp(logp - logp_old)
    surr = torch.minimum(ratio * a, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a)
    p_term = -surr.mean()
    ent = entropy(out, f64(eps)).mean() if eps is not None else torch.zeros((), dtype=F64)
    v = silu_mlp(normalise(priv, f64(stats_p[0]), f64(stats_p[1]), stats_p[2]), val).squeeze(-1)
    v_loss = 0.25 * ((ret - v) ** 2).mean()
    total = p_term - entropy_cost * ent + v_loss
    params = [t for wb in pol + val for t in wb]
    total.backward()
    grads = [p.grad for p in params]
    norm = math.sqrt(sum(float((g * g).sum()) for g in grads))
    coef = min(1.0, max_norm / (norm + 1e-6))
    return {"total": float(total.detach()), "policy": float(p_term.detach()), "entropy": float(ent.detach()), "value_loss": float(v_loss.detach()), "grad_out": out.grad,
            "grad_norm": norm, "clip_coef": coef, "grads": [g * coef for g in grads], "ratio": ratio.detach(),
            "mag": mag + logp_old.abs(), "logp": logp.detach(), "out": out.detach()}


class Adam:
    """Adam with bias correction on fp64 copies: m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g^2,
    p <- p - lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)"""

    def __init__(self, params, lr, b1=0.9, b2=0.999, eps=1e-8):
        self.p = [f64(p).clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.lr, self.b1, self.b2, self.eps, self.t = lr, b1, b2, eps, 0

    def step(self, grads):
        self.t += 1
        for p, m, v, g in zip(self.p, self.m, self.v, grads):
            g = f64(g)
            m.mul_(self.b1).add_((1 - self.b1) * g)
            v.mul_(self.b2).add_((1 - self.b2) * g * g)
            p.sub_(self.lr * (m / (1 - self.b1 ** self.t)) / (torch.sqrt(v / (1 - self.b2 ** self.t)) + self.eps))
        return self.p


def gae(trunc, term, rew, val, boot, lam, gamma):
    """Brax compute_gae as a scalar recursion per env: a truncated step has no temporal-difference error and stops the recursion, a
    terminated one bootstraps with 0; targets vs = acc + V, advantages from vs[t + 1]"""
    trunc, term, rew, val, boot = (f64(t) for t in (trunc, term, rew, val, boot))
    T = rew.shape[0]
    acc = torch.zeros_like(boot)
    vs = torch.zeros_like(val)
    for t in reversed(range(T)):
        vn = boot if t == T - 1 else val[t + 1]
        delta = (rew[t] + gamma * (1 - term[t]) * vn - val[t]) * (1 - trunc[t])
        acc = delta + gamma * lam * (1 - term[t]) * (1 - trunc[t]) * acc
        vs[t] = acc + val[t]
    adv = torch.zeros_like(val)
    for t in range(T):
        vn = boot if t == T - 1 else vs[t + 1]
        adv[t] = (rew[t] + gamma * (1 - term[t]) * vn - val[t]) * (1 - trunc[t])
    return adv, vs


def moments(x):
    """(mean, m2 = sum of squared deviations, count) of the rows of x in fp64"""
    x = f64(x).reshape(-1, x.shape[-1])
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).sum(0), x.shape[0]


def linear_backward_bound(x, dy, K, S):
    """Elementwise worst-case fp32 bound of the split-K weight gradient: one plane is a chain of kc / 2 two-row MFMA steps, the planes are
    added in a chain of Sused, two more roundings for the products: 2 (kc / 2 + Sused + 2) 2^-24 (|dY|^T |X|); the same factor times the
    column sums of |dY| for the bias gradient.  Returns (kc, Sused, bound_dw [N, M], bound_db [N])."""
    kc = (K + S - 1) // S
    kc += kc & 1
    sused = (K + kc - 1) // kc
    f = 2.0 * (kc / 2 + sused + 2) * U32
    ax, ady = f64(x).abs(), f64(dy).abs()
    return kc, sused, f * (ady.T @ ax), f * ady.sum(0)
