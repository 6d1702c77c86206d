"""An fp64 statement of the policy-distillation loss, its gradient and the row gather, written from the formulas in include/pgtt_learn.h
(pgtt_learn_distill_loss, pgtt_learn_gather_rows) and from nothing in distill.py.  A helper module like ppo_reference.py: test_distill_reference.py
holds it to facts of its own on the CPU, test_gpu_distill_kernels.py / test_gpu_distill.py hold the product code to it.  Everything is
torch.float64 on the CPU.

    head = (loc | raw), [B, 2A];   sigma = softplus(raw) + 1e-3,   softplus(r) = max(r, 0) + log1p(exp(-|r|))
    d = loc_t - loc_s,   q = (sigma_t^2 + d^2) / sigma_s^2
    KL = log(sigma_s / sigma_t) + 0.5 (q - 1)                                   KL(teacher || student), per row and dimension
    loss = (1 / B) sum_i sum_a KL,   action error = (1 / (B A)) sum (tanh loc_s - tanh loc_t)^2
    dloss / dloc_s = -d / sigma_s^2 / B,   dloss / draw_s = (1 - q) / sigma_s sigmoid(raw_s) / B
"""
import torch

F64 = torch.float64
U32 = 2.0 ** -24          # unit roundoff of fp32
EPS_SIGMA = 1e-3


def f64(x):
    return x.detach().to("cpu", F64)


def softplus(r):
    return torch.clamp(r, min=0.0) + torch.log1p(torch.exp(-r.abs()))


def sigma(raw):
    return softplus(raw) + EPS_SIGMA


def split(head):
    A = head.shape[-1] // 2
    return head[..., :A], head[..., A:]


def terms(student, teacher):
    """the pieces the loss and its gradient are made of, per row and dimension: a dict of [B, A] tensors
    d, ss (sigma_s), st (sigma_t), q, log (log(sigma_s / sigma_t)), kl, sig (sigmoid(raw_s))"""
    ls, rs = split(f64(student))
    lt, rt = split(f64(teacher))
    ss, st = sigma(rs), sigma(rt)
    d = lt - ls
    q = (st * st + d * d) / (ss * ss)
    lg = torch.log(ss / st)
    return {"d": d, "ss": ss, "st": st, "q": q, "log": lg, "kl": lg + 0.5 * (q - 1.0), "sig": torch.sigmoid(rs)}


def loss(student, teacher):
    """-> (loss_2 [2], grad [B, 2A]): the mean over rows of the KL summed over dimensions, the mean squared error of the deterministic action,
    and the gradient of the first with respect to the student head"""
    t = terms(student, teacher)
    B, A = t["d"].shape
    ls, lt = split(f64(student))[0], split(f64(teacher))[0]
    kl = t["kl"].sum() / B
    act = ((torch.tanh(ls) - torch.tanh(lt)) ** 2).sum() / (B * A)
    g_loc = -t["d"] / (t["ss"] * t["ss"]) / B
    g_raw = (1.0 - t["q"]) / t["ss"] * t["sig"] / B
    return torch.stack([kl, act]), torch.cat([g_loc, g_raw], -1)


def gather_rows(idx, obs, target, mean, std):
    """-> (x [B, obs_dim], y [B, tgt_dim]) for the rows idx clamped into [0, rows)"""
    r = idx.to("cpu").long().clamp(0, obs.shape[0] - 1)
    return (f64(obs)[r] - f64(mean)) / f64(std), f64(target)[r]


def update(policy, mean, std, obs, labels):
    """One distillation minibatch in fp64: policy = [(W [out, in], b [out])] x 4 (any dtype), obs [B, obs_dim] raw rows, labels [B, 2A] teacher
    heads.  -> dict(loss_2, grads: the UNCLIPPED gradient of every tensor in the order W0, b0, ..., W3, b3, grad_norm, head)"""
    import ppo_reference as ref
    pol = [(f64(w).requires_grad_(True), f64(b).requires_grad_(True)) for w, b in policy]
    x = (f64(obs) - f64(mean)) / f64(std)
    head = ref.silu_mlp(x, pol)
    l2, g = loss(head.detach(), labels)
    head.backward(g)
    grads = [t.grad for wb in pol for t in wb]
    norm = float(torch.sqrt(sum((g * g).sum() for g in grads)))
    return {"loss_2": l2, "grads": grads, "grad_norm": norm, "head": head.detach()}
