"""An fp64 statement of the recurrent policy (include/pgtt_learn.h), written from the header's formulas and from nothing in
recurrent_policy.py: the acting step, the sequence with its clears, and truncated back-propagation through time by hand.  A helper module like
distill_reference.py: test_recurrent_policy_reference.py holds it to torch.nn.GRUCell and to autograd on the CPU, the GPU tests hold the
product code to it.  Everything is torch.float64 on the CPU.

    P = dict(mean, std, w = [W0..W3] ([out, in]), b = [b0..b3], w_ih [3R, h3], w_hh [3R, R], b_ih [3R], b_hh [3R], w_m [24, R])
    x  = (obs - mean) / std;  h1 = silu(W0 x + b0);  h2 = silu(W1 h1 + b1);  h3 = silu(W2 h2 + b2)
    m0 = clear ? 0 : m_prev
    gi = W_ih h3 + b_ih (r | u | n);   gh = W_hh m0 + b_hh
    r  = sigmoid(gi_r + gh_r);  u = sigmoid(gi_u + gh_u);  n = tanh(gi_n + r gh_n);   m1 = (1 - u) n + u m0
    head = W3 h3 + b3 + W_m m1

Backward, per step from the last: dm1 = dhead W_m + (dm0 of the step after, zero where that step was cleared, absent at the last step);
    dn = dm1 (1 - u),  du = dm1 (m0 - n),  dpre_n = dn (1 - n^2),  dpre_u = du u (1 - u),  dr = gh_n dpre_n,  dpre_r = dr r (1 - r)
    dgi = (dpre_r | dpre_u | dpre_n),  dgh = (dpre_r | dpre_u | r dpre_n),  dm0 = u dm1 + dgh W_hh
    dh3 = (dhead W3) silu'(z3) + (dgi W_ih) silu'(z3)        the factor once per addend, as the product code applies it
m_init gets no gradient: the sequence is truncated at the unroll's start.
"""
import torch

F64 = torch.float64
U32 = 2.0 ** -24
KEYS = ("w_ih", "w_hh", "b_ih", "b_hh", "w_m")


def f64(x):
    return x.detach().to("cpu", F64)


def params64(P):
    out = {k: f64(P[k]) for k in ("mean", "std") + KEYS}
    out["w"], out["b"] = [f64(w) for w in P["w"]], [f64(b) for b in P["b"]]
    return out


def silu(z):
    return z * torch.sigmoid(z)


def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def cell(gi, gh, m0):
    """-> (r, u, n, m1), every one [.., R]"""
    R = m0.shape[-1]
    r = torch.sigmoid(gi[..., :R] + gh[..., :R])
    u = torch.sigmoid(gi[..., R:2 * R] + gh[..., R:2 * R])
    n = torch.tanh(gi[..., 2 * R:] + r * gh[..., 2 * R:])
    return r, u, n, (1 - u) * n + u * m0


def trunk(P, obs):
    """-> (x, [z1, z2, z3], [h1, h2, h3])"""
    x = (obs - P["mean"]) / P["std"]
    zs, hs, h = [], [], x
    for w, b in zip(P["w"][:3], P["b"][:3]):
        z = h @ w.T + b
        h = silu(z)
        zs.append(z); hs.append(h)
    return x, zs, hs


def step(P, obs, mem, clear):
    """one acting step -> dict(action, head, mem (m1), m0, h3, gi, gh, r, u, n); clear is a bool [N]; a cleared row of mem is not read"""
    P = params64(P)
    obs = f64(obs)
    _, _, hs = trunk(P, obs)
    h3 = hs[-1]
    c = clear.to("cpu").bool()[:, None]
    m0 = torch.where(c, torch.zeros((), dtype=F64), f64(mem))
    gi, gh = h3 @ P["w_ih"].T + P["b_ih"], m0 @ P["w_hh"].T + P["b_hh"]
    r, u, n, m1 = cell(gi, gh, m0)
    head = h3 @ P["w"][3].T + P["b"][3] + m1 @ P["w_m"].T
    return {"action": torch.tanh(head[:, :12]), "head": head, "mem": m1, "m0": m0, "h3": h3, "gi": gi, "gh": gh, "r": r, "u": u, "n": n}


def sequence(P, obs, m_init, clear):
    """obs [T, B, od], m_init [B, R], clear bool [T, B] -> dict of per-step caches and heads [T, B, 24]; P already fp64"""
    T = obs.shape[0]
    x, zs, hs = trunk(P, obs)
    h3 = hs[-1]
    gi = h3 @ P["w_ih"].T + P["b_ih"]
    prev, steps, heads = m_init, [], []
    for t in range(T):
        m0 = torch.where(clear[t][:, None], torch.zeros((), dtype=F64), prev)
        gh = m0 @ P["w_hh"].T + P["b_hh"]
        r, u, n, m1 = cell(gi[t], gh, m0)
        heads.append(h3[t] @ P["w"][3].T + P["b"][3] + m1 @ P["w_m"].T)
        steps.append({"m0": m0, "gh": gh, "r": r, "u": u, "n": n, "m1": m1})
        prev = m1
    return {"x": x, "zs": zs, "hs": hs, "gi": gi, "steps": steps, "heads": torch.stack(heads)}


def cell_backward(s, dm1):
    """the point-wise part of one step's backward: s = a step's cache -> (dgi, dgh, the direct part u dm1 of dm0)"""
    r, u, n, m0 = s["r"], s["u"], s["n"], s["m0"]
    R = m0.shape[-1]
    dn, du = dm1 * (1 - u), dm1 * (m0 - n)
    dpn, dpu = dn * (1 - n * n), du * u * (1 - u)
    dr = s["gh"][..., 2 * R:] * dpn
    dpr = dr * r * (1 - r)
    return torch.cat([dpr, dpu, dpn], -1), torch.cat([dpr, dpu, r * dpn], -1), u * dm1


def bptt(P, obs, m_init, clear, dheads):
    """the gradient of sum(heads * dheads) by hand -> dict: "w" / "b" lists and the five KEYS; obs [T, B, od], dheads [T, B, 24]"""
    P = params64(P)
    obs, m_init, dheads, clear = f64(obs), f64(m_init), f64(dheads), clear.to("cpu").bool()
    T, B = obs.shape[:2]
    c = sequence(P, obs, m_init, clear)
    h3 = c["hs"][-1]
    R = m_init.shape[1]
    dgi, dgh = torch.zeros(T, B, 3 * R, dtype=F64), torch.zeros(T, B, 3 * R, dtype=F64)
    dm0_next = None
    for t in range(T - 1, -1, -1):
        dm1 = dheads[t] @ P["w_m"]
        if dm0_next is not None:
            dm1 = dm1 + torch.where(clear[t + 1][:, None], torch.zeros((), dtype=F64), dm0_next)
        dgi[t], dgh[t], direct = cell_backward(c["steps"][t], dm1)
        dm0_next = direct + dgh[t] @ P["w_hh"]
    rows = lambda a: a.reshape(T * B, -1)
    m0_all, m1_all = torch.stack([s["m0"] for s in c["steps"]]), torch.stack([s["m1"] for s in c["steps"]])
    g = {"w": [None] * 4, "b": [None] * 4}
    g["w_m"] = rows(dheads).T @ rows(m1_all)
    g["w"][3], g["b"][3] = rows(dheads).T @ rows(h3), rows(dheads).sum(0)
    g["w_ih"], g["b_ih"] = rows(dgi).T @ rows(h3), rows(dgi).sum(0)
    g["w_hh"], g["b_hh"] = rows(dgh).T @ rows(m0_all), rows(dgh).sum(0)
    fac = dsilu(c["zs"][2])
    dz = (dheads @ P["w"][3]) * fac + (dgi @ P["w_ih"]) * fac
    inputs = [c["x"], c["hs"][0], c["hs"][1]]
    for i in (2, 1, 0):
        g["w"][i], g["b"][i] = rows(dz).T @ rows(inputs[i]), rows(dz).sum(0)
        if i > 0:
            dz = (dz @ P["w"][i]) * dsilu(c["zs"][i - 1])
    g["heads"] = c["heads"]
    return g


def flat_grads(g):
    """the gradient tensors in the order of RecurrentPolicy.parameters(): w0, b0, .., w3, b3, w_ih, w_hh, b_ih, b_hh, w_m"""
    return [t for i in range(4) for t in (g["w"][i], g["b"][i])] + [g[k] for k in KEYS]


def update(P, obs, m_init, clear, labels):
    """one distillation update over whole unrolls in fp64: the loss of distill_reference.loss over the T B rows (t-major) and its gradient by bptt
    -> dict(loss_2, grads (flat_grads order), grad_norm, heads)"""
    import distill_reference as dref
    P64 = params64(P)
    T, B = obs.shape[:2]
    heads = sequence(P64, f64(obs), f64(m_init), clear.to("cpu").bool())["heads"]
    l2, dh = dref.loss(heads.reshape(T * B, -1), f64(labels).reshape(T * B, -1))
    g = bptt(P, obs, m_init, clear, dh.reshape(T, B, -1))
    grads = flat_grads(g)
    return {"loss_2": l2, "grads": grads, "grad_norm": float(torch.sqrt(sum((x * x).sum() for x in grads))), "heads": heads}
