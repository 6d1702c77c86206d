"""tests/recurrent_ppo_reference.py held to facts that do not come from the product code: with a zero read-out and one step it is ppo_reference's
feed-forward policy loss; its gradient is the central finite difference of its own total loss; a cleared step cuts the gradient to earlier steps
exactly; the value loss and the global-norm clip are the formulas of the headers.  CPU, fp64, small shapes."""
import math
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_reference as pref  # noqa: E402
import recurrent_policy_reference as rref  # noqa: E402
import recurrent_ppo_reference as ref  # noqa: E402

F64 = torch.float64


def _params(dims, R, seed, w_m=0.3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    P = {"mean": r(dims[0]) * 0.3, "std": torch.rand(dims[0], generator=g, dtype=F64) + 0.5,
         "w": [r(dims[i + 1], dims[i]) / math.sqrt(dims[i]) for i in range(4)], "b": [r(dims[i + 1]) * 0.1 for i in range(4)],
         "w_ih": r(3 * R, dims[3]) / math.sqrt(dims[3]), "w_hh": r(3 * R, R) / math.sqrt(R), "b_ih": r(3 * R) * 0.1, "b_hh": r(3 * R) * 0.1,
         "w_m": r(dims[4], R) * w_m}
    return P


def _value(pd, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    d = (pd,) + tuple(hidden) + (1,)
    return [(torch.randn(d[i + 1], d[i], generator=g, dtype=F64) / math.sqrt(d[i]), torch.randn(d[i + 1], generator=g, dtype=F64) * 0.1) for i in range(4)]


def _minibatch(P, T, B, R, pd, seed, clears=(), spread=0.4):
    """rows like a roll-out's: u sampled from the policy's own heads, logp_old = the policy's logp moved by `spread` (ratios on both sides of 1 +- 0.3),
    advantages of both signs"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    od = P["mean"].shape[0]
    mb = {"obs": P["mean"] + P["std"] * r(T, B, od), "m_init": r(B, R) * 0.5, "clear": torch.zeros(T, B, dtype=torch.bool), "eps": r(T * B, 12),
          "priv": r(T, B, pd), "ret": r(T, B), "adv": r(T, B) * 2 + 0.3, "mean_p": r(pd) * 0.1, "std_p": torch.rand(pd, generator=g, dtype=F64) + 0.5}
    for t, e in clears:
        mb["clear"][t, e] = True
    heads = rref.sequence(P, mb["obs"], mb["m_init"], mb["clear"])["heads"]
    scale = pref.softplus(heads[..., 12:]) + 1e-3
    mb["u"] = heads[..., :12] + scale * r(T, B, 12)
    logp, _ = pref.log_prob(heads.reshape(T * B, 24), mb["u"].reshape(T * B, 12))
    mb["logp_old"] = (logp + r(T * B) * spread).reshape(T, B)
    return mb


DIMS, R, PD = (11, 16, 16, 16, 24), 16, 7


def test_with_a_zero_read_out_and_one_step_it_is_the_feed_forward_policy_loss():
    P = _params(DIMS, R, 1, w_m=0.0)
    V = _value(PD, (8, 8, 8), 2)
    mb = _minibatch(P, 1, 9, R, PD, 3)
    out = ref.update(P, V, mb, clip=0.3, entropy_cost=1e-2)
    head = pref.silu_mlp((mb["obs"][0] - P["mean"]) / P["std"], list(zip(P["w"], P["b"])))
    want = pref.policy_loss(head, mb["u"][0], mb["logp_old"][0], pref.normalise_advantage(mb["adv"][0]), mb["eps"], 0.3, 1e-2)
    assert float((out["heads"] - head).abs().max()) <= 1e-12
    for got, key in zip(out["loss_3"], ("total", "policy", "entropy")):
        assert abs(got - want[key]) <= 1e-12 * max(1.0, abs(want[key])), key
    # d total / d heads: the value loss does not reach the head, so it is the policy loss's gradient
    assert float((out["dhead"] - want["grad"]).abs().max()) <= 1e-13
    r = out["ratio"]
    assert bool((r < 0.7).any()) and bool((r > 1.3).any()) and bool(((r > 0.7) & (r < 1.3)).any())       # both clip sides and the inside are met


def test_value_loss_and_the_global_norm_clip():
    P, V = _params(DIMS, R, 4), _value(PD, (8, 8, 8), 5)
    mb = _minibatch(P, 3, 5, R, PD, 6, clears=[(1, 0), (1, 3)])
    out = ref.update(P, V, mb, max_norm=0.05)
    v = pref.silu_mlp((mb["priv"].reshape(15, PD) - mb["mean_p"]) / mb["std_p"], V).squeeze(-1)
    assert abs(out["value_loss"] - float(0.25 * ((mb["ret"].reshape(-1) - v) ** 2).mean())) <= 1e-14
    assert abs(out["total"] - (out["loss_3"][0] + out["value_loss"])) <= 1e-14 and abs(out["loss_3"][0] - (out["loss_3"][1] - 1e-2 * out["loss_3"][2])) <= 1e-14
    assert len(out["grads"]) == 21 and [tuple(g.shape) for g in out["grads"][:13]] == [tuple(t.shape) for t in ref.policy_tensors(P)]
    norm = math.sqrt(sum(float((g * g).sum()) for g in out["grads"]))
    assert abs(out["grad_norm"] - norm) <= 1e-14 * norm and norm > 0.05
    assert abs(out["clip_coef"] - 0.05 / (norm + 1e-6)) <= 1e-15 and ref.update(P, V, mb, max_norm=1e9)["clip_coef"] == 1.0
    crit = ref.update(P, V, mb, policy=False)
    assert all(float(g.abs().max()) == 0.0 for g in crit["grads"][:13])
    assert all(torch.equal(a, b) for a, b in zip(crit["grads"][13:], out["grads"][13:])) and crit["grad_norm"] < out["grad_norm"]


def test_gradients_are_the_central_differences_of_the_total_loss():
    """20 seeded entries of each of the 21 tensors: |fd - g| <= 1e-6 of the tensor's largest gradient entry.  The minibatch keeps every ratio at least
    1e-3 away from 1 +- clip, so that no step of the difference crosses the kink of the surrogate."""
    P, V = _params(DIMS, R, 7), _value(PD, (8, 8, 8), 8)
    mb = _minibatch(P, 3, 5, R, PD, 9, clears=[(1, 1), (2, 4)])
    out = ref.update(P, V, mb)
    assert float(torch.minimum((out["ratio"] - 0.7).abs(), (out["ratio"] - 1.3).abs()).min()) > 1e-3
    tensors = ref.policy_tensors(P) + [t for wb in V for t in wb]
    names = ref.POLICY_NAMES + ref.VALUE_NAMES

    def total():
        return float(ref.losses(ref.with_tensors(P, tensors[:13]), [(tensors[13 + 2 * i], tensors[14 + 2 * i]) for i in range(4)], mb)["total"])
    h = 1e-5
    gen = torch.Generator().manual_seed(10)
    for name, t, g in zip(names, tensors, out["grads"]):
        flat, gf = t.view(-1), g.reshape(-1)
        scale = float(gf.abs().max())
        assert scale > 0, name
        for k in torch.randint(0, flat.numel(), (20,), generator=gen).tolist():
            keep = float(flat[k])
            flat[k] = keep + h
            up = total()
            flat[k] = keep - h
            down = total()
            flat[k] = keep
            fd = (up - down) / (2 * h)
            assert abs(fd - float(gf[k])) <= 1e-6 * scale, (name, k, fd, float(gf[k]))


# the shapes at which the GPU tests lean on this reference: a long unroll at the largest memory, no recurrence at all, a cut at the last step
SHAPES = {"T20_B7_R256": (20, 7, 256), "T1_all_cleared": (1, 6, 48), "T2_all_cleared_at_1": (2, 5, 80)}


def _shape_clears(shape, T, B):
    if shape == "T20_B7_R256":                                                         # at t = 0, in the last row, at every step of one env, the rest never
        return [(0, 0), (T - 1, 1)] + [(t, 2) for t in range(T)]
    return [(0 if shape == "T1_all_cleared" else 1, e) for e in range(B)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_update_is_the_hand_written_bptt_at_the_shapes_the_gpu_tests_use(shape):
    """update()'s gradients are autograd's through rref.sequence; rref.bptt is the recurrence by hand.  Fed update()'s own d total / d heads, the two agree
    on the thirteen policy tensors to the 1e-9 that test_recurrent_policy_reference.py asks of bptt, and the heads to 1e-12."""
    T, B, R_ = SHAPES[shape]
    dims = (11, 16, 16, 16, 24)
    P, V = _params(dims, R_, 21), _value(PD, (8, 8, 8), 22)
    mb = _minibatch(P, T, B, R_, PD, 23, clears=_shape_clears(shape, T, B))
    out = ref.update(P, V, mb)
    by_hand = rref.bptt(P, mb["obs"], mb["m_init"], mb["clear"], out["dhead"].reshape(T, B, 24))
    assert float((by_hand["heads"].reshape(T * B, 24) - out["heads"]).abs().max()) <= 1e-12
    for name, a, g in zip(ref.POLICY_NAMES, rref.flat_grads(by_hand), out["grads"][:13]):
        assert a.shape == g.shape and float((a - g).norm()) <= 1e-9 * float(g.norm()), name
        if shape == "T1_all_cleared" and name == "w_hh":                                # m0 = 0 in every row: exactly zero, by hand and by autograd
            assert bool((a == 0).all()) and bool((g == 0).all())
        else:
            assert float(g.norm()) > 1e-4, name
    assert all(float(g.norm()) > 1e-4 for g in out["grads"][13:]) and len(out["grads"]) == 21


@pytest.mark.parametrize("shape", ["T1_all_cleared", "T2_all_cleared_at_1"])
def test_gradients_are_the_central_differences_where_every_env_is_cleared(shape):
    """the check of test_gradients_are_the_central_differences_of_the_total_loss, 10 seeded entries per tensor, at the two shapes with an all-cleared step;
    W_hh at T = 1 has a zero gradient and a zero difference"""
    T, B, R_ = SHAPES[shape]
    P, V = _params(DIMS, R_, 31), _value(PD, (8, 8, 8), 32)
    mb = _minibatch(P, T, B, R_, PD, 33, clears=_shape_clears(shape, T, B))
    out = ref.update(P, V, mb)
    assert float(torch.minimum((out["ratio"] - 0.7).abs(), (out["ratio"] - 1.3).abs()).min()) > 1e-3
    tensors = ref.policy_tensors(P) + [t for wb in V for t in wb]

    def total():
        return float(ref.losses(ref.with_tensors(P, tensors[:13]), [(tensors[13 + 2 * i], tensors[14 + 2 * i]) for i in range(4)], mb)["total"])
    h = 1e-5
    gen = torch.Generator().manual_seed(34)
    for name, t, g in zip(ref.POLICY_NAMES + ref.VALUE_NAMES, tensors, out["grads"]):
        flat, gf = t.view(-1), g.reshape(-1)
        scale = float(gf.abs().max())
        assert (scale == 0) == (shape == "T1_all_cleared" and name == "w_hh"), name
        for k in torch.randint(0, flat.numel(), (10,), generator=gen).tolist():
            keep = float(flat[k])
            flat[k] = keep + h
            up = total()
            flat[k] = keep - h
            down = total()
            flat[k] = keep
            assert abs((up - down) / (2 * h) - float(gf[k])) <= 1e-6 * scale, (name, k)


def test_a_cleared_step_cuts_the_gradient_to_earlier_steps_exactly():
    P = _params(DIMS, R, 11)
    mb = _minibatch(P, 3, 4, R, PD, 12, clears=[(2, 1), (1, 3)])
    obs, m_init = mb["obs"].clone().requires_grad_(True), mb["m_init"].clone().requires_grad_(True)
    heads = rref.sequence(P, obs, m_init, mb["clear"])["heads"]
    d_obs, d_m = torch.autograd.grad(heads[2].sum(), [obs, m_init])
    # env 1 is cleared at t = 2, env 3 at t = 1: the last step's head reaches nothing before the clear, exactly
    assert float(d_obs[:2, 1].abs().max()) == 0.0 and float(d_m[1].abs().max()) == 0.0
    assert float(d_obs[0, 3].abs().max()) == 0.0 and float(d_m[3].abs().max()) == 0.0 and float(d_obs[1, 3].abs().max()) > 0
    for e in (0, 2):                                                                   # an env that is not cleared carries it back to the start
        assert float(d_obs[0, e].abs().max()) > 0 and float(d_m[e].abs().max()) > 0
    # and the same through the whole update: the rows of env 1 at t < 2 reach the loss through their own heads only
    V = _value(PD, (8, 8, 8), 13)
    a = ref.update(P, V, mb)
    moved = dict(mb, m_init=mb["m_init"].clone())
    moved["m_init"][3] += 1.0                                                          # cleared at t = 1: only its t = 0 head moves
    b = ref.update(P, V, moved)
    ha, hb = a["heads"].view(3, 4, 24), b["heads"].view(3, 4, 24)
    assert not torch.equal(ha[0, 3], hb[0, 3]) and torch.equal(ha[1:, 3], hb[1:, 3]) and torch.equal(ha[:, :3], hb[:, :3])
