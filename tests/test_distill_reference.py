"""tests/distill_reference.py held to facts of its own, on the CPU: the KL of two diagonal Gaussians as torch.distributions states it, its
gradient as torch autograd gives it, its sign and its zero, the softplus form at large arguments, the gather."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distill_reference as dref  # noqa: E402

F64 = torch.float64


def _heads(B, A, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    s = torch.cat([r(B, A) * spread, r(B, A) * 2 - 1], -1)
    t = torch.cat([r(B, A) * spread, r(B, A) * 2 - 1], -1)
    return s, t


def _torch_kl(student, teacher):
    """KL(teacher || student) through torch.distributions, summed over A and averaged over B; sigma by F.softplus without its threshold"""
    from torch.distributions import Normal, kl_divergence
    ls, rs = dref.split(student)
    lt, rt = dref.split(teacher)
    sp = lambda r: torch.nn.functional.softplus(r, threshold=1e9) + 1e-3
    return kl_divergence(Normal(lt, sp(rt)), Normal(ls, sp(rs))).sum(-1).mean()


@pytest.mark.parametrize("B,A", [(1, 1), (7, 12), (65, 12)])
def test_value_is_the_kl_divergence_of_torch_distributions(B, A):
    s, t = _heads(B, A, B + A)
    l2, _ = dref.loss(s, t)
    want = _torch_kl(s, t)
    assert abs(float(l2[0]) - float(want)) <= 1e-12 * (1 + abs(float(want)))
    ls, lt = dref.split(s)[0], dref.split(t)[0]
    assert abs(float(l2[1]) - float(((torch.tanh(ls) - torch.tanh(lt)) ** 2).mean())) <= 1e-14


@pytest.mark.parametrize("B,A", [(1, 1), (7, 12), (65, 12)])
def test_gradient_is_autograd_of_that_expression(B, A):
    s, t = _heads(B, A, 3 * B + A)
    s = s.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(_torch_kl(s, t), s)
    _, g = dref.loss(s.detach(), t)
    assert g.shape == want.shape
    assert float((g - want).abs().max()) <= 1e-12 * (1 + float(want.abs().max()))


def test_kl_is_nonnegative_and_zero_with_zero_gradient_at_equal_heads():
    s, t = _heads(257, 12, 5, spread=3.0)
    k = dref.terms(s, t)["kl"]
    assert bool((k >= 0).all()) and float(k.min()) > 0
    l2, g = dref.loss(t, t)
    assert l2.tolist() == [0.0, 0.0] and bool((g == 0).all())
    k = dref.terms(t, t)
    assert bool((k["kl"] == 0).all()) and bool((k["q"] == 1).all())


def test_softplus_form_is_finite_at_large_arguments():
    raw = torch.tensor([-88.0, 88.0, -20.0, 20.0, 0.0], dtype=F64)
    sp = dref.softplus(raw)
    assert bool(torch.isfinite(sp).all()) and bool((sp > 0).all())
    assert float(sp[1]) == 88.0 and abs(float(sp[4]) - 0.6931471805599453) <= 1e-15 and abs(float(sp[0]) - 6.054601895401186e-39) <= 1e-50
    # the whole loss at those scales, student against teacher in every pairing, with an offset of 10 in the mean
    A = raw.numel()
    s = torch.cat([torch.full((A, A), 10.0, dtype=F64), raw[None].expand(A, A)], -1)
    t = torch.cat([torch.zeros(A, A, dtype=F64), raw[:, None].expand(A, A)], -1)
    l2, g = dref.loss(s, t)
    assert bool(torch.isfinite(l2).all()) and bool(torch.isfinite(g).all())
    assert abs(float(l2[0]) - float(_torch_kl(s, t))) <= 1e-12 * float(l2[0])


def test_gather_rows_clamps_and_normalises():
    g = torch.Generator().manual_seed(1)
    obs, tgt = torch.randn(10, 3, generator=g), torch.randn(10, 2, generator=g)
    mean, std = torch.randn(3, generator=g), torch.rand(3, generator=g) + 0.5
    idx = torch.tensor([-4, 0, 9, 12, 3])
    x, y = dref.gather_rows(idx, obs, tgt, mean, std)
    rows = [0, 0, 9, 9, 3]
    assert torch.equal(y, tgt[rows].double())
    assert torch.equal(x, (obs[rows].double() - mean.double()) / std.double())


def test_update_is_the_chain_rule_through_the_mlp():
    """dref.update's parameter gradients equal autograd of the loss through the MLP as one expression"""
    import ppo_reference as ref
    g = torch.Generator().manual_seed(2)
    dims = (5, 7, 6, 4, 6)
    pol = [(torch.randn(dims[i + 1], dims[i], generator=g, dtype=F64) * 0.5, torch.randn(dims[i + 1], generator=g, dtype=F64) * 0.1) for i in range(4)]
    obs, labels = torch.randn(9, 5, generator=g, dtype=F64), torch.randn(9, 6, generator=g, dtype=F64)
    mean, std = torch.randn(5, generator=g, dtype=F64), torch.rand(5, generator=g, dtype=F64) + 0.5
    got = dref.update(pol, mean, std, obs, labels)
    leaves = [(w.clone().requires_grad_(True), b.clone().requires_grad_(True)) for w, b in pol]
    total = _torch_kl(ref.silu_mlp((obs - mean) / std, leaves), labels)
    want = torch.autograd.grad(total, [t for wb in leaves for t in wb])
    total = total.detach()
    assert abs(float(got["loss_2"][0]) - float(total)) <= 1e-12 * (1 + float(total))
    for a, b in zip(got["grads"], want):
        assert float((a - b).abs().max()) <= 1e-12 * (1 + float(b.abs().max()))
