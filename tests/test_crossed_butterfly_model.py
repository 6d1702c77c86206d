"""A numpy float32 model of the line search's row sums in their two forms (QSolver::ls_points, pair_sum2).

REPLICATED (before): every lane of an env holds the trial steps in END order - slot 0 `lo`'s Newton step, slot 1 `hi`'s, slot 2 the midpoint - sums each
slot over the env's lanes by the full butterfly, and a lane of role r (= lane & 1) picks (slot r, slot 1 - r, slot 2) as (own, partner, midpoint).
CROSSED (now): a lane holds the steps in ROLE order - slot 0 its own end's step, slot 1 the partner's - and the first butterfly step, the one that
pairs lane and lane ^ 1, adds slot 0 to the partner's slot 1 and slot 1 to the partner's slot 0; the later steps and the midpoint are the same.

The claim: both give every lane the same (own, partner, midpoint) bits, for finite operands (the two addends of every add are the same, in either order),
and lanes of equal role agree.  Where a sum is NaN (inf - inf) both forms are NaN; NaN payloads are outside the claim, as they were between the two
lanes of a pair before.  This documents the argument; tests/test_gpu_linesearch_crossed.py holds the kernel to it."""
import numpy as np
import pytest

f32 = np.float32


def _xor(k):
    return [l ^ k for l in range(16)]


def _ror(n):          # row_ror:n - lane l reads lane (l - n) mod 16 of its row
    return [(l - n) % 16 for l in range(16)]


# one 16-lane DPP row per layout: the source lane of every butterfly step (the first one is quad_perm [1,0,3,2] in all three), and the env of a lane
LAYOUTS = {
    "hex": dict(steps=[_xor(1), _xor(2), _ror(8), _ror(4)], env=[0] * 16),                           # 4 sub-lanes x 4 legs, one env per row
    "oct": dict(steps=[_xor(1), _ror(8), _ror(4)], env=[(l >> 1) & 1 for l in range(16)]),           # 2 sub-lanes x 4 legs, two envs per row
    "quad": dict(steps=[_xor(1), _xor(2)], env=[l >> 2 for l in range(16)]),                         # 4 legs, four envs per row
}


def _step(x, src):
    with np.errstate(invalid="ignore", over="ignore"):
        return (x + x[..., src]).astype(f32)


def replicated(p, steps):
    """p [..., 3 (lo's step, hi's step, midpoint), 16 lanes] -> per lane (own, partner, midpoint) [..., 3, 16]"""
    s = p
    for src in steps:
        s = _step(s, src)
    role = np.arange(16) & 1
    own = np.where(role == 1, s[..., 1, :], s[..., 0, :])
    par = np.where(role == 1, s[..., 0, :], s[..., 1, :])
    return np.stack([own, par, s[..., 2, :]], -2)


def crossed(p, steps):
    role = np.arange(16) & 1
    x0 = np.where(role == 1, p[..., 1, :], p[..., 0, :])         # the partial at the own end's step
    x1 = np.where(role == 1, p[..., 0, :], p[..., 1, :])         # the partial at the partner's step
    with np.errstate(invalid="ignore", over="ignore"):
        s0 = (x0 + x1[..., steps[0]]).astype(f32)
        s1 = (x1 + x0[..., steps[0]]).astype(f32)
    mid = _step(p[..., 2, :], steps[0])
    for src in steps[1:]:
        s0, s1, mid = _step(s0, src), _step(s1, src), _step(mid, src)
    return np.stack([s0, s1, mid], -2)


def _inputs():
    rng = np.random.default_rng(7)
    n = 1024
    p = (rng.normal(size=(n, 3, 16)) * np.exp(rng.uniform(-30, 30, size=(n, 3, 16)))).astype(f32)
    sp = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, 3.4028235e38, -3.4028235e38, 1.0, -1.0, 16777216.0, 1.0000001], f32)
    k = n // 4
    p[:k] = sp[rng.integers(0, len(sp), size=(k, 3, 16))]                           # +-0, denormals, the largest finite values
    q = p[k:2 * k]                                                                   # values that cancel: half of the lanes hold the others' negatives
    q[..., 8:] = -q[..., rng.permutation(8)]
    q[::3, :, 5] += f32(1e-3) * q[::3, :, 2]
    inf = p[2 * k:3 * k]                                                       # +-inf
    sel = rng.random(inf.shape) < 0.1
    inf[sel] = np.where(rng.random(int(sel.sum())) < 0.5, np.inf, -np.inf).astype(f32)
    return p


P = _inputs()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_crossed_sums_are_the_replicated_sums(layout):
    L = LAYOUTS[layout]
    a, b = replicated(P, L["steps"]), crossed(P, L["steps"])
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb)
    assert na.any() and not na[-256:].any(), "inf - inf occurs among the special rows, never among the plain random ones"
    same = (a.view(np.uint32) == b.view(np.uint32)) | na
    assert same.all(), (layout, int((~same).sum()))
    assert np.isinf(a).any() and (a == 0).any()
    # lanes of equal role (and of one env) agree, in both forms
    env, role = np.array(L["env"]), np.arange(16) & 1
    for x in (a, b):
        for e in np.unique(env):
            for r in (0, 1):
                lanes = np.nonzero((env == e) & (role == r))[0]
                ref = x[..., lanes[:1]]
                assert (((x[..., lanes].view(np.uint32) == ref.view(np.uint32)) | np.isnan(ref))).all(), (layout, e, r)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_sum_stays_within_its_env(layout):
    """the model's lane maps are the kernel's: no step of a layout reads a lane of another env, and every lane of the env is reached"""
    L = LAYOUTS[layout]
    env = np.array(L["env"])
    reach = np.eye(16, dtype=bool)
    for src in L["steps"]:
        assert (env[src] == env).all()
        reach = reach | reach[src]
    assert np.array_equal(reach, env[:, None] == env[None, :])


def test_the_crossed_step_is_what_makes_the_difference():
    """a plain first step on role-ordered slots would mix the two ends: the model can tell the forms apart"""
    L = LAYOUTS["hex"]
    role = np.arange(16) & 1
    x0 = np.where(role == 1, P[..., 1, :], P[..., 0, :])
    s = x0
    for src in L["steps"]:
        s = _step(s, src)
    a = replicated(P, L["steps"])
    fin = np.isfinite(a[..., 0, :]) & np.isfinite(s)
    assert (s[fin] != a[..., 0, :][fin]).any()
