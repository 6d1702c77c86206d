"""The kernels of libpgtt_learn.so one by one, through the bare C ABI (include/pgtt_learn.h), at edge shapes against fp64 (tests/ppo_reference.py where
it states the operation).  Every output handed to a kernel is a view into a larger allocation filled with a sentinel, at an odd float offset, with
guard bands in front of and behind it.  Every bar is derived from the operation count with u = 2^-24; none is fitted to the kernel."""
import ctypes as C
import itertools
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_reference as ref  # noqa: E402

from phase_guided_terrain_traversal_amd import learn, ppo  # noqa: E402

U = 2.0 ** -24
SENT = 777.0
E_ARG = -1
F64 = torch.float64


class Guarded:
    """a tensor that is a view into a larger allocation of sentinels: guard bands of odd lengths in front of and behind it"""

    def __init__(self, *shape, dtype=torch.float32, fill=SENT, front=19, back=23):
        self.n, self.front, self.fill = 1, front, fill
        for s in shape:
            self.n *= int(s)
        self.big = torch.full((front + self.n + back,), fill, dtype=dtype, device="cuda")
        self.view = self.big[front:front + self.n].view(*shape)

    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        return bool((self.big[:self.front] == self.fill).all()) and bool((self.big[self.front + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.big == self.fill).all())

    def written(self):
        """guards intact and no sentinel left inside (the tests' values never equal the sentinel)"""
        return self.guards_intact() and bool((self.view != self.fill).all())

    def f64(self):
        return self.view.detach().to("cpu", F64)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def _ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def forward(x, w, b, K, M, N, act, y, z):
    return learn.lib().pgtt_learn_linear_forward(_p(x), _p(w), _p(b), K, M, N, act, _p(y), _p(z), _st())


def backward_data(dy, w, zp, K, M, N, dx):
    return learn.lib().pgtt_learn_linear_backward_data(_p(dy), _p(w), _p(zp), K, M, N, _p(dx), _st())


KS, MS, NS = (1, 15, 16, 17, 63, 64, 65, 257), (1, 3, 4, 5, 171, 215, 512), (1, 15, 16, 17, 24, 128)
# the trainer's layers (in, out): policy then value; the hidden ones are those whose input needs a gradient
LAYERS = ((171, 512), (512, 256), (256, 128), (128, 24), (215, 512), (512, 256), (256, 128), (128, 1))
HIDDEN = ((512, 256), (256, 128), (128, 24), (512, 256), (256, 128), (128, 1))


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("M", MS)
def test_forward_integers_are_exact(M):
    """X, W, b integers in [-3, 3], act = 0: every product and every partial sum is an integer below 9 * 512 + 3 < 2^24, so the output equals the
    integer product as bits whatever the order of the sum; once more with Z requested: Z == Y as bits"""
    g = torch.Generator().manual_seed(M)
    for K, N in itertools.product(KS, NS):
        x, w, b = _ints(g, -3, 3, K, M).cuda(), _ints(g, -3, 3, N, M).cuda(), _ints(g, -3, 3, N).cuda()
        want = (x.double() @ w.double().T + b.double()).float()
        y = Guarded(K, N)
        assert forward(x, w, b, K, M, N, 0, y, None) == 0
        assert y.guards_intact() and torch.equal(y.view, want), (K, M, N, float((y.view - want).abs().max()))
        y2, z2 = Guarded(K, N), Guarded(K, N, front=21, back=17)
        assert forward(x, w, b, K, M, N, 0, y2, z2) == 0
        assert y2.guards_intact() and z2.guards_intact() and torch.equal(y2.view, want) and torch.equal(z2.view, want), (K, M, N)


def _forward_bars(x, w, b):
    x64, w64, b64 = ref.f64(x), ref.f64(w), ref.f64(b)
    z64 = x64 @ w64.T + b64
    zbar = (x.shape[1] + 2) * U * (x64.abs() @ w64.abs().T + b64.abs())          # an M-term fp32 dot product in any order, and the bias
    y64 = z64 * torch.sigmoid(z64)
    ybar = 1.1 * zbar + 6 * U * y64.abs() + 1e-37                                 # |silu'| <= 1.1; one expf at 2 ulp, one add, one divide
    return z64, zbar, y64, ybar


@pytest.mark.parametrize("K,M,N", [(320, m, n) for m, n in LAYERS] + [(5120, 171, 512)])
def test_forward_rounding(K, M, N):
    g = torch.Generator().manual_seed(K + M + N)
    x, w, b = torch.randn(K, M, generator=g).cuda(), (torch.randn(N, M, generator=g) * M ** -0.5).cuda(), (torch.randn(N, generator=g) * 0.3).cuda()
    z64, zbar, y64, ybar = _forward_bars(x, w, b)
    y, z = Guarded(K, N), Guarded(K, N, front=21, back=17)
    assert forward(x, w, b, K, M, N, 1, y, z) == 0
    assert y.written() and z.written()
    rz, ry = ((z.f64() - z64).abs() / zbar).max(), ((y.f64() - y64).abs() / ybar).max()
    print(f"forward {K}x{M}->{N}: worst |Z - Z64| / bar {float(rz):.3f}, worst |Y - silu(Z64)| / bar {float(ry):.3f}")
    assert float(rz) <= 1.0 and float(ry) <= 1.0
    y0 = Guarded(K, N)
    assert forward(x, w, b, K, M, N, 0, y0, None) == 0                            # act = 0: Y is Z, the same bits
    assert y0.guards_intact() and torch.equal(y0.view, z.view)


def test_forward_silu_at_large_arguments():
    """W = 0 and b = the wanted pre-activation, so Z == b exactly: silu neither overflows nor returns NaN at +-100, +-20, 0"""
    vals = [-100.0, -20.0, 0.0, 20.0, 100.0, -88.0, 88.5, -1.2785, 1e-30, -1e-30]
    N, M, K = len(vals), 5, 17
    x, w, b = torch.randn(K, M).cuda(), torch.zeros(N, M).cuda(), torch.tensor(vals).cuda()
    y, z = Guarded(K, N), Guarded(K, N)
    assert forward(x, w, b, K, M, N, 1, y, z) == 0
    assert y.guards_intact() and z.guards_intact() and torch.equal(z.view, b.expand(K, N))
    assert bool(torch.isfinite(y.view).all())
    z64 = ref.f64(b).expand(K, N)
    y64 = z64 * torch.sigmoid(z64)
    assert bool(((y.f64() - y64).abs() <= 6 * U * y64.abs() + 1e-37).all()), (y.view[0].tolist(), y64[0].tolist())


# ------------------------------------------------------------------ backward data
@pytest.mark.parametrize("M", MS)
def test_backward_data_integers_are_exact(M):
    g = torch.Generator().manual_seed(100 + M)
    for K, N in itertools.product(KS, NS):
        dy, w = _ints(g, -3, 3, K, N).cuda(), _ints(g, -3, 3, N, M).cuda()
        want = (dy.double() @ w.double()).float()
        dx = Guarded(K, M)
        assert backward_data(dy, w, None, K, M, N, dx) == 0
        assert dx.guards_intact() and torch.equal(dx.view, want), (K, M, N, float((dx.view - want).abs().max()))


def _dsilu64(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


@pytest.mark.parametrize("M,N", HIDDEN)
def test_backward_data_rounding(M, N):
    K = 320
    g = torch.Generator().manual_seed(7 * M + N)
    dy, w = torch.randn(K, N, generator=g).cuda(), (torch.randn(N, M, generator=g) * M ** -0.5).cuda()
    zp = (torch.rand(K, M, generator=g) * 40 - 20)
    zp[0, :8] = torch.tensor([-20.0, 20.0, 0.0, -1.2785, -1.27846, -1.278465, 1.0, -5.0])        # the ends, and the root of silu'
    zp = zp.cuda()
    d64 = ref.f64(dy) @ ref.f64(w)
    f64 = _dsilu64(ref.f64(zp))
    dx64 = d64 * f64
    bar = (N + 2) * U * (ref.f64(dy).abs() @ ref.f64(w).abs()) * f64.abs() + 8 * U * dx64.abs()
    dx = Guarded(K, M)
    assert backward_data(dy, w, zp, K, M, N, dx) == 0
    assert dx.written()
    r = ((dx.f64() - dx64).abs() / bar).max()
    print(f"backward data {K}x{N}->{M}: worst |dX - dX64| / bar {float(r):.3f}")
    assert float(r) <= 1.0
    dx0 = Guarded(K, M)                                                           # no factor: the bar of the product alone
    assert backward_data(dy, w, None, K, M, N, dx0) == 0
    assert bool(((dx0.f64() - d64).abs() <= (N + 2) * U * (ref.f64(dy).abs() @ ref.f64(w).abs())).all())


# ------------------------------------------------------------------ gather
def _gather_call(B, od, pd, batch, idx, stats, outs):
    a = learn.PgttLearnGatherArgs()
    a.idx = _p(idx)
    for k in ("obs", "priv", "u", "logp", "adv", "ret"):
        setattr(a, k, _p(batch[k]))
    a.mean_s, a.std_s, a.mean_p, a.std_p = (_p(t) for t in stats)
    for k in ("x_s", "x_p", "u_out", "logp_out", "adv_out", "ret_out"):
        setattr(a, k, _p(outs[k]))
    a.B, a.rows, a.obs_dim, a.priv_dim, a.act_dim = B, batch["rows"], od, pd, 12
    return a


def _gather_setup(B, od, pd, const_adv=False, rows=2048):
    g = torch.Generator().manual_seed(B * 7 + od)
    r = lambda *s: torch.randn(*s, generator=g)
    batch = {"obs": (r(rows, od) * 3 + 1).cuda(), "priv": (r(rows, pd) * 0.2 - 2).cuda(), "u": r(rows, 12).cuda(), "logp": r(rows).cuda(),
             "adv": (torch.full((rows,), 0.7) if const_adv else r(rows) * 2 + 0.3).cuda(), "ret": (r(rows) * 10).cuda(), "rows": rows}
    stats = [(r(od) * 2).cuda(), (torch.rand(od, generator=g) * 4.95 + 0.05).cuda(), (r(pd) * 2).cuda(), (torch.rand(pd, generator=g) * 4.95 + 0.05).cuda()]
    idx = torch.randint(0, rows, (B,), generator=g)
    if B >= 4:
        idx[0], idx[1], idx[2], idx[3] = rows - 1, 0, idx[B - 1], rows - 1           # the ends of the batch, and repeats
    else:
        idx[0] = rows - 1
    outs = lambda: {"x_s": Guarded(B, od), "x_p": Guarded(B, pd, front=21), "u_out": Guarded(B, 12), "logp_out": Guarded(B, front=17),
                    "adv_out": Guarded(B, back=29), "ret_out": Guarded(B)}
    return batch, stats, idx.cuda(), outs


@pytest.mark.parametrize("od,pd", [(1, 1), (171, 215)])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1031])
def test_gather(B, od, pd):
    batch, stats, idx, outs = _gather_setup(B, od, pd)
    o1, o2 = outs(), outs()
    for o in (o1, o2):
        assert learn.lib().pgtt_learn_gather(C.byref(_gather_call(B, od, pd, batch, idx, stats, o)), _st()) == 0
    torch.cuda.synchronize()
    for k, t in o1.items():
        assert t.guards_intact(), k
        assert torch.equal(t.view, o2[k].view), k                                 # two calls: equal bits
    for k, src in (("u_out", "u"), ("logp_out", "logp"), ("ret_out", "ret")):
        assert torch.equal(o1[k].view, batch[src][idx]), k
    for k, src, (mean, std) in (("x_s", "obs", stats[:2]), ("x_p", "priv", stats[2:])):
        x64 = (ref.f64(batch[src][idx]) - ref.f64(mean)) / ref.f64(std)
        bar = 3 * U * x64.abs() + U * ref.f64(mean).abs() / ref.f64(std)
        assert bool(((o1[k].f64() - x64).abs() <= bar).all()), (k, float(((o1[k].f64() - x64).abs() / bar).max()))
    a64 = ref.f64(batch["adv"][idx])
    want = ref.normalise_advantage(a64)
    bar = (B * U + 4 * U) * ((a64 - a64.mean()).abs() + a64.abs().mean()) / (a64.std(unbiased=False) + 1e-8)
    err = (o1["adv_out"].f64() - want).abs()
    print(f"gather B={B}: worst advantage error / bar {float((err / bar.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bar).all())
    if B == 1:
        assert o1["adv_out"].view.tolist() == [0.0]                               # std 0: (a - a) / 1e-8


def test_gather_constant_advantage():
    B = 64
    batch, stats, idx, outs = _gather_setup(B, 171, 215, const_adv=True)
    o = outs()
    assert learn.lib().pgtt_learn_gather(C.byref(_gather_call(B, 171, 215, batch, idx, stats, o)), _st()) == 0
    a64 = ref.f64(batch["adv"][idx])
    bar = (B * U + 4 * U) * ((a64 - a64.mean()).abs() + a64.abs().mean()) / (a64.std(unbiased=False) + 1e-8)
    got = o["adv_out"].f64()
    assert o["adv_out"].guards_intact() and bool(torch.isfinite(got).all()) and bool(((got - ref.normalise_advantage(a64)).abs() <= bar).all())
    assert bool((got == got[0]).all())                                            # equal inputs, equal outputs


# ------------------------------------------------------------------ value loss
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1031])
def test_value_loss(B):
    g = torch.Generator().manual_seed(B)
    v, ret = (torch.randn(B, generator=g) * 3).cuda(), (torch.randn(B, generator=g) * 20 + 5).cuda()
    loss, dv = Guarded(1), Guarded(B)
    assert learn.lib().pgtt_learn_value_loss(_p(v), _p(ret), B, _p(loss), _p(dv), _st()) == 0
    assert loss.written() and dv.written()
    v64, r64 = ref.f64(v), ref.f64(ret)
    dv64, l64 = 0.5 * (v64 - r64) / B, 0.25 * ((r64 - v64) ** 2).mean()
    assert bool(((dv.f64() - dv64).abs() <= 4 * U * dv64.abs()).all())
    assert abs(float(loss.f64()) - float(l64)) <= (B + 4) * U * float(l64)
    loss2, dv2 = Guarded(1), Guarded(B)
    assert learn.lib().pgtt_learn_value_loss(_p(v), _p(ret), B, _p(loss2), _p(dv2), _st()) == 0
    assert torch.equal(loss.view, loss2.view) and torch.equal(dv.view, dv2.view)


# ------------------------------------------------------------------ clip + Adam
LR = 3e-4


class AdamState:
    def __init__(self, P, p0):
        self.P = P
        self.p, self.g, self.m, self.v = Guarded(P), Guarded(P, front=21), Guarded(P, back=29), Guarded(P, front=17)
        self.p.view.copy_(p0); self.m.view.zero_(); self.v.view.zero_()
        self.t = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.partial, self.norm = Guarded(learn.lib().pgtt_learn_adam_partials(P)), Guarded(1)

    def args(self, max_norm, grad_scale=1.0):
        a = learn.PgttLearnAdamArgs()
        a.p, a.g, a.m, a.v, a.t, a.partial, a.norm_1, a.P = _p(self.p), _p(self.g), _p(self.m), _p(self.v), _p(self.t), _p(self.partial), _p(self.norm), self.P
        a.lr, a.beta1, a.beta2, a.eps, a.max_norm, a.grad_scale = LR, 0.9, 0.999, 1e-8, max_norm, grad_scale
        return a

    def step(self, g, max_norm, grad_scale=1.0):
        self.g.view.copy_(g)
        assert learn.lib().pgtt_learn_clip_adam(C.byref(self.args(max_norm, grad_scale)), _st()) == 0
        torch.cuda.synchronize()
        for t in (self.p, self.g, self.m, self.v, self.partial, self.norm):
            assert t.guards_intact()


@pytest.mark.parametrize("active", [True, False])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 4097, 530_000])
def test_clip_adam_five_steps(P, active):
    """five steps against ppo_reference.Adam fed coef64 g: after step k, |p - p64| <= k (2^-23 |p| + 1e-5 lr) (the Adam bar of DESIGN.md 13); the
    norm within (P / 64 + 70) u: a lane's chain of <= P / 65536 + 8 terms, a wave butterfly of 6, four waves, a chain of <= 4 partials per lane,
    butterfly and waves again, the squares and the root - and far below P / 64 for a large P; t advances by one per call"""
    g = torch.Generator().manual_seed(P + active)
    p0 = torch.randn(P, generator=g)
    A, B = AdamState(P, p0.cuda()), AdamState(P, p0.cuda())
    adam = ref.Adam([p0], LR)
    max_norm = 1.0
    for k in range(1, 6):
        gk = torch.randn(P, generator=g)
        gk = gk * ((3.0 if active else 0.3) / float(gk.norm()))                   # norm 3: coef 1 / 3; norm 0.3: coef 1
        for s in (A, B):
            s.step(gk.cuda(), max_norm)
        n64 = float(ref.f64(gk).norm())
        coef = min(1.0, max_norm / (n64 + 1e-6))
        assert (coef < 1.0) == active
        (p64,) = adam.step([coef * ref.f64(gk)])
        assert abs(float(A.norm.view) - n64) <= (P / 64 + 70) * U * n64, (k, float(A.norm.view), n64)
        assert A.t.tolist() == [k]
        dp = (A.p.f64() - p64).abs()
        tol = k * (2.0 ** -23 * p64.abs() + 1e-5 * LR)
        assert bool((dp <= tol).all()), (k, float((dp / tol).max()))
        assert torch.equal(A.g.view, gk.cuda())                                   # grad_scale 1: the gradient is left as it was
        for name in ("p", "m", "v", "norm"):                                      # two runs from equal state: equal bits
            assert torch.equal(getattr(A, name).view, getattr(B, name).view), (k, name)
    print(f"clip + Adam P={P} clip {'active' if active else 'inactive'}: worst |p - p64| / bar after five steps {float((dp / tol).max()):.3f}")


@pytest.mark.parametrize("P", [65, 4097])
def test_clip_adam_grad_scale_is_a_scaled_gradient(P):
    g = torch.Generator().manual_seed(P)
    p0, gk = torch.randn(P, generator=g).cuda(), (torch.randn(P, generator=g) * 0.2).cuda()
    A, B = AdamState(P, p0), AdamState(P, p0)
    for _ in range(2):
        A.step(gk, 1.0, grad_scale=0.5)
        B.step(gk * 0.5, 1.0)
        assert torch.equal(A.g.view, gk * 0.5)
    for name in ("p", "m", "v", "norm"):
        assert torch.equal(getattr(A, name).view, getattr(B, name).view), name
    assert A.t.tolist() == [2]


# ------------------------------------------------------------------ GAE
def _gae_case(T, N, shift, g):
    """pattern of env e by (e + shift) % 5: 0 truncated at the last step, 1 terminated at the first, 2 truncated on every step, 3 no flag, 4 random
    done at rate 0.1 with a truncation on a third of them"""
    rew, val, boot = torch.randn(T, N, generator=g), torch.randn(T, N, generator=g) * 3 + 1, torch.randn(N, generator=g) * 3 + 1
    done = (torch.rand(T, N, generator=g) < 0.1).float()
    trunc = done * (torch.rand(T, N, generator=g) < 1 / 3).float()
    for e in range(N):
        k = (e + shift) % 5
        if k < 4:
            done[:, e] = 0; trunc[:, e] = 0
        if k == 0:
            done[T - 1, e] = 1; trunc[T - 1, e] = 1
        elif k == 1:
            done[0, e] = 1
        elif k == 2:
            done[:, e] = 1; trunc[:, e] = 1
    return trunc, done, rew, val, boot


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("T", [1, 2, 20])
def test_gae(T, N):
    lam, gamma = 0.95, 0.97
    g = torch.Generator().manual_seed(31 * T + N)
    worst = 0.0
    for shift in (range(5) if N < 5 else range(1)):
        trunc, done, rew, val, boot = _gae_case(T, N, shift, g)
        adv64, vs64 = ref.gae(trunc, done * (1 - trunc), rew, val, boot, lam, gamma)
        v_next = torch.cat([val[1:], boot[None]], 0)
        S = (ref.f64(rew).abs() + ref.f64(val).abs() + ref.f64(v_next).abs()).sum(0)            # [N]
        d = [t.cuda() for t in (trunc, done, rew, val, boot)]
        adv, vs = Guarded(T, N), Guarded(T, N, front=21, back=17)
        assert learn.lib().pgtt_learn_gae(*[_p(t) for t in d], T, N, lam, gamma, _p(adv), _p(vs), _st()) == 0
        assert adv.written() and vs.written()
        bar_vs, bar_adv = (2 * T + 6) * U * S, (2 * T + 12) * U * S
        assert bool(((vs.f64() - vs64).abs() <= bar_vs).all()) and bool(((adv.f64() - adv64).abs() <= bar_adv).all())
        worst = max(worst, float(((vs.f64() - vs64).abs() / bar_vs).max()), float(((adv.f64() - adv64).abs() / bar_adv).max()))
        assert bool((adv.view[d[0] == 1] == 0).all())                             # exactly 0 on a truncated step
        ta, tv = ppo.compute_gae(d[0], d[1] * (1.0 - d[0]), d[2], d[3], d[4], lam, gamma)        # the PyTorch-op form on the same device
        assert bool(((vs.f64() - ref.f64(tv)).abs() <= bar_vs).all()) and bool(((adv.f64() - ref.f64(ta)).abs() <= bar_adv).all())
    print(f"gae T={T} N={N}: worst error / bar {worst:.3f}")


# ------------------------------------------------------------------ refusals
def _refusal_cases():
    """per entry: (call(args) -> rc, the valid arguments by name, the names of the sizes, the outputs to inspect, the pointers that may be NULL)"""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    K, M, N = 17, 5, 3
    cases = []
    a = dict(x=r(K, M), w=r(N, M), b=r(N), K=K, M=M, N=N, y=Guarded(K, N), z=Guarded(K, N))
    cases.append(("forward", lambda a: forward(a["x"], a["w"], a["b"], a["K"], a["M"], a["N"], 1, a["y"], a["z"]), a, ("K", "M", "N"), ()))
    a = dict(dy=r(K, N), w=r(N, M), zp=r(K, M), K=K, M=M, N=N, dx=Guarded(K, M))
    cases.append(("backward_data", lambda a: backward_data(a["dy"], a["w"], a["zp"], a["K"], a["M"], a["N"], a["dx"]), a, ("K", "M", "N"), ("zp",)))
    a = dict(v=r(K), ret=r(K), B=K, loss=Guarded(1), dv=Guarded(K))
    cases.append(("value_loss", lambda a: learn.lib().pgtt_learn_value_loss(_p(a["v"]), _p(a["ret"]), a["B"], _p(a["loss"]), _p(a["dv"]), _st()), a, ("B",), ()))
    T = 4
    a = dict(trunc=torch.zeros(T, K).cuda(), done=torch.zeros(T, K).cuda(), rew=r(T, K), val=r(T, K), boot=r(K), T=T, N=K, adv=Guarded(T, K), vs=Guarded(T, K))
    cases.append(("gae", lambda a: learn.lib().pgtt_learn_gae(_p(a["trunc"]), _p(a["done"]), _p(a["rew"]), _p(a["val"]), _p(a["boot"]), a["T"], a["N"], 0.95, 0.97,
                                                              _p(a["adv"]), _p(a["vs"]), _st()), a, ("T", "N"), ()))
    rows, B = 40, 9
    a = dict(idx=torch.randint(0, rows, (B,), generator=g).cuda(), obs=r(rows, M), priv=r(rows, N), u=r(rows, 12), logp=r(rows), adv=r(rows), ret=r(rows),
             mean_s=r(M), std_s=torch.ones(M).cuda(), mean_p=r(N), std_p=torch.ones(N).cuda(), x_s=Guarded(B, M), x_p=Guarded(B, N), u_out=Guarded(B, 12),
             logp_out=Guarded(B), adv_out=Guarded(B), ret_out=Guarded(B), B=B, rows=rows, obs_dim=M, priv_dim=N, act_dim=12)

    def gather(a):
        s = learn.PgttLearnGatherArgs()
        for k, v in a.items():
            setattr(s, k, v if isinstance(v, int) else _p(v))
        return learn.lib().pgtt_learn_gather(C.byref(s), _st())
    cases.append(("gather", gather, a, ("B", "rows", "obs_dim", "priv_dim", "act_dim"), ()))
    P = 70
    a = dict(p=Guarded(P), g=Guarded(P), m=Guarded(P), v=Guarded(P), t=Guarded(1, dtype=torch.int64, fill=-777), partial=Guarded(1), norm_1=Guarded(1), P=P)

    def adam(a):
        s = learn.PgttLearnAdamArgs()
        for k, v in a.items():
            setattr(s, k, v if isinstance(v, int) else _p(v))
        s.lr, s.beta1, s.beta2, s.eps, s.max_norm, s.grad_scale = LR, 0.9, 0.999, 1e-8, 1.0, 1.0
        return learn.lib().pgtt_learn_clip_adam(C.byref(s), _st())
    cases.append(("clip_adam", adam, a, ("P",), ()))
    return cases


def test_refusals_write_nothing():
    """every entry: each NULL pointer and each non-positive size gives PGTT_E_ARG with every sentinel intact (the pointers that may be NULL are the
    named ones: Zprev of backward_data; Z of forward only with act == 0, so here, with act = 1, it is refused too); NULL argument structs"""
    n = 0
    for name, call, args, sizes, optional in _refusal_cases():
        outs = [v for v in args.values() if isinstance(v, Guarded)]
        trials = [(k, None) for k, v in args.items() if not isinstance(v, int) and k not in optional] + [(k, bad) for k in sizes for bad in (0, -1)]
        for key, bad in trials:
            rc = call(dict(args, **{key: bad}))
            torch.cuda.synchronize()
            assert rc == E_ARG, (name, key, bad, rc)
            assert learn.lib().pgtt_learn_last_error().decode().startswith("pgtt_learn_"), (name, key)
            assert all(o.untouched() for o in outs), (name, key, bad)
            n += 1
    assert learn.lib().pgtt_learn_gather(None, _st()) == E_ARG and learn.lib().pgtt_learn_clip_adam(None, _st()) == E_ARG
    assert learn.lib().pgtt_learn_adam_partials(0) == 0 and learn.lib().pgtt_learn_adam_partials(-5) == 0
    assert n > 60
    info = learn.build_info()
    from phase_guided_terrain_traversal_amd import srchash
    assert info["flavor"] == "product" and info["src"] == srchash.side_sha256("learn")
