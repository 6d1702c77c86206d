"""The two distillation entries of libpgtt_learn.so through the bare C ABI (include/pgtt_learn.h): pgtt_learn_distill_loss against the fp64
statement in tests/distill_reference.py, pgtt_learn_gather_rows against pgtt_learn_gather and the indexed rows, bit for bit.  Every output is a
view into a larger allocation of sentinels at an odd float offset, as in test_gpu_learn_kernels.py.

The bars, first order in u = 2^-24, none fitted to the kernel.  expf, log1pf, logf and tanhf are taken at 2 ulp = 4 u, every other operation at u.
  sigma = max(r, 0) + log1pf(expf(-|r|)) + 1e-3: 4 u (expf) + 4 u (log1pf) on a part of the sum, two additions and the rounded constant: 12 u.
  q = (st^2 + d^2) / ss^2: st^2 25 u, d^2 3 u, their sum 26 u; ss^2 25 u; the division: 52 u.  1 - q: 53 u q + u.
  draw = (1 - q) / ss * sigmoid / B: on top of 1 - q a factor of 12 + 1 (/ ss), 6 + 1 (sigmoid: expf, add, divide; multiply), 1 (/ B) = 21 u of
      |1 - q| <= 1 + q: at most 74 u q / ss + 22 u / ss, times sigmoid / B.  Bar: 80 u (1 / ss + q / ss) sigmoid / B - relative to the TERMS, whose
      difference vanishes at the optimum - plus (1 / ss + q / ss) / B times 2^-126, the underflow threshold, for a sigmoid in the denormal range.
  dloc = -d / ss^2 / B: d 1 u, ss^2 25 u, two divisions: 28 u.  Bar: 32 u |d| / ss^2 / B.
  KL = log(ss / st) + 0.5 (q - 1): the ratio 25 u, so the logarithm 25 u absolute and 4 u of itself; 0.5 (q - 1) 27 u q + u; against the terms
      |log|, 0.5 q, 0.5 that is at most 51 u of their sum per element; the sums over A, the lanes and the blocks add at most (B + A) u of it, the
      division by B one more.  Bar: (B + 80) u (1 / B) sum (|log| + 0.5 q + 0.5).
  action error: tanh 4 u each, so the difference D is off by 4 u (|ts| + |tt|) + u |D| and its square by 8 u |D| (|ts| + |tt|) + 3 u D^2 + 64 u^2;
      the sum over B A elements adds (B + A) u sum D^2.  Bar: (1 / (B A)) sum (8 u |D| (|ts| + |tt|) + 64 u^2 + (B + A + 4) u D^2).
"""
import ctypes as C
import itertools
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distill_reference as dref  # noqa: E402

from phase_guided_terrain_traversal_amd import learn  # noqa: E402

U = 2.0 ** -24
SENT = 777.0
E_ARG = -1
F64 = torch.float64
RAWS = (-88.0, 88.0, -20.0, 20.0, 0.0)
TINY = 2.0 ** -126


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
        return self.guards_intact() and bool((self.view != self.fill).all())

    def f64(self):
        return self.view.detach().to("cpu", F64)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def distill_loss(s, t, B, A, partial, loss, grad):
    return learn.lib().pgtt_learn_distill_loss(_p(s), _p(t), B, A, _p(partial), _p(loss), _p(grad), _st())


def gather_rows(idx, obs, tgt, mean, std, B, rows, od, td, x, y):
    return learn.lib().pgtt_learn_gather_rows(_p(idx), _p(obs), _p(tgt), _p(mean), _p(std), B, rows, od, td, _p(x), _p(y), _st())


def _heads(B, A, seed):
    """random heads; element k = i A + a takes by k % 11: 0 - 4 the student's raw at +-88, +-20, 0; 5 the teacher's; 6 d = 0; 7 |d| = 10; 8 both raws
    at +-88 with d = 0; 9, 10 as drawn"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    ls, rs, lt, rt = r(B * A) * 1.5, r(B * A) * 2 - 1, r(B * A) * 1.5, r(B * A) * 2 - 1
    for k in range(B * A):
        p, c = k % 11, (k // 11) % 5
        if p < 5:
            rs[k] = RAWS[p]
        elif p == 5:
            rt[k] = RAWS[c]
        elif p == 6:
            lt[k] = ls[k]
        elif p == 7:
            lt[k] = ls[k] + (10.0 if c % 2 else -10.0)
        elif p == 8:
            rs[k] = rt[k] = RAWS[c % 2]
            lt[k] = ls[k]
    s = torch.cat([ls.view(B, A), rs.view(B, A)], -1).contiguous()
    t = torch.cat([lt.view(B, A), rt.view(B, A)], -1).contiguous()
    return s, t


def _check_loss(s, t, B, A, tag):
    sc, tc = s.cuda(), t.cuda()
    outs = []
    for _ in range(2):
        partial, loss, grad = Guarded(2 * ((B + 63) // 64), front=21), Guarded(2, back=17), Guarded(B, 2 * A)
        assert distill_loss(sc, tc, B, A, partial, loss, grad) == 0
        torch.cuda.synchronize()
        assert partial.written() and loss.written() and grad.written(), tag
        outs.append((loss, grad))
    assert torch.equal(outs[0][0].view, outs[1][0].view) and torch.equal(outs[0][1].view, outs[1][1].view), tag      # two calls: equal bits
    loss, grad = outs[0]
    assert bool(torch.isfinite(loss.view).all()) and bool(torch.isfinite(grad.view).all()), tag
    k = dref.terms(s, t)
    l64, g64 = dref.loss(s, t)
    bar_loc = 32 * U * k["d"].abs() / (k["ss"] * k["ss"]) / B
    bar_raw = (80 * U * k["sig"] + TINY) * (1 / k["ss"] + k["q"] / k["ss"]) / B
    e = (grad.f64() - g64).abs()
    r_loc = float((e[:, :A] / bar_loc.clamp(min=1e-300)).max()) if bool((bar_loc > 0).any()) else 0.0
    assert bool((e[:, :A] <= bar_loc).all()), (tag, r_loc)
    r_raw = float((e[:, A:] / bar_raw).max())
    assert bool((e[:, A:] <= bar_raw).all()), (tag, r_raw)
    bar_kl = (B + 80) * U * float((k["log"].abs() + 0.5 * k["q"] + 0.5).sum()) / B
    ls, lt = dref.split(dref.f64(s))[0], dref.split(dref.f64(t))[0]
    ts, tt = torch.tanh(ls), torch.tanh(lt)
    D = ts - tt
    bar_act = float((8 * U * D.abs() * (ts.abs() + tt.abs()) + 64 * U * U + (B + A + 4) * U * D * D).sum()) / (B * A)
    e_kl, e_act = abs(float(loss.f64()[0]) - float(l64[0])), abs(float(loss.f64()[1]) - float(l64[1]))
    print(f"distill loss {tag}: worst / bar  KL {e_kl / bar_kl:.3f}  action error {e_act / bar_act:.3f}  dloc {r_loc:.3f}  draw {r_raw:.3f}")
    assert e_kl <= bar_kl and e_act <= bar_act, (tag, e_kl / bar_kl, e_act / bar_act)


@pytest.mark.parametrize("A", [1, 12])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1031])
def test_distill_loss_against_fp64(B, A):
    s, t = _heads(B, A, 13 * B + A)
    _check_loss(s, t, B, A, f"B={B} A={A}")


@pytest.mark.parametrize("A", [1, 12])
def test_distill_loss_at_every_pairing_of_the_large_raws(A):
    """raw_s x raw_t in {+-88, +-20, 0}^2 x d in {0, 1e-3, -10, 10}: 100 elements, as 100 rows of one or 9 rows of twelve (the rest as drawn)"""
    combos = list(itertools.product(RAWS, RAWS, (0.0, 1e-3, -10.0, 10.0)))
    B = -(-len(combos) // A)
    s, t = _heads(B, A, 5 + A)
    for k, (rs, rt, d) in enumerate(combos):
        i, a = divmod(k, A)
        s[i, A + a], t[i, A + a] = rs, rt
        t[i, a] = s[i, a] + d
    _check_loss(s, t, B, A, f"pairings A={A}")


@pytest.mark.parametrize("A", [1, 12])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1031])
def test_equal_heads_give_exact_zeros(B, A):
    _, t = _heads(B, A, 7 * B + A)
    tc = t.cuda()
    partial, loss, grad = Guarded(2 * ((B + 63) // 64)), Guarded(2), Guarded(B, 2 * A)
    assert distill_loss(tc.clone(), tc, B, A, partial, loss, grad) == 0
    torch.cuda.synchronize()
    assert loss.guards_intact() and grad.guards_intact() and partial.guards_intact()
    assert loss.view.tolist() == [0.0, 0.0] and bool((grad.view == 0).all()) and bool((partial.view == 0).all())


def _gather_inputs(B, od, td, rows=2048):
    g = torch.Generator().manual_seed(B * 5 + od)
    r = lambda *s: torch.randn(*s, generator=g)
    obs, tgt = (r(rows, od) * 3 + 1).cuda(), r(rows, td).cuda()
    mean, std = (r(od) * 2).cuda(), (torch.rand(od, generator=g) * 4.95 + 0.05).cuda()
    idx = torch.randint(0, rows, (B,), generator=g)
    edge = [-1, rows, rows - 1, 0, -(2 ** 40), 2 ** 40, rows + 7]
    if B >= len(edge):
        idx[:len(edge)] = torch.tensor(edge)
    else:
        idx[0] = rows + 3
    return obs, tgt, mean, std, idx.cuda()


@pytest.mark.parametrize("od,td", [(1, 1), (171, 24)])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1031])
def test_gather_rows(B, od, td):
    rows = 2048
    obs, tgt, mean, std, idx = _gather_inputs(B, od, td, rows)
    x, y = Guarded(B, od), Guarded(B, td, front=21, back=17)
    assert gather_rows(idx, obs, tgt, mean, std, B, rows, od, td, x, y) == 0
    x2, y2 = Guarded(B, od), Guarded(B, td)
    assert gather_rows(idx, obs, tgt, mean, std, B, rows, od, td, x2, y2) == 0
    torch.cuda.synchronize()
    assert x.written() and y.written()
    assert torch.equal(x.view, x2.view) and torch.equal(y.view, y2.view)
    clamped = idx.clamp(0, rows - 1)
    assert torch.equal(y.view, tgt[clamped])
    # pgtt_learn_gather on the same observations, statistics and indices: its x_s, bit for bit
    z = lambda *s: torch.zeros(*s, device="cuda")
    a = learn.PgttLearnGatherArgs()
    keep = dict(priv=z(rows, 1), u=z(rows, 1), logp=z(rows), adv=z(rows), ret=z(rows), mean_p=z(1), std_p=torch.ones(1, device="cuda"),
                x_p=z(B, 1), u_out=z(B, 1), logp_out=z(B), adv_out=z(B), ret_out=z(B))
    xs = Guarded(B, od)
    a.idx, a.obs, a.mean_s, a.std_s, a.x_s = _p(idx), _p(obs), _p(mean), _p(std), _p(xs)
    for k, v in keep.items():
        setattr(a, k, _p(v))
    a.B, a.rows, a.obs_dim, a.priv_dim, a.act_dim = B, rows, od, 1, 1
    assert learn.lib().pgtt_learn_gather(C.byref(a), _st()) == 0
    torch.cuda.synchronize()
    assert xs.written() and torch.equal(x.view, xs.view)
    x64, y64 = dref.gather_rows(idx, obs, tgt, mean, std)
    bar = 3 * U * x64.abs() + U * dref.f64(mean).abs() / dref.f64(std)
    assert bool(((x.f64() - x64).abs() <= bar).all()) and torch.equal(y.f64(), y64)


def test_refusals_write_nothing():
    """both entries: each NULL pointer and each non-positive size gives PGTT_E_ARG, a message, and every sentinel intact"""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    B, A, rows, od, td = 9, 3, 40, 5, 4
    cases = []
    a = dict(s=r(B, 2 * A), t=r(B, 2 * A), B=B, A=A, partial=Guarded(2), loss=Guarded(2), grad=Guarded(B, 2 * A))
    cases.append(("distill_loss", lambda a: distill_loss(a["s"], a["t"], a["B"], a["A"], a["partial"], a["loss"], a["grad"]), a, ("B", "A")))
    a = dict(idx=torch.randint(0, rows, (B,), generator=g).cuda(), obs=r(rows, od), tgt=r(rows, td), mean=r(od), std=torch.ones(od).cuda(),
             B=B, rows=rows, od=od, td=td, x=Guarded(B, od), y=Guarded(B, td))
    cases.append(("gather_rows", lambda a: gather_rows(a["idx"], a["obs"], a["tgt"], a["mean"], a["std"], a["B"], a["rows"], a["od"], a["td"], a["x"], a["y"]),
                  a, ("B", "rows", "od", "td")))
    n = 0
    for name, call, args, sizes in cases:
        outs = [v for v in args.values() if isinstance(v, Guarded)]
        trials = [(k, None) for k, v in args.items() if not isinstance(v, int)] + [(k, bad) for k in sizes for bad in (0, -1)]
        for key, bad in trials:
            rc = call(dict(args, **{key: bad}))
            torch.cuda.synchronize()
            assert rc == E_ARG, (name, key, bad, rc)
            assert learn.lib().pgtt_learn_last_error().decode().startswith("pgtt_learn_" + name), (name, key)
            assert all(o.untouched() for o in outs), (name, key, bad)
            n += 1
        assert call(args) == 0                                                    # the valid call, for contrast
        torch.cuda.synchronize()
        assert all(o.written() for o in outs), name
    assert n == 5 + 4 + 7 + 8
