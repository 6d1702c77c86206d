"""The recurrent policy's entries of libpgtt_learn.so through the bare C ABI (include/pgtt_learn.h): the point-wise GRU cell forward and backward,
the clear, the add, and pgtt_learn_recurrent_act, against the fp64 statement in tests/recurrent_policy_reference.py.  Every output is a view into
a larger allocation of sentinels at an odd float offset, as in test_gpu_learn_kernels.py.  The acting step runs at every trip count of its tile loop
(R = 16, 32, 48, 64, 80, 256) on policy177's trunk and, through the bare ABI, on three small trunks (ACT_CASES).

The bars, first order in u = 2^-24, none fitted to the kernel.  expf is taken at 2 ulp = 4 u, every other operation at u; TINY = 2^-126 is added where
an expf result can be denormal (its relative accuracy is lost there).  A bar X_bar is an absolute bound of |X - X64|.

  sigmoid(v) = 1 / (1 + t) or t / (1 + t), t = expf(-|v|): expf 4 u, the sum u, the division u: 6 u s; an argument off by dv moves it by s (1 - s) dv.
      s_bar = 6 u s + s (1 - s) dv + TINY.
  tanh(v) = sign(v) (1 - t) / (1 + t), t = expf(-2 |v|): t off by 4 u t moves the quotient by 2 / (1 + t)^2 * 4 u t = 2 u (1 - n^2) (absolute: 1 - t
      cancels near v = 0); 1 - t, 1 + t and the division u each: 3 u |n|; an argument off by dv moves it by (1 - n^2) dv.
      n_bar = 2 u (1 - n^2) + 3 u |n| + (1 - n^2) dv + TINY.
  The cell from exact gi, gh, m0:  dv_r = u |gi_r + gh_r| (one addition), dv_u likewise;  pre_n = gi_n + r gh_n: dv_n = |gh_n| r_bar + u |r gh_n| + u |pre_n|;
      m1 = (1 - u) n + u m0:  1 - u is off by u_bar + u |1 - u|, so
      m1_bar = |n| (u_bar + u |1 - u|) + |1 - u| n_bar + u |(1 - u) n| + |m0| u_bar + u |u m0| + u |m1|.
  The cell's backward from exact (fp32) gates, gh, m0, dm1_head, dm0_next - every step is a handful of rounded operations on exact inputs; a saturated
  gate (u or 1 - u down to 4e-44) makes products that fall below the normal range, where the relative model does not hold: every bar gets + TINY:
      dm1 = a + b: u |dm1|.   dn = dm1 (1 - u): 3 u |dn|.   du = dm1 (m0 - n): 3 u |du|.   direct = u dm1: 2 u |direct|.
      dpre_n = dn (1 - n^2): n^2 u, 1 - n^2 off by u n^2 + u (1 - n^2) <= u (absolute: it cancels near |n| = 1), so dpn_bar = 4 u |dpre_n| + u |dn|.
      dpre_u = du (u (1 - u)): 1 - u u, the product u, times du (3 u) u: 6 u |dpre_u|.
      dr = gh_n dpre_n: |gh_n| dpn_bar + u |dr|.   dpre_r = dr (r (1 - r)): r (1 - r) dr_bar + 3 u |dpre_r|.   dgh_n = r dpre_n: r dpn_bar + u |r dpre_n|.
  pgtt_learn_recurrent_act.  A K-term fp32 dot product in any order with its biases: (K + 1 + biases) u (sum |w| |x| + |b|), as test_gpu_learn_kernels.py
      takes it, plus |W| x_bar for an input that is off by x_bar.  Propagation:
      x = (obs - mean) / std: 2 u |x|.   z_l = W_l h + b_l: (K + 2) u (|W| |h| + |b|) + |W| h_bar.   h = silu(z): 1.1 z_bar + 6 u |h|  (|silu'| <= 1.1).
      gi_r + gh_r (one chain, two biases): dv_r = (h3 + R + 3) u (|W_ih| |h3| + |W_hh| |m0| + |b_ih| + |b_hh|) + |W_ih| h3_bar  (m0 is an exact input); u likewise.
      gi_n: (h3 + 2) u (..) + |W_ih| h3_bar;   gh_n: (R + 2) u (..);   dv_n = gi_n_bar + r gh_n_bar + |gh_n| r_bar + u |r gh_n| + u |pre_n|.
      r, u, n, m1 by the formulas above.   head = chain over h3 and R terms, one bias: (h3 + R + 2) u (|W3| |h3| + |W_m| |m1| + |b3|) + |W3| h3_bar + |W_m| m1_bar.
      action = tanh(loc) by n_bar with dv = head_bar.
      Through three layers these worst-case sums grow large, so the same outputs are also held to the bars that start at h3: the h3 the trunk left in
      the scratch is read back and taken as an exact input (h3_bar = 0), which leaves the chains, gates, m1, head and tanh of the new kernel alone.
"""
import ctypes as C
import os
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recurrent_policy_reference as rref  # noqa: E402

from phase_guided_terrain_traversal_amd import learn  # noqa: E402
from phase_guided_terrain_traversal_amd.learn import PgttLearnRecurrentActArgs  # noqa: E402
from phase_guided_terrain_traversal_amd.policy import PolicyMLP, _DIR as POLICY_DIR  # noqa: E402
from phase_guided_terrain_traversal_amd.recurrent_policy import RecurrentPolicy  # noqa: E402

U = 2.0 ** -24
TINY = 2.0 ** -126
SENT = 777.0
E_ARG = -1
F64 = torch.float64
f64 = rref.f64


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


def _msg():
    return learn.lib().pgtt_learn_last_error().decode()


def sig_bar(s, dv):
    return 6 * U * s + s * (1 - s) * dv + TINY


def tanh_bar(n, dv):
    return 2 * U * (1 - n * n) + 3 * U * n.abs() + (1 - n * n) * dv + TINY


def m1_bar(u, n, m0, m1, u_bar, n_bar):
    return (n.abs() * (u_bar + U * (1 - u).abs()) + (1 - u).abs() * n_bar + U * ((1 - u) * n).abs() + m0.abs() * u_bar + U * (u * m0).abs()
            + U * m1.abs())


# ------------------------------------------------------------------ the cell
EDGES = (0.0, 20.0, -20.0, 100.0, -100.0, 200.0, -200.0)


def _cell_inputs(B, R, seed):
    """random gi, gh, m0; element k of each gate's block takes, by k % 13 < 7, one of the pre-activations 0, +-20, +-100, +-200 in gi with gh = 0 there
    (+-100 / +200 saturate a gate; -200 makes u exactly 0, +100 and +200 exactly 1)"""
    g = torch.Generator().manual_seed(seed)
    gi, gh, m0 = torch.randn(B, 3 * R, generator=g) * 2, torch.randn(B, 3 * R, generator=g) * 2, torch.randn(B, R, generator=g)
    k = torch.arange(B * 3 * R).view(B, 3 * R) + torch.arange(B)[:, None] * 5          # the rows start at different phases
    for i, v in enumerate(EDGES):
        sel = (k % 13) == i
        gi[sel] = v
        gh[sel & (torch.arange(3 * R)[None, :] < 2 * R)] = 0.0                          # r and u: the sum is the edge value; n keeps r * gh_n
    return gi.contiguous(), gh.contiguous(), m0.contiguous()


def _clear(kind, B):
    c = torch.zeros(B, dtype=torch.uint8)
    if kind == "all":
        c[:] = 1
    elif kind == "alternating":
        c[::2] = 1
    return c


def _cell_forward(gi, gh, m0, clear_next, B, R, with_next=True):
    gates, m1 = Guarded(B, 3 * R), Guarded(B, R, front=21, back=17)
    nxt = Guarded(B, R, front=17, back=29) if with_next else None
    rc = learn.lib().pgtt_learn_gru_cell_forward(_p(gi), _p(gh), _p(m0), _p(clear_next), B, R, _p(gates), _p(m1), _p(nxt), _st())
    assert rc == 0, _msg()
    return gates, m1, nxt


@pytest.mark.parametrize("R", [16, 48, 256])
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_cell_forward_and_backward(B, R):
    gi, gh, m_prev = _cell_inputs(B, R, 1000 * B + R)
    lib = learn.lib()
    for kind in ("none", "all", "alternating"):
        clear, clear_next = _clear(kind, B), _clear(kind, B).flip(0)
        # ---- the clear: a cleared row is exactly 0 and its m is not read (NaN there)
        mp = m_prev.clone()
        mp[clear.bool()] = float("nan")
        m0g = Guarded(B, R)
        dmp, dclear, dcn = mp.cuda(), clear.cuda(), clear_next.cuda()                  # named: a temporary's block could be handed out again before the launch
        assert lib.pgtt_learn_gru_clear_rows(_p(dmp), _p(dclear), B, R, _p(m0g), _st()) == 0, _msg()
        want0 = torch.where(clear.bool()[:, None], torch.zeros(()), m_prev)
        assert m0g.guards_intact() and torch.equal(m0g.view.cpu(), want0)
        m0 = want0.contiguous()
        # ---- forward
        dgi, dgh, dm0 = gi.cuda(), gh.cuda(), m0.cuda()
        gates, m1, nxt = _cell_forward(dgi, dgh, dm0, dcn, B, R)
        assert gates.written() and m1.written() and nxt.guards_intact()
        g2, m2, n2 = _cell_forward(dgi, dgh, dm0, dcn, B, R)
        assert torch.equal(gates.view, g2.view) and torch.equal(m1.view, m2.view) and torch.equal(nxt.view, n2.view)      # two calls, equal bits
        gi64, gh64, m064 = f64(gi), f64(gh), f64(m0)
        r, u, n, m1_64 = rref.cell(gi64, gh64, m064)
        r_bar = sig_bar(r, U * (gi64[:, :R] + gh64[:, :R]).abs())
        u_bar = sig_bar(u, U * (gi64[:, R:2 * R] + gh64[:, R:2 * R]).abs())
        ghn = gh64[:, 2 * R:]
        pre_n = gi64[:, 2 * R:] + r * ghn
        n_bar = tanh_bar(n, ghn.abs() * r_bar + U * (r * ghn).abs() + U * pre_n.abs())
        bar = m1_bar(u, n, m064, m1_64, u_bar, n_bar) + 1e-45                       # + 1e-45: no 0 / 0 where a cleared row's m1 is exactly 0
        got = gates.f64()
        worst = {"r": ((got[:, :R] - r).abs() / r_bar).max(), "u": ((got[:, R:2 * R] - u).abs() / u_bar).max(),
                 "n": ((got[:, 2 * R:] - n).abs() / n_bar).max(), "m1": ((m1.f64() - m1_64).abs() / bar).max()}
        print(f"cell forward B={B} R={R} clear={kind}: worst / bar " + "  ".join(f"{k} {float(v):.3f}" for k, v in worst.items()))
        assert all(float(v) <= 1.0 for v in worst.values()), worst
        assert bool(torch.isfinite(gates.view).all()) and bool(torch.isfinite(m1.view).all())
        gu, gn = gates.view[:, R:2 * R], gates.view[:, 2 * R:]
        one, zero = gu == 1.0, gu == 0.0
        assert bool(one.any()) and bool(zero.any())                                    # u exactly 1 and exactly 0 are among the inputs
        assert torch.equal(m1.view[one], dm0[one]) and torch.equal(m1.view[zero], gn[zero])      # u = 1 keeps m0 exactly, u = 0 takes n
        cn = dcn.bool()
        assert torch.equal(nxt.view[~cn], m1.view[~cn]) and bool((nxt.view[cn] == 0).all())      # the next step's m0: exactly 0 where it is cleared
        _, m1b, none = _cell_forward(dgi, dgh, dm0, None, B, R, with_next=False)                  # both optional pointers NULL
        assert none is None and torch.equal(m1b.view, m1.view)
        # ---- backward, from the kernel's own (fp32) gates: both sides read the same numbers
        gen = torch.Generator().manual_seed(B + R)
        dm1h, dnext = torch.randn(B, R, generator=gen), torch.randn(B, R, generator=gen)
        ddm1h = dm1h.cuda()
        outs = []
        for variant in ("next", "next_moved", "last"):
            dn_in = None if variant == "last" else (dnext if variant == "next" else dnext + torch.where(clear_next.bool()[:, None], 5.0, 0.0)).cuda()
            o = (Guarded(B, 3 * R), Guarded(B, 3 * R, front=21, back=17), Guarded(B, R, front=17, back=29))
            rc = lib.pgtt_learn_gru_cell_backward(_p(gates.view), _p(dgh), _p(dm0), _p(ddm1h), _p(dn_in), None if variant == "last" else _p(dcn),
                                                  B, R, _p(o[0]), _p(o[1]), _p(o[2]), _st())
            assert rc == 0, _msg()
            assert all(x.written() for x in o)
            outs.append(o)
        # what comes back from a cleared next step is exactly 0: moving it there changes no bit
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(a.view, b.view)
        for variant, o in (("next", outs[0]), ("last", outs[2])):
            s = {"r": f64(gates.view[:, :R]), "u": f64(gates.view[:, R:2 * R]), "n": f64(gates.view[:, 2 * R:]), "m0": m064, "gh": gh64}
            a, b = f64(dm1h), (torch.zeros(B, R, dtype=F64) if variant == "last" else torch.where(clear_next.bool()[:, None], torch.zeros((), dtype=F64), f64(dnext)))
            dm1 = a + b
            dgi64, dgh64, direct64 = rref.cell_backward(s, dm1)
            dn_ = dm1 * (1 - s["u"])
            dpn, dpu = dgi64[:, 2 * R:], dgi64[:, R:2 * R]
            dpn_bar = 4 * U * dpn.abs() + U * dn_.abs()
            dpu_bar = 6 * U * dpu.abs()
            dr = ghn * dpn
            dr_bar = ghn.abs() * dpn_bar + U * dr.abs()
            dpr_bar = s["r"] * (1 - s["r"]) * dr_bar + 3 * U * dgi64[:, :R].abs()
            dghn_bar = s["r"] * dpn_bar + U * dgh64[:, 2 * R:].abs()
            bars_gi = torch.cat([dpr_bar, dpu_bar, dpn_bar], -1) + TINY
            bars_gh = torch.cat([dpr_bar, dpu_bar, dghn_bar], -1) + TINY
            w = {"dgi": ((o[0].f64() - dgi64).abs() / bars_gi).max(), "dgh": ((o[1].f64() - dgh64).abs() / bars_gh).max(),
                 "dm0": ((o[2].f64() - direct64).abs() / (2 * U * direct64.abs() + TINY)).max()}
            print(f"cell backward B={B} R={R} clear={kind} {variant}: worst / bar " + "  ".join(f"{k} {float(v):.3f}" for k, v in w.items()))
            assert all(float(v) <= 1.0 for v in w.values()), w


def test_add_rows_and_the_refusals_of_the_pieces():
    lib = learn.lib()
    a, b = torch.randn(1001).cuda(), torch.randn(1001).cuda()
    out = Guarded(1001)
    assert lib.pgtt_learn_add_rows(_p(a), _p(b), 1001, _p(out), _st()) == 0
    assert out.guards_intact() and torch.equal(out.view, a + b)
    c = a.clone()
    assert lib.pgtt_learn_add_rows(_p(c), _p(b), 1001, _p(c), _st()) == 0 and torch.equal(c, a + b)         # in place
    B, R = 5, 16
    gi, gh, m0, cl = torch.zeros(B, 48).cuda(), torch.zeros(B, 48).cuda(), torch.zeros(B, R).cuda(), torch.zeros(B, dtype=torch.uint8).cuda()
    o = [Guarded(B, 48), Guarded(B, 48), Guarded(B, R), Guarded(B, R)]
    calls = []
    for bad in range(3):
        args = [a, b, 1001, o[2]]
        args[bad if bad < 2 else 3] = None
        calls.append(lambda args=args: lib.pgtt_learn_add_rows(_p(args[0]), _p(args[1]), args[2], _p(args[3]), _st()))
    calls.append(lambda: lib.pgtt_learn_add_rows(_p(a), _p(b), 0, _p(o[2]), _st()))
    for Rbad in (0, 8, 24, 272):
        calls.append(lambda Rbad=Rbad: lib.pgtt_learn_gru_clear_rows(_p(m0), _p(cl), B, Rbad, _p(o[2]), _st()))
        calls.append(lambda Rbad=Rbad: lib.pgtt_learn_gru_cell_forward(_p(gi), _p(gh), _p(m0), None, B, Rbad, _p(o[0]), _p(o[2]), _p(o[3]), _st()))
        calls.append(lambda Rbad=Rbad: lib.pgtt_learn_gru_cell_backward(_p(gi), _p(gh), _p(m0), _p(m0), None, None, B, Rbad, _p(o[0]), _p(o[1]), _p(o[2]), _st()))
    for Bbad in (0, -3):
        calls.append(lambda Bbad=Bbad: lib.pgtt_learn_gru_clear_rows(_p(m0), _p(cl), Bbad, R, _p(o[2]), _st()))
        calls.append(lambda Bbad=Bbad: lib.pgtt_learn_gru_cell_forward(_p(gi), _p(gh), _p(m0), None, Bbad, R, _p(o[0]), _p(o[2]), None, _st()))
        calls.append(lambda Bbad=Bbad: lib.pgtt_learn_gru_cell_backward(_p(gi), _p(gh), _p(m0), _p(m0), None, None, Bbad, R, _p(o[0]), _p(o[1]), _p(o[2]), _st()))
    fw = [gi, gh, m0, o[0], o[2]]
    for k in range(5):
        x = list(fw); x[k] = None
        calls.append(lambda x=x: lib.pgtt_learn_gru_cell_forward(_p(x[0]), _p(x[1]), _p(x[2]), None, B, R, _p(x[3]), _p(x[4]), None, _st()))
    bw = [gi, gh, m0, m0, o[0], o[1], o[2]]
    for k in range(7):
        x = list(bw); x[k] = None
        calls.append(lambda x=x: lib.pgtt_learn_gru_cell_backward(_p(x[0]), _p(x[1]), _p(x[2]), _p(x[3]), None, None, B, R, _p(x[4]), _p(x[5]), _p(x[6]), _st()))
    cr = [m0, cl, o[2]]
    for k in range(3):
        x = list(cr); x[k] = None
        calls.append(lambda x=x: lib.pgtt_learn_gru_clear_rows(_p(x[0]), _p(x[1]), B, R, _p(x[2]), _st()))
    for i, call in enumerate(calls):
        assert call() == E_ARG and _msg().startswith("pgtt_learn_"), i
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o)


# ------------------------------------------------------------------ pgtt_learn_recurrent_act
OD, DIMS = 171, (171, 512, 256, 128, 24)
TRUNK = DIMS[:4]                                                                    # (od, h1, h2, h3) of policy177
SMALL = [((5, 16, 16, 16), 16, 17), ((171, 64, 32, 48), 80, 33), ((20, 32, 48, 144), 256, 17)]       # (od, h1, h2, h3), R, N: one kb trip; h3 no power of two
_CACHE = {}


def _policy(R, trunk=TRUNK):
    """policy177's layers, seeded GRU tensors, a non-zero W_m; for another trunk (od, h1, h2, h3) a seeded RecurrentPolicy as
    test_gpu_recurrent_distill._policy builds it, with statistics away from (0, 1); built once per (R, trunk)"""
    trunk = tuple(trunk)
    if (R, trunk) not in _CACHE:
        if trunk == TRUNK:
            pi = RecurrentPolicy.from_teacher(PolicyMLP(os.path.join(POLICY_DIR, "policy177.npz")), R, seed=7)
            with torch.no_grad():
                pi.mem_w.copy_(torch.randn(24, R, generator=torch.Generator().manual_seed(R)) * 0.2)
        else:
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(1000 * R + sum(trunk))
                pi = RecurrentPolicy(trunk + (24,), R)
                cell = torch.nn.GRUCell(trunk[3], R)
                with torch.no_grad():
                    pi.gru_w_ih.copy_(cell.weight_ih); pi.gru_w_hh.copy_(cell.weight_hh); pi.gru_b_ih.copy_(cell.bias_ih); pi.gru_b_hh.copy_(cell.bias_hh)
                    pi.mem_w.copy_(torch.randn(24, R) * 0.3)
                    pi.layers[3].weight.mul_(3.0); pi.layers[3].bias.add_(torch.randn(24) * 0.3)
                    pi.mean.copy_(torch.randn(trunk[0]) * 2 + 0.5); pi.std.copy_(torch.rand(trunk[0]) * 2 + 0.1)
        pi.requires_grad_(False)
        _CACHE[(R, trunk)] = pi
    return _CACHE[(R, trunk)]


def _P(pi):
    return {"mean": pi.mean, "std": pi.std, "w": [l.weight for l in pi.layers], "b": [l.bias for l in pi.layers],
            "w_ih": pi.gru_w_ih, "w_hh": pi.gru_w_hh, "b_ih": pi.gru_b_ih, "b_hh": pi.gru_b_hh, "w_m": pi.mem_w}


def _inputs(pi, N, seed):
    g = torch.Generator().manual_seed(seed)
    obs = (pi.mean + pi.std * torch.randn(N, pi.dims[0], generator=g)).contiguous()
    return obs, torch.randn(N, pi.memory, generator=g).contiguous()


class Act:
    """one call of pgtt_learn_recurrent_act with guarded outputs; the weights live on the device once per policy.  The trunk (od, h1, h2, h3) is the
    policy's: the scratch is sized for it by pgtt_learn_recurrent_act_work_floats and sits between guard bands like every output"""

    def __init__(self, pi, N, T=3, head=True, stores=True):
        R = pi.memory
        OD, H1, H2, H3 = self.trunk = tuple(pi.dims[:4])
        self.pi, self.N, self.R, self.T = pi, N, R, T
        self.dev = {k: (v.cuda().contiguous() if torch.is_tensor(v) else [t.cuda().contiguous() for t in v]) for k, v in _P(pi).items()}
        self.mem, self.action = Guarded(N, R), Guarded(N, 12, front=21, back=17)
        self.head = Guarded(N, 24, front=17, back=29) if head else None
        self.s_obs = Guarded(T, N, OD) if stores else None
        self.s_mem0 = Guarded(T, N, R, front=21, back=17) if stores else None
        self.s_clear = Guarded(T, N, dtype=torch.uint8, fill=7, front=5, back=3) if stores else None
        floats = int(learn.lib().pgtt_learn_recurrent_act_work_floats(N, OD, H1, H2, H3))
        assert floats == N * (OD + H1 + H2 + H3 + max(H1, H2, H3))                    # x, h1, h2, h3 in this order, then the pre-activations
        self.work_guarded = Guarded(floats, front=20, back=23)                         # 80 bytes in front: the scratch keeps torch's 16-byte alignment
        self.work = self.work_guarded.view

    def h3(self):
        """the trunk's output [N, h3] as the last call left it in the scratch"""
        OD, H1, H2, H3 = self.trunk
        lo = self.N * (OD + H1 + H2)
        return self.work[lo:lo + self.N * H3].view(self.N, H3)

    def args(self, obs, t=0, clear_all=0, clear_mask=None, done=None, use_done=0):
        a, d = PgttLearnRecurrentActArgs(), self.dev
        a.obs, a.mean, a.std = obs.data_ptr(), d["mean"].data_ptr(), d["std"].data_ptr()
        for i in range(4):
            setattr(a, f"w{i}", d["w"][i].data_ptr()); setattr(a, f"b{i}", d["b"][i].data_ptr())
        a.w_ih, a.w_hh, a.b_ih, a.b_hh, a.w_m = (d[k].data_ptr() for k in ("w_ih", "w_hh", "b_ih", "b_hh", "w_m"))
        a.done, a.clear_mask = _p(done), _p(clear_mask)
        a.mem, a.action, a.head, a.work = self.mem.ptr(), self.action.ptr(), _p(self.head), self.work.data_ptr()
        a.store_obs, a.store_mem0, a.store_clear = _p(self.s_obs), _p(self.s_mem0), _p(self.s_clear)
        a.num_envs, a.memory = self.N, self.R
        a.obs_dim, a.h1, a.h2, a.h3 = self.trunk
        a.t, a.store_rows, a.clear_all, a.use_done = t, self.T, clear_all, use_done
        return a

    def run(self, obs, mem, **kw):
        self.mem.view.copy_(mem)
        self._keep = (obs.cuda().contiguous(), {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()})
        rc = learn.lib().pgtt_learn_recurrent_act(C.byref(self.args(self._keep[0], **self._keep[1])), _st())
        assert rc == 0, _msg()
        torch.cuda.synchronize()
        return self


def _act_bars(pi, obs, mem, clear, h3=None):
    """fp64 outputs and the propagated bars of the docstring; with h3 (the trunk's fp32 output as the kernel left it in `work`) everything from h3
    on is taken from those bits as exact inputs: the bars of the new kernel alone, h3_bar = 0"""
    P = rref.params64(_P(pi))
    R = pi.memory
    s = rref.step(_P(pi), obs, mem, clear)
    x = (f64(obs) - P["mean"]) / P["std"]
    h, h_bar = x, 2 * U * x.abs()
    for w, b in zip(P["w"][:3], P["b"][:3]):
        z = h @ w.T + b
        z_bar = (w.shape[1] + 2) * U * (h.abs() @ w.abs().T + b.abs()) + h_bar @ w.abs().T
        h = rref.silu(z)
        h_bar = 1.1 * z_bar + 6 * U * h.abs()
    if h3 is not None:
        h, h_bar = f64(h3), torch.zeros_like(h_bar)
        gi, gh = h @ P["w_ih"].T + P["b_ih"], s["m0"] @ P["w_hh"].T + P["b_hh"]
        r, u, n, m1 = rref.cell(gi, gh, s["m0"])
        head = h @ P["w"][3].T + P["b"][3] + m1 @ P["w_m"].T
        s = dict(s, gi=gi, gh=gh, r=r, u=u, n=n, mem=m1, head=head, action=torch.tanh(head[:, :12]))
    H = h.shape[1]
    m0 = s["m0"]
    Wi, Wh, bi, bh = P["w_ih"], P["w_hh"], P["b_ih"], P["b_hh"]
    mag_i, mag_h = h.abs() @ Wi.abs().T, m0.abs() @ Wh.abs().T
    prop = h_bar @ Wi.abs().T
    dv = (H + R + 3) * U * (mag_i + mag_h + bi.abs() + bh.abs()) + prop                      # the chains of r and u
    r_bar, u_bar = sig_bar(s["r"], dv[:, :R]), sig_bar(s["u"], dv[:, R:2 * R])
    gin_bar = (H + 2) * U * (mag_i + bi.abs())[:, 2 * R:] + prop[:, 2 * R:]
    ghn_bar = (R + 2) * U * (mag_h + bh.abs())[:, 2 * R:]
    ghn = s["gh"][:, 2 * R:]
    pre_n = s["gi"][:, 2 * R:] + s["r"] * ghn
    n_bar = tanh_bar(s["n"], gin_bar + s["r"] * ghn_bar + ghn.abs() * r_bar + U * (s["r"] * ghn).abs() + U * pre_n.abs())
    mem_bar = m1_bar(s["u"], s["n"], m0, s["mem"], u_bar, n_bar) + 1e-45
    W3, b3, Wm = P["w"][3], P["b"][3], P["w_m"]
    head_bar = (H + R + 2) * U * (h.abs() @ W3.abs().T + s["mem"].abs() @ Wm.abs().T + b3.abs()) + h_bar @ W3.abs().T + mem_bar @ Wm.abs().T
    act_bar = tanh_bar(s["action"], head_bar[:, :12])
    return s, {"head": head_bar, "action": act_bar, "mem": mem_bar}


# The tail walks the memory tiles with ct = wave, wave + 4, .. < R / 16.  R = 16: wave 0 alone; 32, 48: whole waves reach the barrier without a tile;
# 64: one tile per wave; 80: wave 0 makes a second trip, the others one; 256: four trips per wave and the largest LDS (33,280 bytes dynamic).
# The first ten ids are the cases this test had before the others were added.
ACT_CASES = [pytest.param(N, R, TRUNK, id=f"{N}-{R}") for R in (16, 64) for N in (1, 15, 16, 17, 65)]
ACT_CASES += [pytest.param(N, R, TRUNK, id=f"{N}-{R}") for R, N in ((32, 17), (48, 1), (48, 33), (80, 17), (80, 33), (256, 1), (256, 17), (256, 33))]
ACT_CASES += [pytest.param(N, R, trunk, id=f"{N}-{R}-" + "x".join(str(d) for d in trunk)) for trunk, R, N in SMALL]


@pytest.mark.parametrize("N,R,trunk", ACT_CASES)
def test_recurrent_act_against_fp64(N, R, trunk):
    pi = _policy(R, trunk)
    assert tuple(pi.dims[:4]) == tuple(trunk) and pi.memory == R
    obs, mem = _inputs(pi, N, 10 * N + R)
    clear = torch.zeros(N, dtype=torch.bool)
    clear[N // 2] = True
    a = Act(pi, N).run(obs, mem, t=1, clear_mask=clear.to(torch.uint8))
    assert a.mem.written() and a.action.written() and a.head.written() and a.work_guarded.guards_intact()
    want, bars = _act_bars(pi, obs, mem, clear)
    worst = {k: float(((getattr(a, k).f64() - want[k]).abs() / bars[k]).max()) for k in ("head", "action", "mem")}
    print(f"recurrent act N={N} R={R} trunk={trunk}: worst / bar " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    # the new kernel alone: from the h3 the trunk left in `work` (x, h1, h2, h3 in this order), taken as exact
    h3 = a.h3()
    want3, bars3 = _act_bars(pi, obs, mem, clear, h3=h3)
    worst3 = {k: float(((getattr(a, k).f64() - want3[k]).abs() / bars3[k]).max()) for k in ("head", "action", "mem")}
    print(f"recurrent act N={N} R={R} trunk={trunk} from the kernel's h3: worst / bar " + "  ".join(f"{k} {v:.2e}" for k, v in worst3.items()))
    assert all(v <= 1.0 for v in worst3.values()), worst3
    # the stored rows: row t = 1 holds the inputs' bits, rows 0 and 2 and every guard band are untouched
    od = obs.cuda()
    assert a.s_obs.guards_intact() and a.s_mem0.guards_intact() and a.s_clear.guards_intact()
    assert torch.equal(a.s_obs.view[1], od) and torch.equal(a.s_mem0.view[1].cpu(), want["m0"].float()) and torch.equal(a.s_clear.view[1].cpu(), clear.to(torch.uint8))
    for t in (0, 2):
        assert bool((a.s_obs.view[t] == SENT).all()) and bool((a.s_mem0.view[t] == SENT).all()) and bool((a.s_clear.view[t] == 7).all())
    first = (a.mem.view.clone(), a.action.view.clone(), a.head.view.clone())
    for t in (0, 2):                                                                # t = 0 and t = T - 1; two calls give equal bits
        a.run(obs, mem, t=t, clear_mask=clear.to(torch.uint8))
        assert torch.equal(a.s_obs.view[t], od) and torch.equal(a.s_mem0.view[t], a.s_mem0.view[1]) and torch.equal(a.s_clear.view[t], a.s_clear.view[1])
        assert all(torch.equal(x, y) for x, y in zip(first, (a.mem.view, a.action.view, a.head.view)))
    assert a.s_obs.guards_intact() and a.s_mem0.guards_intact() and a.s_clear.guards_intact()
    # head == NULL and no stores
    b = Act(pi, N, head=False, stores=False).run(obs, mem, clear_mask=clear.to(torch.uint8))
    assert torch.equal(b.mem.view, first[0]) and torch.equal(b.action.view, first[1]) and b.action.guards_intact() and b.mem.guards_intact()


@pytest.mark.parametrize("R", [16, 64, 80, 256])
def test_recurrent_act_rows_do_not_depend_on_the_batch(R):
    pi = _policy(R)
    obs, mem = _inputs(pi, 65, 3 + R)
    obs[64], mem[64] = obs[0], mem[0]                                               # the same env at positions 0 and N - 1, and alone
    big = Act(pi, 65).run(obs, mem)
    one = Act(pi, 1).run(obs[:1], mem[:1])
    for k in ("mem", "action", "head"):
        g = getattr(big, k).view
        assert torch.equal(g[0], g[64]) and torch.equal(g[0], getattr(one, k).view[0]), k
    # a cleared env whose memory row is NaN: the bits of the same env with a zero row, and finite outputs
    mask = torch.zeros(65, dtype=torch.uint8); mask[5] = 1; mask[64] = 1
    poisoned = mem.clone(); poisoned[5] = float("nan"); poisoned[64] = float("nan")
    zeroed = mem.clone(); zeroed[5] = 0; zeroed[64] = 0
    a = Act(pi, 65).run(obs, poisoned, clear_mask=mask)
    b = Act(pi, 65).run(obs, zeroed)
    for k in ("mem", "action", "head"):
        assert torch.equal(getattr(a, k).view, getattr(b, k).view) and bool(torch.isfinite(getattr(a, k).view).all()), k


def test_recurrent_act_clears_exactly_the_envs_named():
    for R in (16, 80):                                                              # one tile in wave 0; unequal trip counts among the waves
        _clears_exactly_the_envs_named(R)


def _clears_exactly_the_envs_named(R):
    pi = _policy(R)
    N = 33
    obs, mem = _inputs(pi, N, 77)
    named = torch.zeros(N, dtype=torch.bool); named[[0, 7, 16, 32]] = True
    zeroed = torch.where(named[:, None], torch.zeros(()), mem)
    want_some = Act(pi, N).run(obs, zeroed)
    want_all = Act(pi, N).run(obs, torch.zeros_like(mem))
    want_none = Act(pi, N).run(obs, mem)
    nan_some = torch.where(named[:, None], torch.full((), float("nan")), mem)
    flags_u8, flags_f = named.to(torch.uint8), named.float()
    cases = [("clear_all", dict(clear_all=1), torch.full_like(mem, float("nan")), want_all, torch.ones(N, dtype=torch.uint8)),
             ("clear_mask", dict(clear_mask=flags_u8), nan_some, want_some, flags_u8),
             ("use_done", dict(done=flags_f, use_done=1), nan_some, want_some, flags_u8),
             ("done without use_done", dict(done=flags_f, use_done=0), mem, want_none, torch.zeros(N, dtype=torch.uint8)),
             ("use_done without done", dict(use_done=1), mem, want_none, torch.zeros(N, dtype=torch.uint8))]
    for name, kw, mem_in, want, flags in cases:
        a = Act(pi, N).run(obs, mem_in, t=0, **kw)
        for k in ("mem", "action", "head"):
            assert torch.equal(getattr(a, k).view, getattr(want, k).view), (R, name, k)
        assert torch.equal(a.s_clear.view[0].cpu(), flags), (R, name)
        assert bool((a.s_mem0.view[0][flags.bool().cuda()] == 0).all()), (R, name)


def test_recurrent_act_refusals():
    pi = _policy(16)
    N = 5
    obs, mem = _inputs(pi, N, 1)
    a = Act(pi, N)
    a.mem.view.fill_(SENT)
    dobs = obs.cuda()
    lib = learn.lib()
    required = ["obs", "mean", "std", "w0", "w1", "w2", "w3", "b0", "b1", "b2", "b3", "w_ih", "w_hh", "b_ih", "b_hh", "w_m", "mem", "action", "work"]
    cases = [(k, None) for k in required]
    cases += [(k, v) for k in ("num_envs", "obs_dim", "h1", "h2", "h3") for v in (0, -1)]
    cases += [("memory", v) for v in (0, 8, 24, 272)] + [("h3", 120), ("t", -1), ("t", 3), ("store_rows", 0)]
    for k, v in cases:
        args = a.args(dobs, t=0)
        setattr(args, k, v)
        assert lib.pgtt_learn_recurrent_act(C.byref(args), _st()) == E_ARG, (k, v)
        assert _msg().startswith("pgtt_learn_recurrent_act"), (k, v)
    assert lib.pgtt_learn_recurrent_act(None, _st()) == E_ARG
    torch.cuda.synchronize()
    for g in (a.mem, a.action, a.head, a.s_obs, a.s_mem0, a.s_clear):
        assert g.untouched()
    assert lib.pgtt_learn_recurrent_act_work_floats(0, 171, 512, 256, 128) == 0
    assert lib.pgtt_learn_recurrent_act_work_floats(4, 171, 512, 256, 128) == 4 * (171 + 512 + 256 + 128 + 512)


def test_with_a_zero_read_out_the_actor_is_the_feed_forward_actor():
    """W_m = 0 and policy177's weights: the action is within the derived bar of fp64 and within 1e-5 of FusedActor.act(deterministic=True) on the same
    observation - two summation orders of the same numbers"""
    import numpy as np
    from phase_guided_terrain_traversal_amd import configs
    from phase_guided_terrain_traversal_amd.acting import FusedActor
    from phase_guided_terrain_traversal_amd.env import Joystick
    from phase_guided_terrain_traversal_amd.recurrent_policy import RecurrentActor
    teacher = PolicyMLP(os.path.join(POLICY_DIR, "policy177.npz"))
    pi = RecurrentPolicy.from_teacher(teacher, 16, seed=0)
    pi.requires_grad_(False)
    n = 32
    terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level1.npy"))
    variant = np.random.default_rng(0).integers(0, terrain.shape[0], n).astype(np.int32)
    env = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", variant=torch.from_numpy(variant), autoreset=True)
    env.reset(3)
    ff = FusedActor(env, 1, seed=0)
    ff.load([(m.weight, m.bias) for m in teacher.layers], teacher.mean, teacher.std)
    rec = RecurrentActor(env, 2, 16)
    rec.load(pi)
    for t in range(2):
        head = torch.zeros(n, 24, device="cuda")
        obs = env.buffers["obs_state"].clone()
        rec.act(t, head=head)
        ff.act(deterministic=True, store=False)
        torch.cuda.synchronize()
        assert float((rec.action - ff.action).abs().max()) <= 1e-5
        want, bars = _act_bars(pi, obs.cpu(), rec.storage["mem0"][t].cpu(), rec.storage["clear"][t].cpu().bool())
        assert float(((f64(rec.action) - want["action"]).abs() / bars["action"]).max()) <= 1.0
        assert float(((f64(head) - want["head"]).abs() / bars["head"]).max()) <= 1.0
        assert torch.equal(rec.storage["obs"][t], obs)
        env.step(rec.action)
    assert bool((rec.storage["clear"][0] == 1).all()) and bool((rec.storage["mem0"][0] == 0).all())    # the first call clears every env
    env.close()
