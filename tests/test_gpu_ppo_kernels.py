"""The two trainer kernels of csrc/pgtt_ppo.hip through the bare C ABI (include/pgtt_train.h), against fp64 (tests/ppo_reference.py):

pgtt_ppo_linear_backward - an EXACT leg (small-integer inputs: every product and partial sum is an integer below 2^24, so dW and db must equal
the integer result bit for bit at every shape and every split S), a rounding leg at the trainer's real shapes with an elementwise worst-case
bound, and the frame (guarded scratch / outputs, determinism, refused arguments).
pgtt_ppo_policy_loss - all three entries of loss_3 and the whole gradient against fp64 under an error model built from the magnitude of the
terms of each sample's log-probability; the PyTorch-op fp32 form goes through the same comparison, so the model is not tuned to the kernel."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ppo_reference as ref

E_ARG = -1            # PGTT_E_ARG of include/pgtt.h
SENT = -777.25        # sentinel of the guard zones
G = 67                # guard floats on either side of a view (odd: the ABI promises float alignment only)


def _lib():
    from phase_guided_terrain_traversal_amd import native
    return native.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """n floats in the middle of a sentinel-filled allocation"""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * G,), SENT, device="cuda")
        self.view = self.buf[G:G + n]
        self.n = n

    def guards_intact(self):
        return bool((self.buf[:G] == SENT).all()) and bool((self.buf[G + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def plan(K, S):
    """the chunking of pgtt_ppo_linear_backward restated: even chunk height, planes actually used"""
    kc = (K + S - 1) // S
    kc += kc & 1
    return kc, (K + kc - 1) // kc


def linear_backward(x, dy, S, partial=None, dw=None, db=None):
    K, M = x.shape
    N = dy.shape[1]
    partial = partial or Guarded(S * (N * M + N))
    dw, db = dw or Guarded(N * M), db or Guarded(N)
    rc = _lib().pgtt_ppo_linear_backward(_ptr(x), _ptr(dy), C.c_int(K), C.c_int(M), C.c_int(N), C.c_int(S), _ptr(partial.view), _ptr(dw.view), _ptr(db.view), _stream())
    torch.cuda.synchronize()
    return rc, partial, dw, db


KS = (1, 2, 3, 15, 16, 17, 31, 33, 640, 1031, 1280, 2560, 5120)
MS = (1, 12, 24, 31, 32, 33, 63, 64, 65, 171, 215, 512)
NS = (1, 24, 33, 64, 65, 128, 512)
SS = (1, 2, 3, 7, 8, 9, 23, 24, 63, 64)


def exact_cases():
    """every (K, S) pair once, walking the 84 (M, N) pairs with a stride coprime to 84 so that each occurs at least once (130 cases), then the
    corners: the widest tile grid at every K, the trainer's shapes at splits that are not multiples of 8, single rows and columns"""
    mn = [(m, n) for m in MS for n in NS]
    cases, j = [], 0
    for K in KS:
        for S in SS:
            cases.append((K, *mn[(37 * j) % len(mn)], S)); j += 1
    cases += [(K, 512, 512, S) for K, S in ((1, 64), (15, 8), (17, 9), (33, 23), (1031, 7), (5120, 3), (5120, 63))]
    cases += [(K, M, N, S) for K in (5120, 1280) for (M, N) in ((171, 512), (215, 512), (128, 24), (128, 1)) for S in (7, 23, 63)]
    cases += [(1, 1, 1, 1), (2, 1, 1, 2), (3, 65, 65, 2), (16, 64, 64, 8), (31, 33, 33, 24), (640, 63, 65, 9), (2560, 65, 33, 63)]
    return cases


def test_linear_backward_exact_sweep_covers_the_edges():
    """what the sweep must contain, from the restated kc / Sused arithmetic (no GPU work)"""
    cases = exact_cases()
    assert 150 <= len(cases) <= 200, len(cases)
    used = [plan(K, S)[1] for K, M, N, S in cases]
    assert sum(1 for s in used if s % 8 != 0 and s > 8) >= 20          # the reduce kernel's tail loop after at least one full group of eight
    assert sum(1 for s in used if 0 < s < 8) >= 20                     # ... and with no full group
    assert sum(1 for (K, M, N, S), s in zip(cases, used) if s < S) >= 20
    assert sum(1 for K, M, N, S in cases if K < 16) >= 20
    assert any(plan(K, S)[0] > K - (plan(K, S)[1] - 1) * plan(K, S)[0] for K, M, N, S in cases)      # a short last chunk
    for dim in (1, 2):
        seen = {c[dim] for c in cases}
        assert {31, 33} & seen and {63, 65} & seen and {24, 33, 64, 65} & seen, seen
    assert {(m, n) for _, m, n, _ in cases} >= {(m, n) for m in MS for n in NS}


def test_linear_backward_exact():
    """integers in [-3, 3]: |sum| <= 9 K <= 46080 < 2^24, every fp32 step is exact, so dW / db equal the integer result whatever the order.
    A dropped or doubled row, a wrong column mask or plane count shows as a whole number."""
    g = torch.Generator(device="cuda").manual_seed(17)
    bad = []
    for K, M, N, S in exact_cases():
        x = torch.randint(-3, 4, (K, M), device="cuda", generator=g).float()
        dy = torch.randint(-3, 4, (K, N), device="cuda", generator=g).float()
        rc, partial, dw, db = linear_backward(x, dy, S)
        assert rc == 0, (K, M, N, S, rc)
        want_w = (dy.double().T @ x.double()).to(torch.int64)          # fp64 products of small integers: exact
        want_b = dy.double().sum(0).to(torch.int64)
        got_w, got_b = dw.view.view(N, M), db.view
        ok = (bool((got_w == got_w.round()).all()) and torch.equal(got_w.to(torch.int64), want_w) and torch.equal(got_b.to(torch.int64), want_b)
              and bool((got_b == got_b.round()).all()))
        frame = partial.guards_intact() and dw.guards_intact() and db.guards_intact()
        if not (ok and frame):
            bad.append((K, M, N, S, plan(K, S), "values" if not ok else "frame", int((got_w.to(torch.int64) != want_w).sum()), int((got_b.to(torch.int64) != want_b).sum())))
    assert not bad, (len(bad), bad[:10])


def trainer_split(K, M, N):
    """the S that ppo._LinearLongBatch.backward chooses (default PGTT_PPO_SPLITK)"""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    return max(1, min(64, 768 // tiles, K // 16))


ROUNDING_SHAPES = [(K, M, N) for K in (5120, 2560, 1280) for (M, N) in ((171, 512), (215, 512), (512, 256), (256, 128), (128, 24), (128, 1))]


@pytest.mark.parametrize("spread", [False, True])
def test_linear_backward_rounding_at_trainer_shapes(spread):
    """random floats at the four policy layers, the four value layers (two shapes are shared) and K = 5120 / 2560 / 1280 with the trainer's own S:
    |dW - dW64|[n][m] <= 2 (kc / 2 + Sused + 2) 2^-24 (|dY|^T |X|)[n][m] elementwise (the chain of one plane plus the plane sum), the same with
    the column sums of |dY| for db.  `spread`: one shape with a 1e3 spread of column scales (small columns next to large ones)."""
    g = torch.Generator(device="cuda").manual_seed(23)
    worst = 0.0
    for K, M, N in (ROUNDING_SHAPES if not spread else [(5120, 171, 512)]):
        S = trainer_split(K, M, N)
        x = torch.randn(K, M, device="cuda", generator=g)
        dy = torch.randn(K, N, device="cuda", generator=g)
        if spread:
            x = x * torch.logspace(-1.5, 1.5, M, device="cuda")[torch.randperm(M, device="cuda", generator=g)]
            dy = dy * torch.logspace(-1.5, 1.5, N, device="cuda")[torch.randperm(N, device="cuda", generator=g)]
        rc, partial, dw, db = linear_backward(x, dy, S)
        assert rc == 0
        kc, sused, bw, bb = ref.linear_backward_bound(x, dy, K, S)
        assert (kc, sused) == plan(K, S)
        want_w, want_b = ref.f64(dy).T @ ref.f64(x), ref.f64(dy).sum(0)
        ew, eb = (ref.f64(dw.view).view(N, M) - want_w).abs(), (ref.f64(db.view) - want_b).abs()
        rw, rb = float((ew / bw).max()), float((eb / bb).max())
        worst = max(worst, rw, rb)
        print(f"K={K} M={M} N={N} S={S} kc={kc} Sused={sused}: worst |err| / bound dW {rw:.3f} db {rb:.3f}")
        assert bool((ew <= bw).all()) and bool((eb <= bb).all()), (K, M, N, S, rw, rb)
        assert partial.guards_intact() and dw.guards_intact() and db.guards_intact()
    print(f"spread={spread}: worst error / bound {worst:.3f}")


def test_linear_backward_frame():
    """two calls give the same bits; refused arguments leave every output at its sentinel"""
    g = torch.Generator(device="cuda").manual_seed(29)
    K, M, N, S = 1031, 171, 65, 23
    x, dy = torch.randn(K, M, device="cuda", generator=g), torch.randn(K, N, device="cuda", generator=g)
    rc1, p1, w1, b1 = linear_backward(x, dy, S)
    rc2, p2, w2, b2 = linear_backward(x, dy, S)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(w1.view.view(torch.int32), w2.view.view(torch.int32)) and torch.equal(b1.view.view(torch.int32), b2.view.view(torch.int32))
    L = _lib()
    part, dw, db = Guarded(S * (N * M + N)), Guarded(N * M), Guarded(N)
    for k_, m_, n_, s_ in ((0, M, N, S), (-1, M, N, S), (K, 0, N, S), (K, -5, N, S), (K, M, 0, S), (K, M, -1, S), (K, M, N, 0), (K, M, N, -3)):
        rc = L.pgtt_ppo_linear_backward(_ptr(x), _ptr(dy), C.c_int(k_), C.c_int(m_), C.c_int(n_), C.c_int(s_), _ptr(part.view), _ptr(dw.view), _ptr(db.view), _stream())
        assert rc == E_ARG, (k_, m_, n_, s_, rc)
    ptrs = [x, dy, part.view, dw.view, db.view]
    for hole in range(5):
        a = [None if i == hole else _ptr(t) for i, t in enumerate(ptrs)]
        rc = L.pgtt_ppo_linear_backward(a[0], a[1], C.c_int(K), C.c_int(M), C.c_int(N), C.c_int(S), a[2], a[3], a[4], _stream())
        assert rc == E_ARG, (hole, rc)
    torch.cuda.synchronize()
    assert part.untouched() and dw.untouched() and db.untouched()


# ---------------------------------------------------------------------------------------------------------------- pgtt_ppo_policy_loss
A = 12
CLIP, COST = 0.3, 1e-2
# ref.LOGP_OPS = 8 is a derived count of rounded operations per term of logp (ppo_reference.logp_error).  Measured on an MI355X with
# these inputs (worst error / tolerance over the gradient elements and the three loss entries, all seven cases; DESIGN.md "Trainer parity"):
#   B                     1      63     64     65     4097   5157   5157 (|u| <= 10)
#   PyTorch-op fp32 form  0.022  0.043  0.047  0.064  0.073  0.080  0.100
#   fused kernel          0.045  0.098  0.069  0.064  0.092  0.082  0.079
# The op form stays below 1.0, so the constant stands as derived (had it not: twice its worst ratio; the kernel's own result never sets it).


def loss_inputs(B, wide_u=False):
    """the inputs of test_fused_policy_loss_matches_autograd at height B, drawn on the CPU with seed 3: out ~ 1.5 randn, u = loc + 0.7 randn,
    logp_old = logp64 + 0.4 randn; for B > 128 one block of rows with raw scale 25 (softplus threshold branch) and one with -3 (small
    scales, |logp| ~ 1e4).  wide_u: loc uniform in [-10, 10], so |u| reaches 10 (the tanh correction's cancellation)."""
    g = torch.Generator().manual_seed(3)
    out = torch.randn(B, 2 * A, generator=g) * 1.5
    if B > 128:
        out[:64, A:] = 25.0; out[64:128, A:] = -3.0
    if wide_u:
        out[:, :A] = torch.rand(B, A, generator=g) * 20 - 10
    u = out[:, :A] + torch.randn(B, A, generator=g) * 0.7
    adv = torch.randn(B, generator=g)
    eps = torch.randn(B, A, generator=g)
    logp64, _ = ref.log_prob(out.double(), u.double())
    logp_old = (logp64 + torch.randn(B, generator=g).double() * 0.4).float()
    return out, u, logp_old, adv, eps


def fused(out, u, logp_old, adv, eps, B):
    partial, loss, grad = Guarded(2 * ((B + 63) // 64)), Guarded(3), Guarded((B + 3) * 2 * A)        # three guard rows behind row B - 1, then the guard floats
    rc = _lib().pgtt_ppo_policy_loss(_ptr(out), _ptr(u), _ptr(logp_old), _ptr(adv), _ptr(eps), C.c_int(B), C.c_int(A), C.c_float(CLIP), C.c_float(COST),
                                     _ptr(partial.view), _ptr(loss.view), _ptr(grad.view), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert partial.guards_intact() and loss.guards_intact() and grad.guards_intact()
    assert bool((grad.view[B * 2 * A:] == SENT).all()), "rows behind B - 1 were written"
    return loss.view.cpu(), grad.view[:B * 2 * A].view(B, 2 * A).cpu()


def op_form(out, u, logp_old, adv, eps):
    """the PyTorch-op fp32 form on the GPU (ppo.ActorCritic.log_prob / entropy, autograd): the reference form of the project"""
    from phase_guided_terrain_traversal_amd import ppo
    o = out.clone().requires_grad_(True)
    loc, raw = torch.chunk(o, 2, dim=-1)
    scale = torch.nn.functional.softplus(raw) + 1e-3
    logp = ppo.ActorCritic.log_prob(loc, scale, u)
    ratio = torch.exp(logp - logp_old)
    pol = -torch.min(ratio * adv, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv).mean()
    ent = ppo.ActorCritic.entropy(loc, scale, loc + scale * eps).mean()
    total = pol - COST * ent
    total.backward()
    torch.cuda.synchronize()
    return torch.stack([total.detach(), pol.detach(), ent.detach()]).cpu(), o.grad.cpu()


def compare(name, loss3, grad, want, B):
    """worst error / tolerance of one form against the fp64 result `want`: (gradient, total, policy term, entropy)"""
    err, edge, g64 = want["err"], want["edge"], want["grad"]
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(loss3).all()), name
    tol_g = (4 * err + 1e-5)[:, None] * g64.abs() + 1e-6 * g64.abs().max()
    rg = ((grad.double() - g64).abs() / tol_g)[~edge]
    r_grad = float(rg.max()) if rg.numel() else 0.0
    tol_pol = float((err * want["surr"].abs()).mean()) + B * ref.U32 * float(want["surr"].abs().mean())
    tol_ent = float(err.mean()) + B * ref.U32 * float(want["ent"].abs().mean())
    r_pol = abs(float(loss3[1]) - want["policy"]) / tol_pol
    r_ent = abs(float(loss3[2]) - want["entropy"]) / tol_ent
    r_tot = abs(float(loss3[0]) - want["total"]) / (tol_pol + COST * tol_ent)
    print(f"  {name:10s} B={B}: error / tolerance  grad {r_grad:.3f}  total {r_tot:.3f}  policy {r_pol:.3f}  entropy {r_ent:.3f}"
          f"   (|policy err| {abs(float(loss3[1]) - want['policy']):.2e}, |entropy err| {abs(float(loss3[2]) - want['entropy']):.2e})")
    return r_grad, r_tot, r_pol, r_ent


@pytest.mark.parametrize("B,wide_u", [(1, False), (63, False), (64, False), (65, False), (4097, False), (5157, False), (5157, True)])
def test_policy_loss_against_fp64(B, wide_u):
    """loss_3 = {total, policy term, mean entropy} and the whole gradient against fp64.  err_i = 8 2^-24 mag_i is the fp32 error of
    logp_i - logp_old_i (mag_i: sum of the sizes of its terms); gradient within (4 err_i + 1e-5) |g64| + 1e-6 max |g64| per element; the loss
    entries within the mean of err_i |surr_i| (err_i for the entropy) plus B 2^-24 relative for the sums.  A sample whose fp64 ratio is within
    4 err_i ratio of a clip boundary may fall on either side: out of the gradient check (not of the finiteness check), at most max(2, 1 %)."""
    out, u, logp_old, adv, eps = loss_inputs(B, wide_u)
    want = ref.policy_loss(out, u, logp_old, adv, eps, CLIP, COST)
    n_edge = int(want["edge"].sum())
    share = float(((want["ratio"] - 1).abs() > CLIP).double().mean())
    print(f"B={B} wide_u={wide_u}: {n_edge} edge samples, clipped share {share:.2f}, max mag {float(want['mag'].max()):.3g}, max err_i {float(want['err'].max()):.2e}")
    assert n_edge <= max(2, B // 100)
    if B >= 63:
        assert 0.2 < share < 0.8
    dev = [t.cuda() for t in (out, u, logp_old, adv, eps)]
    r_op = compare("op form", *op_form(*dev), want, B)
    l1, g1 = fused(*dev, B)
    l2, g2 = fused(*dev, B)
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))      # deterministic
    r_k = compare("kernel", l1, g1, want, B)
    print(f"  worst error / tolerance: op form {max(r_op):.3f}, kernel {max(r_k):.3f}")
    assert max(r_op) <= 1.0, ("the PyTorch-op fp32 form exceeds the error model: the constant LOGP_OPS is too small", r_op)
    assert max(r_k) <= 1.0, r_k


def test_policy_loss_frame():
    """A != 12, B <= 0 and a NULL pointer are refused and nothing is written"""
    B = 65
    dev = [t.cuda() for t in loss_inputs(B)]
    partial, loss, grad = Guarded(2 * ((B + 63) // 64)), Guarded(3), Guarded(B * 2 * A)
    L = _lib()

    def call(ptrs, b, a):
        return L.pgtt_ppo_policy_loss(*ptrs[:5], C.c_int(b), C.c_int(a), C.c_float(CLIP), C.c_float(COST), *ptrs[5:], _stream())

    full = [_ptr(t) for t in dev] + [_ptr(partial.view), _ptr(loss.view), _ptr(grad.view)]
    for b, a in ((B, 11), (B, 13), (B, 0), (B, 24), (0, A), (-1, A)):
        assert call(full, b, a) == E_ARG, (b, a)
    for hole in range(8):
        assert call([None if i == hole else p for i, p in enumerate(full)], B, A) == E_ARG, hole
    torch.cuda.synchronize()
    assert partial.untouched() and loss.untouched() and grad.untouched()
