"""The recurrent PPO update and loop (recurrent_ppo.SequencePPOLearner, Rollout, finetune): one update against the fp64 statement of
tests/recurrent_ppo_reference.py and against the torch-autograd fp32 form of the same update, the bit equalities of the learner (learning rate 0,
graph replay against eager calls, the critic-only update, the truncation at a clear), the acting step and the learner on one roll-out, and
finetune() end to end with its file.

The bars, U = 2^-24, none fitted to the code under test.

  loss_3, from the learner's own fp32 head taken as exact: the bars test_gpu_ppo_kernels.py::compare derives for pgtt_ppo_policy_loss, err_i = 8 U mag_i
      (ppo_reference.logp_error):  policy mean(err |surr|) + B U mean |surr|,  entropy mean(err) + B U mean |ent|,  total = policy + entropy_cost entropy.
  heads against fp64: 1e-4, the bar tests/test_gpu_recurrent_distill.py holds SequenceLearner's head to at these shapes; the total against the full fp64
      update: the bar above plus that head bar through the reference's own gradient, 1e-4 sum |d total / d heads| (first order).
  value loss: the critic's forward is the 2e-5 (1 + max |v64|) of the project's MLP bar (test_gpu_acting_edges.py::check_mlp); 0.25 mean (ret - v)^2 moves by
      0.5 mean |ret - v| per unit of v, plus B U for the sum: 0.5 mean |ret - v64| v_bar + B U value_loss64.
  gradients: relative L2 per tensor against fp64, native / op form <= 4; the norm as test_gpu_recurrent_distill.py holds it.

  Acting and learning on one roll-out.  From the stored rows obs_t, mem0_t, clear_t, u_t the fp64 step gives head64_t and logp64_t.
  (a) the acting kernel read exactly those rows, so its head is within head_bar_t = the propagated bar of test_gpu_recurrent_kernels.py (_act_bars, from the
      observation on), and its logp within  logp_error(mag) + sum_j |d logp / d head_j| head_bar_tj  (first order in the head's error).
  (b) the learner starts from the same m_init and clear flags, but from step 1 on its m0 is its own m1, not the stored one.  With e_t >= |m0_t(learner) -
      mem0_t(stored)|, e_0 = 0:  both m1 are within mem_bar_t of the fp64 m1 of their own m0 (the learner's separate products and sums have no more
      roundings than the acting kernel's single chains: (H + 2) a + (R + 2) b + (a + b) <= (H + R + 3)(a + b)), and the fp64 cell moves by at most
      J_t e_t with J_t = |d m1 / d m0| elementwise, so  e_{t+1} = clear_{t+1} ? 0 : 2 mem_bar_t + J_t e_t  and the learner's head is within
      head_bar_t + |W_m| J_t e_t.  Its log-probability is not an output; what the loss kernel makes of it is: with unchanged parameters the ratio is
      exp(logp_learner - logp_stored) with |logp_learner - logp_stored| <= d_i = bar_a + bar_b (bar_b with the learner's head bar, and the loss kernel's
      own 8 U mag), so loss_3[1] = -mean(min(r a, clip(r) a)) is within mean |a_i| (exp(d_i) - 1) + B U mean |a| of -mean(a).
  The bar propagated from the observation is loose by construction (test_gpu_recurrent_kernels.py says so of itself): through |d logp / d head| it
  reaches hundreds.  So (a) and (b) are held a second time to the sharp bars of that file, which start at h3: the trunk's fp32 output is read back
  (from the acting step's scratch; the learner's has the same bits, which is asserted) and taken as an exact input, h3_bar = 0, the fp64 step is
  evaluated from it, and everything above is repeated with those bars.
"""
import copy
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_reference as pref  # noqa: E402
import recurrent_policy_reference as rref  # noqa: E402
import recurrent_ppo_reference as ref  # noqa: E402
import recurrent_update_cases as cases  # noqa: E402
import test_gpu_recurrent_kernels as rk  # noqa: E402

from phase_guided_terrain_traversal_amd import configs, learn, ppo, recurrent_ppo  # noqa: E402
from phase_guided_terrain_traversal_amd.policy import PolicyMLP, _DIR as POLICY_DIR  # noqa: E402
from phase_guided_terrain_traversal_amd.recurrent_policy import GRU_KEYS, RecurrentActor, RecurrentPolicy  # noqa: E402

DIMS, PD = (171, 512, 256, 128, 24), 215
P177 = os.path.join(POLICY_DIR, "policy177.npz")
NAMES = [f"{k}{i}" for i in range(4) for k in "wb"] + list(GRU_KEYS) + [f"v{k}{i}" for i in range(4) for k in "wb"]
U = 2.0 ** -24
f64 = rref.f64


def _P(pi):
    return {"mean": pi.mean, "std": pi.std, "w": [l.weight for l in pi.layers], "b": [l.bias for l in pi.layers],
            "w_ih": pi.gru_w_ih, "w_hh": pi.gru_w_hh, "b_ih": pi.gru_b_ih, "b_hh": pi.gru_b_hh, "w_m": pi.mem_w}


def _V(value):
    return [(m.weight, m.bias) for m in value if isinstance(m, torch.nn.Linear)]


def _tensors(model):
    """the 21 trained tensors in the order of NAMES (the reference's order)"""
    return model.policy.tensors() + [t for wb in _V(model.value) for t in wb]


def _model(seed, R):
    """torch's default initialisation of every layer and of the cell, a head away from its initial point and a non-zero read-out (as
    test_gpu_recurrent_distill.py), the value net at its default initialisation"""
    torch.manual_seed(seed)
    pi = RecurrentPolicy(DIMS, R)
    cell = torch.nn.GRUCell(DIMS[3], R)
    with torch.no_grad():
        pi.gru_w_ih.copy_(cell.weight_ih); pi.gru_w_hh.copy_(cell.weight_hh); pi.gru_b_ih.copy_(cell.bias_ih); pi.gru_b_hh.copy_(cell.bias_hh)
        pi.mem_w.copy_(torch.randn(24, R) * 0.3)
        pi.layers[3].weight.mul_(3.0); pi.layers[3].bias.add_(torch.randn(24) * 0.3)
    return recurrent_ppo.RecurrentActorCritic(pi, PD).cuda()


def _stores(model, seed, T, N, clears=(), spread=0.4):
    """[T, N, .] rows like a roll-out's: observations with offsets and scales like real ones (their statistics go into the policy), a stored mem0, clear
    flags at `clears`, u sampled from the policy's own fp64 heads, logp_old = their fp64 log-probability moved by `spread` (ratios inside and outside
    1 +- 0.3), advantages of both signs, privileged rows with their statistics, value targets"""
    pi = model.policy
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    obs = (r(171) * 2 + 0.5 + r(T, N, 171) * torch.logspace(-1.3, 0.7, 171, device="cuda")).contiguous()
    with torch.no_grad():
        pi.mean.copy_(obs.view(-1, 171).mean(0)); pi.std.copy_(obs.view(-1, 171).std(0))
    mem0 = (r(T, N, pi.memory) * 0.5).contiguous()
    clear = torch.zeros(T, N, dtype=torch.uint8, device="cuda")
    for t, e in clears:
        clear[t, e] = 1
    heads = rref.sequence(rref.params64(_P(pi)), f64(obs), f64(mem0[0]), clear.cpu().bool())["heads"]
    u64 = heads[..., :12] + (pref.softplus(heads[..., 12:]) + 1e-3) * f64(r(T, N, 12))
    u = u64.float().cuda().contiguous()
    logp, _ = pref.log_prob(heads.reshape(T * N, 24), f64(u).reshape(T * N, 12))
    logp_old = (logp.reshape(T, N) + f64(r(T, N)) * spread).float().cuda().contiguous()
    priv = (r(PD) + r(T, N, PD) * (torch.rand(PD, device="cuda", generator=g) + 0.5)).contiguous()
    mean_p, std_p = priv.view(-1, PD).mean(0).contiguous(), priv.view(-1, PD).std(0).contiguous()
    adv, ret = (r(T, N) * 2 + 0.3).contiguous(), r(T, N).contiguous()
    return {"obs": obs, "u": u, "logp": logp_old, "mem0": mem0, "clear": clear, "priv": priv, "adv": adv, "ret": ret, "mean_p": mean_p, "std_p": std_p}


def _learner(model, S, b_env, lr, use_graph, max_norm=1.0):
    cfg = recurrent_ppo.FinetuneConfig(learning_rate=lr, max_grad_norm=max_norm)
    flat = learn.FlatParams(model)
    return recurrent_ppo.SequencePPOLearner(model, flat, S["obs"], S["u"], S["logp"], S["mem0"], S["clear"], S["priv"], S["adv"], S["ret"], S["mean_p"],
                                            S["std_p"], b_env, cfg, use_graph=use_graph), flat, cfg


def _minibatch(S, envs, eps):
    return {"obs": S["obs"][:, envs], "m_init": S["mem0"][0, envs], "clear": S["clear"][:, envs], "u": S["u"][:, envs], "logp_old": S["logp"][:, envs],
            "adv": S["adv"][:, envs], "eps": eps, "priv": S["priv"][:, envs], "ret": S["ret"][:, envs], "mean_p": S["mean_p"], "std_p": S["std_p"]}


def _op_form(op, mb, cfg):
    """the torch-autograd fp32 form of the same update on the GPU -> the gradients of the 21 tensors"""
    T, B = mb["obs"].shape[:2]
    head = op.policy.sequence(mb["obs"], mb["m_init"], mb["clear"]).reshape(T * B, 24)
    loc, scale = head[:, :12], torch.nn.functional.softplus(head[:, 12:]) + 1e-3
    logp = ppo.ActorCritic.log_prob(loc, scale, mb["u"].reshape(T * B, 12))
    a = mb["adv"].reshape(-1)
    a = (a - a.mean()) / (a.std(unbiased=False) + 1e-8)
    ratio = torch.exp(logp - mb["logp_old"].reshape(-1))
    pol = -torch.min(ratio * a, torch.clamp(ratio, 1 - cfg.clipping_epsilon, 1 + cfg.clipping_epsilon) * a).mean()
    ent = ppo.ActorCritic.entropy(loc, scale, loc + scale * mb["eps"]).mean()
    v = op.value((mb["priv"].reshape(T * B, PD) - mb["mean_p"]) / mb["std_p"]).squeeze(-1)
    total = pol - cfg.entropy_cost * ent + 0.25 * ((mb["ret"].reshape(-1) - v) ** 2).mean()
    return torch.autograd.grad(total, _tensors(op))


def _seeded_eps(seed, rows):
    """the eps the learner's next eager update draws after torch.manual_seed(seed)"""
    torch.manual_seed(seed)
    eps = torch.randn(rows, 12, dtype=torch.float32, device="cuda")
    torch.manual_seed(seed)
    return eps


@pytest.mark.parametrize("case", cases.IDS)
def test_update_losses_and_gradients_against_fp64_and_the_op_form(case, monkeypatch):
    """one update at each shape of recurrent_update_cases.py ("small" is T = 3, 5 envs, R = 16; "shipped" is 51 envs x 20 steps at R = 64 with the
    split-K factors of a real run).  In "one_step" m0 is zero everywhere: W_hh's gradient is exactly 0 in fp64 and on the device, and that one tensor
    has no relative error to compare.

    As first written this test failed at [wide] on vb3 (the value head's bias gradient, a single fp32 number, 260 terms of both signs with a
    condition number of 58): op form 1.45e-07, native 7.87e-07, native / op 5.43.  The rows were as close to fp64 as the op form's; the fp32 chain
    that pgtt_ppo_linear_backward summed them in was not.  Its column sums are carried in fp64 now: vb3 at [wide] 1.88e-07, 1.30, and
    the 125 (case, tensor) ratios are 0.22 to 2.17."""
    monkeypatch.delenv("PGTT_PPO_SPLITK", raising=False)
    T, N, B, R, env_list, clears = cases.minibatch(case)
    model = _model(31, R)
    envs = torch.tensor(env_list, device="cuda")
    S = _stores(model, 31, T, N, clears=clears)
    op = copy.deepcopy(model)
    before = [p.detach().clone() for p in model.parameters()]
    learner, flat, cfg = _learner(model, S, B, lr=0.0, use_graph=False)
    cases.check_split_k(case, learner.S)
    eps = _seeded_eps(5, T * B)
    loss3 = learner.update(envs).clone()
    torch.cuda.synchronize()
    vloss = float(learner.vloss)
    mb = _minibatch(S, envs, eps)
    assert int(mb["clear"].sum()) == cases.clears_inside(env_list, clears) and int(S["clear"].sum()) == len(set(clears))
    if case == "small":
        assert int(mb["clear"].sum()) == 2 and int(mb["clear"][1].sum()) == 2
    if case in ("shipped", "wide"):
        assert int(mb["clear"][0].sum()) == 2 and int(mb["clear"][T - 1].sum()) == 2 and int(mb["clear"].all(0).sum()) == 1
    if case in ("one_step", "cut"):
        assert bool(mb["clear"][T - 1].all()) and int(mb["clear"].sum()) == B
    assert T * B >= 15                                                              # every case is large enough to meet all three kinds of ratio
    want = ref.update(_P(op.policy), _V(op.value), mb, cfg.clipping_epsilon, cfg.entropy_cost, cfg.max_grad_norm)
    r = want["ratio"]
    assert bool((r < 0.7).any()) and bool((r > 1.3).any()) and bool(((r > 0.7) & (r < 1.3)).any()) and bool((mb["adv"] > 0).any()) and bool((mb["adv"] < 0).any())
    # the three numbers of loss_3 from the learner's own head
    a_norm = pref.normalise_advantage(f64(mb["adv"]).reshape(-1))
    assert float((f64(learner.adv) - a_norm).abs().max()) <= 16 * U * float(a_norm.abs().max()) + 1e-6
    own = pref.policy_loss(learner.head, learner.y, learner.logp_old, learner.adv, eps, cfg.clipping_epsilon, cfg.entropy_cost)
    TB = T * B
    tol_pol = float((own["err"] * own["surr"].abs()).mean()) + TB * U * float(own["surr"].abs().mean())
    tol_ent = float(own["err"].mean()) + TB * U * float(own["ent"].abs().mean())
    print(f"recurrent PPO update: loss_3 {loss3.tolist()} from its own head {own['total']:.7f} {own['policy']:.7f} {own['entropy']:.7f}; fp64 {want['loss_3']}")
    print(f"  error / bar: total {abs(float(loss3[0]) - own['total']) / (tol_pol + cfg.entropy_cost * tol_ent):.3f}  policy {abs(float(loss3[1]) - own['policy']) / tol_pol:.3f}"
          f"  entropy {abs(float(loss3[2]) - own['entropy']) / tol_ent:.3f}")
    assert abs(float(loss3[1]) - own["policy"]) <= tol_pol and abs(float(loss3[2]) - own["entropy"]) <= tol_ent
    assert abs(float(loss3[0]) - own["total"]) <= tol_pol + cfg.entropy_cost * tol_ent
    # the heads, and the total against the full fp64 update
    head_err = float((f64(learner.head) - want["heads"]).abs().max())
    tol_full = tol_pol + cfg.entropy_cost * tol_ent + 1e-4 * float(want["dhead"].abs().sum())
    print(f"  heads: max error {head_err:.2e} (bar 1e-4); total against the fp64 update: error {abs(float(loss3[0]) - want['loss_3'][0]):.2e} bar {tol_full:.2e}")
    assert head_err <= 1e-4 and abs(float(loss3[0]) - want["loss_3"][0]) <= tol_full
    # the value loss
    v64 = pref.silu_mlp((f64(mb["priv"]).reshape(TB, PD) - f64(mb["mean_p"])) / f64(mb["std_p"]), [(f64(w), f64(b)) for w, b in _V(op.value)]).squeeze(-1)
    v_bar = 2e-5 * (1 + float(v64.abs().max()))
    tol_v = 0.5 * float((f64(mb["ret"]).reshape(-1) - v64).abs().mean()) * v_bar + TB * U * want["value_loss"]
    print(f"  value loss {vloss:.7f} fp64 {want['value_loss']:.7f}: error / bar {abs(vloss - want['value_loss']) / tol_v:.3f}")
    assert abs(vloss - want["value_loss"]) <= tol_v
    # the unclipped norm
    own_norm = float(f64(flat.grad).norm())
    assert abs(float(learner.norm) - own_norm) <= (flat.numel / 64 + 70) * U * own_norm and abs(own_norm - want["grad_norm"]) <= 1e-4 * own_norm
    # every tensor's gradient
    op_grads = _op_form(op, mb, cfg)
    bad = []
    print(f"recurrent PPO update [{case}], {T} steps x {B} envs, R = {R}, S = {learner.S}: gradient error against fp64, relative L2")
    for name, p, g64, gop in zip(NAMES, _tensors(model), want["grads"], op_grads):
        if case == "one_step" and name == "gru_w_hh":                              # m0 = 0 in every row: exactly zero on both sides, no ratio
            assert bool((g64 == 0).all()) and bool((flat.grad_of(p) == 0).all())
            print(f"  {name:9s}: exactly 0 in fp64 and on the device")
            continue
        e_na = float((f64(flat.grad_of(p)) - g64).norm() / g64.norm())
        e_op = float((f64(gop) - g64).norm() / g64.norm())
        print(f"  {name:9s}: op form {e_op:.2e}   native {e_na:.2e}   native / op {e_na / max(e_op, 1e-300):.2f}")
        if e_na > 4 * e_op:
            bad.append((name, e_op, e_na))
    assert not bad, bad
    for a, p in zip(before, model.parameters()):                                    # learning_rate 0: the parameters keep their bits
        assert torch.equal(a, p)


def test_a_clear_truncates_the_sequence():
    """changing m_init of an env cleared at t = 1 changes that env's heads at t = 0 only: rows t >= 1 are bit for bit equal"""
    T, N, B, R = 3, 6, 6, 16
    model = _model(32, R)
    S = _stores(model, 32, T, N, clears=[(1, 2)])
    learner, flat, _ = _learner(model, S, B, lr=0.0, use_graph=False)
    before = flat.flat.clone()
    learner.update(torch.arange(N, device="cuda"))
    h0 = learner.head.clone().view(T, B, 24)
    learner.m_init[2] += 1.0
    learner.m_init[4] += 1.0
    learner.update(None)                                                            # the fixed buffers as they stand
    h1 = learner.head.view(T, B, 24)
    torch.cuda.synchronize()
    assert not torch.equal(h0[0, 2], h1[0, 2]) and torch.equal(h0[1:, 2], h1[1:, 2])
    assert not torch.equal(h0[0, 4], h1[0, 4]) and not torch.equal(h0[2, 4], h1[2, 4])         # an env that is not cleared carries the change on
    assert torch.equal(h0[:, [0, 1, 3, 5]], h1[:, [0, 1, 3, 5]])
    assert torch.equal(flat.flat, before) and flat.t.tolist() == [2]


def test_graph_replay_gives_the_bits_of_eager_calls():
    """two learners from equal state, one captured at its third call, one eager throughout, the generator seeded alike before every call: after each of
    five updates on changing minibatches, the inputs changed in place before the fifth, the losses, the gradient, the norm and the parameters have
    equal bits"""
    T, N, B, R = 4, 18, 6, 16
    runs = []
    for use_graph in (True, False):
        model = _model(33, R)
        S = _stores(model, 33, T, N, clears=[(0, 1), (2, 5), (1, 12), (3, 17)])
        learner, flat, _ = _learner(model, S, B, lr=1e-3, use_graph=use_graph)
        perm = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
        rec = []
        for k in range(5):
            if k == 4:
                with torch.no_grad():                                               # the graph reads its inputs in place
                    S["u"].mul_(0.9); S["obs"].add_(0.01); S["mem0"].mul_(0.5); S["clear"][1, :] = 1; S["priv"].add_(0.02); S["ret"].mul_(1.1)
            torch.manual_seed(100 + k)
            l3 = learner.update(perm[(k % 3) * B:(k % 3 + 1) * B]).clone()
            torch.cuda.synchronize()
            rec.append((l3, learner.vloss.clone(), flat.grad.clone(), flat.flat.clone(), learner.norm.clone()))
        assert (learner.graph is not None) == use_graph and flat.t.tolist() == [5]
        runs.append(rec)
    for k, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
    assert not torch.equal(runs[0][0][3], runs[0][4][3]) and all(bool(torch.isfinite(x).all()) for rec in runs[0] for x in rec)


def test_the_critic_only_update_leaves_the_policy_its_bits():
    T, N, B, R = 3, 10, 5, 16
    model = _model(34, R)
    S = _stores(model, 34, T, N, clears=[(1, 3)])
    learner, flat, _ = _learner(model, S, B, lr=1e-3, use_graph=True)
    P = learner.policy_numel
    pol0, val0 = flat.flat[:P].clone(), flat.flat[P:].clone()
    envs = torch.arange(N, device="cuda")
    for k in range(4):                                                              # two eager calls, the capture, a replay
        learner.update(envs[(k % 2) * B:(k % 2 + 1) * B], policy=False)
    torch.cuda.synchronize()
    assert learner.graph_critic is not None and learner.graph is None and flat.t.tolist() == [4]
    assert torch.equal(flat.flat[:P], pol0) and not torch.equal(flat.flat[P:], val0) and bool((flat.grad[:P] == 0).all())
    v1 = float(learner.vloss)
    learner.update(envs[:B], policy=True)
    torch.cuda.synchronize()
    assert not torch.equal(flat.flat[:P], pol0) and bool((flat.grad[:P] != 0).any())
    learner.update(envs[:B], policy=False)                                          # back to the warm-up: the policy's gradient segment is zeroed
    torch.cuda.synchronize()
    assert bool((flat.grad[:P] == 0).all()) and bool((flat.grad[P:] != 0).any()) and np.isfinite(v1) and np.isfinite(float(learner.vloss))


# ------------------------------------------------------------------ acting and learning on one roll-out
T_ROLL, N_ROLL, R_ROLL = 4, 32, 16
SEED = 0x9E3779B97F4A7C15


def _env():
    from phase_guided_terrain_traversal_amd.env import Joystick
    env = Joystick("flat_terrain", configs.training_config(), num_envs=N_ROLL, device="cuda:0", autoreset=True)
    env.reset(seed=1)
    return env


def _student(seed=1):
    pi = RecurrentPolicy.from_teacher(PolicyMLP(P177), R_ROLL, seed=seed)
    with torch.no_grad():
        pi.mem_w.copy_(torch.randn(24, R_ROLL, generator=torch.Generator().manual_seed(seed)) * 0.2)
    return pi


def _abs_jacobian_m1_m0(P64, h3, m0):
    """|d m1 / d m0| of the fp64 cell, [N, R (m1), R (m0)]"""
    m0 = m0.clone().requires_grad_(True)
    gi, gh = h3 @ P64["w_ih"].T + P64["b_ih"], m0 @ P64["w_hh"].T + P64["b_hh"]
    m1 = rref.cell(gi, gh, m0)[3]
    rows = [torch.autograd.grad(m1[:, k].sum(), m0, retain_graph=True)[0] for k in range(m0.shape[1])]
    return torch.stack(rows, 1).abs()


def test_acting_and_learning_agree_on_one_rollout():
    from phase_guided_terrain_traversal_amd import abi
    env = _env()
    cfg = recurrent_ppo.FinetuneConfig(unroll_length=T_ROLL, num_minibatches=1, learning_rate=0.0)
    pi_cpu = _student()
    model = recurrent_ppo.RecurrentActorCritic(copy.deepcopy(pi_cpu), PD).cuda()
    pi_cpu.requires_grad_(False)                                                    # the CPU copy is the fp64 reference's input only
    flat = learn.FlatParams(model)
    actor = RecurrentActor(env, T_ROLL, R_ROLL, seed=SEED)
    actor.load(model.policy)
    actor.reset_memory()
    roll = recurrent_ppo.Rollout(env, actor, cfg)
    S = actor.storage
    L = int(env.config["episode_length"])
    seen = {"rew": [], "done": [], "trunc": [], "h3": []}
    lo = N_ROLL * (171 + 512 + 256)
    actor.counters[0].zero_()
    for t in range(T_ROLL):
        roll.step(t)
        torch.cuda.synchronize()
        seen["h3"].append(actor.work[lo:lo + N_ROLL * 128].view(N_ROLL, 128).clone())       # the trunk's output as the acting step left it in its scratch
        seen["rew"].append(env.buffers["reward"].clone() * float(cfg.reward_scaling)); seen["done"].append(env.buffers["done"].clone())
        fallen = env.buffers["frame"][abi.F_UPVECTOR + 2] < 0
        seen["trunc"].append(((env.buffers["istate"][abi.I_EP_STEPS] >= L) & ~fallen).float())
    assert actor.counters.tolist() == [T_ROLL, T_ROLL]                               # the record advanced the row and the draw counter by T
    for k in ("rew", "done", "trunc"):
        assert torch.equal(S[k], torch.stack(seen[k])), k                           # the env's rows, bit for bit
    assert bool((S["clear"][0] == 1).all()) and bool((S["mem0"][0] == 0).all())
    # the learner's first forward, parameters unchanged (learning rate 0)
    adv, ret = torch.randn(T_ROLL, N_ROLL, device="cuda"), torch.zeros(T_ROLL, N_ROLL, device="cuda")
    learner = recurrent_ppo.SequencePPOLearner(model, flat, S["obs"], S["u"], S["logp"], S["mem0"], S["clear"], S["priv"], adv, ret,
                                               torch.zeros(PD, device="cuda"), torch.ones(PD, device="cuda"), N_ROLL, cfg, use_graph=False)
    loss3 = learner.update(torch.arange(N_ROLL, device="cuda")).clone()
    torch.cuda.synchronize()
    head = f64(learner.head).view(T_ROLL, N_ROLL, 24)
    # the same trunk kernel on the same normalised rows: the learner's h3 has the acting step's bits, so one h3 serves both as the exact input of the sharp bars
    assert torch.equal(learner.h[2].view(T_ROLL, N_ROLL, 128), torch.stack(seen["h3"]))
    P64 = rref.params64(_P(pi_cpu))
    Wm_abs = P64["w_m"].abs()
    a_norm = f64(learner.adv)
    for kind in ("from the observation", "from the kernels' h3"):
        e = torch.zeros(N_ROLL, R_ROLL, dtype=torch.float64)
        ds = []
        for t in range(T_ROLL):
            obs, mem0, clear, u = S["obs"][t].cpu(), S["mem0"][t].cpu(), S["clear"][t].cpu().bool(), f64(S["u"][t])
            h3 = None if kind == "from the observation" else seen["h3"][t].cpu()
            step, bars = rk._act_bars(pi_cpu, obs, mem0, clear, h3=h3)              # fp64 from the stored rows (and, sharp, from h3 as exact) and its bars
            h64 = step["head"].clone().requires_grad_(True)
            lp, mag = pref.log_prob(h64, u)
            dl = torch.autograd.grad(lp.sum(), h64)[0].abs()                        # |d logp / d head|
            lp = lp.detach()
            if h3 is None:                                                          # the reference module states the same step
                assert float((ref.stored_logp(_P(pi_cpu), obs, mem0, clear, u)[0] - lp).abs().max()) <= 1e-12
            # (a) the acting step's stored logp
            bar_a = pref.logp_error(mag) + (dl * bars["head"]).sum(-1)
            err_a = (f64(S["logp"][t]) - lp).abs()
            # (b) the learner's head: the memory it carries is its own
            J = _abs_jacobian_m1_m0(P64, step["h3"] if h3 is None else f64(h3), step["m0"])
            drift = torch.einsum("nij,nj->ni", J, e)                                # J_t e_t
            bar_head = (dl * (bars["head"] + drift @ Wm_abs.T)).sum(-1)
            err_b = (pref.log_prob(head[t], u)[0] - lp).abs()
            print(f"row {t}, bars {kind}: stored logp error / bar {float((err_a / bar_a).max()):.3e} (worst bar {float(bar_a.max()):.2e});  the learner's logp "
                  f"(fp64 of its fp32 head) error / bar {float((err_b / bar_head).max()):.3e} (worst bar {float(bar_head.max()):.2e})")
            assert bool((err_a <= bar_a).all()) and bool((err_b <= bar_head).all()), (kind, t)
            if t + 1 < T_ROLL:
                e = torch.where(S["clear"][t + 1].cpu().bool()[:, None], torch.zeros((), dtype=torch.float64), 2 * bars["mem"] + drift)
            ds.append(bar_a + bar_head + pref.logp_error(mag))                      # + the loss kernel's own fp32 evaluation of logp
        # what the loss kernel makes of the learner's log-probabilities: every ratio within exp(+-d) of 1
        d = torch.cat(ds)
        tol = float((a_norm.abs() * torch.expm1(d)).mean()) + T_ROLL * N_ROLL * U * float(a_norm.abs().mean())
        got = float(loss3[1]) + float(a_norm.mean())
        print(f"unchanged parameters, bars {kind}: -mean(surr) + mean(a) = {got:.3e}, bar {tol:.3e}")
        assert abs(got) <= tol
    env.close()


def test_finetune_end_to_end(tmp_path):
    env = _env()
    pi = _student(seed=2)
    start = [t.detach().clone() for t in pi.tensors()]
    mean0, std0 = pi.mean.clone(), pi.std.clone()
    snaps = []
    cfg = recurrent_ppo.FinetuneConfig(iterations=2, unroll_length=T_ROLL, num_minibatches=2, num_updates_per_batch=1, critic_warmup_iters=1, seed=3)

    def progress(it, m):
        snaps.append(([t.detach().cpu().clone() for t in pi.tensors()], m))
        return False
    out = recurrent_ppo.finetune(env, pi, cfg, obs=env.buffers["obs_state"], progress_fn=progress)
    torch.cuda.synchronize()
    assert len(out.history) == 2 and [m["policy_updates"] for m in out.history] == [0.0, 1.0] and all(m["updates"] == 2 for m in out.history)
    for m in out.history:
        assert all(np.isfinite(v) for v in m.values()), m
    assert all(torch.equal(a, b) for a, b in zip(snaps[0][0], start))               # iteration 1 is a critic warm-up: the policy keeps its bits
    assert all(not torch.equal(a, b) for a, b in zip(snaps[1][0], start))           # iteration 2 moves every tensor
    assert torch.equal(out.policy.mean.cpu(), mean0) and torch.equal(out.policy.std.cpu(), std0)      # the normalisation is frozen
    path = str(tmp_path / "finetuned.npz")
    out.save(path)
    back = RecurrentPolicy.load(path)
    assert back.memory == R_ROLL and all(torch.equal(a, b.detach().cpu()) for a, b in zip(back.tensors(), out.policy.tensors()))
    with pytest.raises(recurrent_ppo.FinetuneError, match="does not divide"):
        recurrent_ppo.finetune(env, _student(), recurrent_ppo.FinetuneConfig(num_minibatches=5), obs=env.buffers["obs_state"])
    env.close()
