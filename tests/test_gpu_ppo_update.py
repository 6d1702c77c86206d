"""The captured PPO minibatch update as a whole (ppo._Learner.update: two MLPs forward / backward on two streams, the fused policy loss, the
split-K weight gradients, clip, fused Adam, one HIP graph after two eager calls) against the fp64 statement of the update in
tests/ppo_reference.py, on a synthetic batch (no env); fresh entropy draws on every replay; and the on-policy invariant across the
_Actor / _Learner seam on a 1024-env Joystick."""
import itertools
import math

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ppo_reference as ref

LOSS_TOL = 2e-5        # the loss is a mean of per-sample terms that each carry ~1e-6 of fp32 forward error; a mean does not amplify it (test_ppo_reference.py)


def _layers(seq):
    return [(m.weight.detach().clone(), m.bias.detach().clone()) for m in seq if isinstance(m, torch.nn.Linear)]


def _stats(nm):
    return nm.mean.clone(), nm.m2.clone(), float(nm.count)


def _observations(n, g):
    """rows with offsets and scales like real observations: per-column means of a few units, scales from 0.05 to 5"""
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    obs = r(171) * 2 + 0.5 + r(n, 171) * torch.logspace(-1.3, 0.7, 171, device="cuda")
    priv = r(215) * 2 - 0.3 + r(n, 215) * torch.logspace(-1.3, 0.7, 215, device="cuda")
    return obs, priv


def _setup(mb, clip_active, entropy_cost, lr, use_graph):
    """model, normalisers (updated once), a synthetic batch of 4 mb rows, Adam as ppo.train creates it, the learner"""
    from phase_guided_terrain_traversal_amd import ppo
    torch.manual_seed(mb)
    g = torch.Generator(device="cuda").manual_seed(mb + 1)
    model = ppo.ActorCritic().cuda()
    with torch.no_grad():                       # a policy head away from its initial point
        model.policy[-1].weight.mul_(3.0); model.policy[-1].bias.add_(torch.randn(24, device="cuda", generator=g) * 0.3)
    n = 4 * mb
    obs, priv = _observations(n, g)
    norm_s, norm_p = ppo.RunningNorm(171, "cuda"), ppo.RunningNorm(215, "cuda")
    norm_s.update(obs); norm_p.update(priv)
    u = torch.randn(n, 12, device="cuda", generator=g) * 0.8
    st = _stats(norm_s)
    out64 = ref.silu_mlp(ref.normalise(ref.f64(obs), ref.f64(st[0]), ref.f64(st[1]), st[2]), [(ref.f64(w), ref.f64(b)) for w, b in _layers(model.policy)])
    logp64, _ = ref.log_prob(out64, ref.f64(u))
    logp = (logp64 + torch.randn(n, dtype=torch.float64) * 0.3).float().cuda()
    B = {"obs": obs, "priv": priv, "u": u, "logp": logp, "adv": 0.3 + torch.randn(n, device="cuda", generator=g) * 2,
         "ret": torch.randn(n, device="cuda", generator=g) * (60.0 if clip_active else 1.0) + (40.0 if clip_active else 0.0)}      # large targets with a mean: gradient norm >> 1
    cfg = ppo.PPOConfig(max_grad_norm=1.0 if clip_active else 100.0, entropy_cost=entropy_cost, learning_rate=lr)
    opt = torch.optim.Adam(model.parameters(), lr=cfg.learning_rate, capturable=use_graph, fused=True)
    learner = ppo._Learner(model, opt, norm_s, norm_p, B, mb, cfg, use_graph=use_graph)
    return model, norm_s, norm_p, B, cfg, learner, g


def _run_six(mb, clip_active, product, monkeypatch):
    """six updates (product path: 1, 2 eager, 3 captures, 4-6 replay); between the replays the test changes what the graph reads through
    pointers.  Returns per call the errors of the loss and of every clipped gradient tensor against fp64, after asserting Adam."""
    if product:
        for k in ("PGTT_PPO_FUSED", "PGTT_PPO_STREAMS", "PGTT_PPO_LINEAR", "PGTT_PPO_SPLITK", "PGTT_PPO_FORCE_DP"):
            monkeypatch.delenv(k, raising=False)
    else:                                       # the PyTorch-op trainer: the reference form of the project
        monkeypatch.setenv("PGTT_PPO_FUSED", "0"); monkeypatch.setenv("PGTT_PPO_STREAMS", "1")
    model, norm_s, norm_p, B, cfg, learner, g = _setup(mb, clip_active, 0.0, 3e-4, use_graph=product)
    assert (learner.side is not None) == product
    params = list(model.parameters())
    assert len(params) == 16
    adam = ref.Adam(params, cfg.learning_rate)
    perm = torch.randperm(4 * mb, device="cuda", generator=g)
    rows, coefs = [], []
    for k in range(1, 7):
        with torch.no_grad():
            if k == 4:                          # new advantages and value targets in place (what ppo.train does every iteration)
                B["adv"].copy_(torch.randn(4 * mb, device="cuda", generator=g) * 3 - 1.0)
                B["ret"].copy_(B["ret"] * 0.5 + torch.randn(4 * mb, device="cuda", generator=g))
            if k == 5:                          # the running statistics move
                o2, p2 = _observations(2 * mb, g)
                norm_s.update(o2 * 1.5 + 0.7); norm_p.update(p2 * 0.6 - 0.4)
            if k == 6:                          # one weight tensor set in place
                w = model.policy[2].weight
                w.copy_(w * 1.25 + torch.randn(w.shape, device="cuda", generator=g) * 0.01)
                adam.p[2].copy_(ref.f64(w))
        idx = perm[(k % 4) * mb:(k % 4 + 1) * mb] if k < 5 else perm.flip(0)[(k % 4) * mb:(k % 4 + 1) * mb]
        before = _layers(model.policy), _layers(model.value), _stats(norm_s), _stats(norm_p)
        mbatch = {key: B[key][idx].clone() for key in B}
        loss = float(learner.update(idx))
        torch.cuda.synchronize()
        assert (learner.graph is not None) == (product and k >= 3), (k, learner.graph, learner.use_graph)
        grads = [p.grad.detach().clone() for p in params]
        want = ref.update(before[0], before[1], before[2], before[3], mbatch, None, cfg.clipping_epsilon, 0.0, cfg.max_grad_norm)
        coefs.append(want["clip_coef"])
        assert math.isfinite(loss) and abs(loss - want["total"]) <= LOSS_TOL * (1 + abs(want["total"])), (k, loss, want["total"])
        errs = []
        for gq, g64 in zip(grads, want["grads"]):
            d = ref.f64(gq) - g64
            errs.append((float(d.norm() / g64.norm()), float(d.abs().max() / g64.abs().max())))
        rows.append(errs)
        # Adam on the learner's own recorded gradients, in fp64
        p64 = adam.step(grads)
        for i, (p, q) in enumerate(zip(params, p64)):
            tol = k * (2.0 ** -23 * q.abs() + 1e-5 * cfg.learning_rate)
            dp = (ref.f64(p) - q).abs()
            assert bool((dp <= tol).all()), ("adam", k, i, float(dp.max()), float((dp / tol).max()))
    assert all(c < 1.0 for c in coefs) if clip_active else all(c == 1.0 for c in coefs), coefs
    return rows


@pytest.mark.parametrize("mb,clip_active", [(5120, True), (1280, False)])
def test_update_matches_fp64_reference(mb, clip_active, monkeypatch):
    """Loss, the clipped gradient of each of the 16 parameter tensors and the Adam step of six updates against fp64.  The gradient bar is not a
    fixed number: the same errors are measured for the PyTorch-op trainer (PGTT_PPO_FUSED=0, one stream, no graph) on the same GPU, and the
    product path must stay within 4x of it per tensor (worst of the six calls; relative L2 and max-norm) - the two paths sum in different
    orders and carry independent rounding of the same size."""
    op = _run_six(mb, clip_active, False, monkeypatch)
    pr = _run_six(mb, clip_active, True, monkeypatch)
    from phase_guided_terrain_traversal_amd import ppo
    names = [n for n, _ in ppo.ActorCritic().named_parameters()]
    bad = []
    print(f"mb={mb} clip {'active' if clip_active else 'inactive'}: gradient error against fp64, worst of six calls (relative L2 | max-norm)")
    for i, name in enumerate(names):
        e_op = [max(r[i][j] for r in op) for j in (0, 1)]
        e_pr = [max(r[i][j] for r in pr) for j in (0, 1)]
        print(f"  {name:18s} op form {e_op[0]:.2e} | {e_op[1]:.2e}   product {e_pr[0]:.2e} | {e_pr[1]:.2e}   ratio {e_pr[0] / max(e_op[0], 1e-300):.2f} | {e_pr[1] / max(e_op[1], 1e-300):.2f}")
        if e_pr[0] > 4 * e_op[0] or e_pr[1] > 4 * e_op[1]:
            bad.append((name, e_op, e_pr))
    for k in range(6):
        print(f"  call {k + 1}: worst relative L2  op form {max(e[0] for e in op[k]):.2e}  product {max(e[0] for e in pr[k]):.2e}")
    assert not bad, bad


def test_replays_draw_fresh_entropy_noise(monkeypatch):
    """entropy_cost 1e-2, learning rate 0, the same minibatch on four replays: the parameters stand still, so the loss may differ only through
    the draw of eps - the four losses must be pairwise different and each within six standard errors of the fp64 loss whose entropy term is
    the mean of its one-sample estimator (standard error in fp64 from 200 draws of eps on the CPU)"""
    for k in ("PGTT_PPO_FUSED", "PGTT_PPO_STREAMS", "PGTT_PPO_LINEAR", "PGTT_PPO_SPLITK", "PGTT_PPO_FORCE_DP"):
        monkeypatch.delenv(k, raising=False)
    mb = 5120
    model, norm_s, norm_p, B, cfg, learner, g = _setup(mb, False, 1e-2, 0.0, use_graph=True)
    idx = torch.randperm(4 * mb, device="cuda", generator=g)[:mb]
    before = [p.detach().clone() for p in model.parameters()]
    losses = []
    for k in range(1, 8):
        loss = float(learner.update(idx))
        torch.cuda.synchronize()
        if k >= 4:
            assert learner.graph is not None
            losses.append(loss)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    want = ref.update(_layers(model.policy), _layers(model.value), _stats(norm_s), _stats(norm_p), {key: B[key][idx] for key in B}, None,
                      cfg.clipping_epsilon, 0.0, cfg.max_grad_norm)
    g64 = torch.Generator().manual_seed(9)
    ents = torch.stack([ref.entropy(want["out"], torch.randn(mb, 12, dtype=torch.float64, generator=g64)).mean() for _ in range(200)])
    totals = want["total"] - cfg.entropy_cost * ents
    mean, se = float(totals.mean()), float(totals.std())
    print(f"replay losses {losses}; fp64 mean {mean:.6f}, standard error of one draw {se:.2e}, deviations / se {[round((l - mean) / se, 2) for l in losses]}")
    assert all(a != b for a, b in itertools.combinations(losses, 2)), losses
    assert all(abs(l - mean) <= 6 * se for l in losses), (losses, mean, se)


def test_stored_logp_is_the_current_models(monkeypatch):
    """The on-policy invariant across the _Actor / _Learner seam: after the learner has moved the weights and the statistics, the next
    actor.rollout() repacks them (FusedActor.load_sequential), and the log-probability it stores for every (obs, u) is the CURRENT model's -
    ratio = 1 at the first minibatch.  fp64 log-probability under the model and statistics as they stand, within err_i (ppo_reference.logp_error)."""
    for k in ("PGTT_PPO_FUSED", "PGTT_PPO_STREAMS", "PGTT_PPO_LINEAR", "PGTT_PPO_ACT_FUSED", "PGTT_PPO_FORCE_DP"):
        monkeypatch.delenv(k, raising=False)
    from phase_guided_terrain_traversal_amd import abi, configs, ppo
    from phase_guided_terrain_traversal_amd.env import Joystick
    n, T, nmb = 1024, 20, 4
    env = Joystick("flat_terrain", configs.training_config(), num_envs=n, device="cuda:0", autoreset=True)
    cfg = ppo.PPOConfig(seed=3)
    torch.manual_seed(cfg.seed)
    model = ppo.ActorCritic(env.observation_size["state"], env.observation_size["privileged_state"]).cuda()
    norm_s, norm_p = ppo.RunningNorm(env.observation_size["state"], "cuda"), ppo.RunningNorm(env.observation_size["privileged_state"], "cuda")
    opt = torch.optim.Adam(model.parameters(), lr=cfg.learning_rate, capturable=True, fused=True)
    env.reset(seed=cfg.seed)
    ep_sums = torch.zeros(abi.NMETRIC + 3, device="cuda")
    acc = (ep_sums[abi.NMETRIC], ep_sums[abi.NMETRIC + 1], ep_sums[abi.NMETRIC + 2], ep_sums[:abi.NMETRIC])
    learner = None
    initial = [p.detach().clone() for p in model.parameters()]
    with torch.no_grad():
        actor = ppo._Actor(env, model, norm_s, T, cfg, env.config["episode_length"], acc=acc, use_graph=True, ep_sums=ep_sums)
    assert actor.fused is not None and actor.graph is not None
    flat = lambda x: x.reshape(T * n, *x.shape[2:])
    for it in range(2):                         # two iterations of ppo.train's loop body
        with torch.no_grad():
            batch = actor.rollout()
            last_priv = env._obs()["privileged_state"].clone()
            norm_s.update(batch["obs"]); norm_p.update(batch["priv"])
            values = model.value(norm_p(torch.cat([batch["priv"], last_priv[None]], 0))).squeeze(-1)
            adv, ret = ppo.compute_gae(batch["trunc"], batch["done"] * (1.0 - batch["trunc"]), batch["rew"], values[:-1], values[-1], cfg.gae_lambda, cfg.discounting)
        if learner is None:
            B = {k: flat(batch[k]) for k in ("obs", "priv", "u", "logp")}
            B["adv"], B["ret"] = torch.zeros(T * n, device="cuda"), torch.zeros(T * n, device="cuda")
            learner = ppo._Learner(model, opt, norm_s, norm_p, B, T * n // nmb, cfg, use_graph=True)
        learner.B["adv"].copy_(flat(adv)); learner.B["ret"].copy_(flat(ret))
        perm = torch.randperm(T * n, device="cuda")
        for k in range(nmb):
            learner.update(perm[k * (T * n // nmb):(k + 1) * (T * n // nmb)])
    assert learner.graph is not None
    before = [p.detach().clone() for p in model.parameters()]
    with torch.no_grad():
        S = actor.rollout()                     # no normaliser update in between
    torch.cuda.synchronize()
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    obs, u, logp = ref.f64(flat(S["obs"])), ref.f64(flat(S["u"])), ref.f64(flat(S["logp"]))
    st = _stats(norm_s)
    out64 = ref.silu_mlp(ref.normalise(obs, ref.f64(st[0]), ref.f64(st[1]), st[2]), [(ref.f64(w), ref.f64(b)) for w, b in _layers(model.policy)])
    logp64, mag = ref.log_prob(out64, u)
    err = ref.logp_error(mag + logp.abs())
    ratio = ((logp - logp64).abs() / err)
    print(f"on-policy: {T * n} rows, worst |logp - logp64| {float((logp - logp64).abs().max()):.2e}, worst error / err_i {float(ratio.max()):.3f}, "
          f"the learner moved the weights by up to {max(float((a - b).abs().max()) for a, b in zip(before, initial)):.2e}")
    assert all(float((a - b).abs().max()) > 0 for a, b in zip(before, initial)), "the learner did not move every tensor: the repack would not be exercised"
    assert bool(torch.isfinite(logp).all()) and float(u.abs().max()) > 0
    assert bool((ratio <= 1.0).all()), (int((ratio > 1).sum()), float(ratio.max()))
    env.close()
