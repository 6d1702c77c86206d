"""The recurrent policy's update and loop (recurrent_policy.SequenceLearner, distill.py with memory > 0, evaluate.py): one BPTT update against the
fp64 statement (tests/recurrent_policy_reference.py) and against the torch-autograd fp32 form of the same update, the truncation at a clear, graph
replay against eager calls, a task only a memory can solve next to the feed-forward learner, the roll-out's rows bit for bit, distill() end to end
with its file, and the evaluator on both kinds of file."""
import copy
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recurrent_policy_reference as rref  # noqa: E402
import recurrent_update_cases as cases  # noqa: E402

from phase_guided_terrain_traversal_amd import configs, distill, learn  # noqa: E402
from phase_guided_terrain_traversal_amd.policy import PolicyMLP, _DIR as POLICY_DIR  # noqa: E402
from phase_guided_terrain_traversal_amd.recurrent_policy import GRU_KEYS, RecurrentPolicy, SequenceLearner  # noqa: E402

DIMS = (171, 512, 256, 128, 24)
LEVEL1 = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level1.npy")
P177 = os.path.join(POLICY_DIR, "policy177.npz")
NAMES = [f"{k}{i}" for i in range(4) for k in "wb"] + list(GRU_KEYS)


def _P(pi):
    return {"mean": pi.mean, "std": pi.std, "w": [l.weight for l in pi.layers], "b": [l.bias for l in pi.layers],
            "w_ih": pi.gru_w_ih, "w_hh": pi.gru_w_hh, "b_ih": pi.gru_b_ih, "b_hh": pi.gru_b_hh, "w_m": pi.mem_w}


def _policy(seed, R):
    """torch's default initialisation of every layer and of the cell, a head away from its initial point (as test_gpu_distill.py), a non-zero read-out"""
    torch.manual_seed(seed)
    pi = RecurrentPolicy(DIMS, R)
    cell = torch.nn.GRUCell(DIMS[3], R)
    with torch.no_grad():
        pi.gru_w_ih.copy_(cell.weight_ih); pi.gru_w_hh.copy_(cell.weight_hh); pi.gru_b_ih.copy_(cell.bias_ih); pi.gru_b_hh.copy_(cell.bias_hh)
        pi.mem_w.copy_(torch.randn(24, R) * 0.3)
        pi.layers[3].weight.mul_(3.0); pi.layers[3].bias.add_(torch.randn(24) * 0.3)
    return pi.cuda()


def _stores(pi, seed, T, N, noise=(0.1, 0.1), clears=()):
    """[T, N, .] rows like a roll-out's: observations with offsets and scales like real ones (their statistics go into the policy), a stored mem0
    (row 0 is the unrolls' m_init), clear flags at `clears` = [(t, e)], labels = the policy's own fp64 heads moved by noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    obs = (r(171) * 2 + 0.5 + r(T, N, 171) * torch.logspace(-1.3, 0.7, 171, device="cuda")).contiguous()
    with torch.no_grad():
        pi.mean.copy_(obs.view(-1, 171).mean(0)); pi.std.copy_(obs.view(-1, 171).std(0))
    mem0 = (r(T, N, pi.memory) * 0.5).contiguous()
    clear = torch.zeros(T, N, dtype=torch.uint8, device="cuda")
    for t, e in clears:
        clear[t, e] = 1
    heads = rref.sequence(rref.params64(_P(pi)), rref.f64(obs), rref.f64(mem0[0]), clear.cpu().bool())["heads"]
    labels = heads.float().cuda()
    labels[..., :12] += r(T, N, 12) * noise[0]
    labels[..., 12:] += r(T, N, 12) * noise[1]
    return obs, labels.contiguous(), mem0, clear


def _learner(pi, stores, b_env, lr, use_graph, max_norm=1.0):
    cfg = distill.DistillConfig(learning_rate=lr, max_grad_norm=max_norm, memory=pi.memory)
    flat = learn.FlatParams(pi)
    return SequenceLearner(pi, flat, *stores, b_env, cfg, use_graph=use_graph), flat


def _kl_torch(head, labels):
    ls, rs, lt, rt = head[:, :12], head[:, 12:], labels[:, :12], labels[:, 12:]
    ss, st = torch.nn.functional.softplus(rs) + 1e-3, torch.nn.functional.softplus(rt) + 1e-3
    d = lt - ls
    return (torch.log(ss / st) + 0.5 * ((st * st + d * d) / (ss * ss) - 1.0)).sum(-1).mean()


@pytest.mark.parametrize("case", cases.IDS)
def test_update_gradients_against_fp64_and_the_op_form(case, monkeypatch):
    """one update at each shape of recurrent_update_cases.py (the full trunk; "small" is T = 3 steps of 5 envs, R = 16, a clear at t = 1 in two of
    them; "shipped" is 51 envs x 20 steps at R = 64, where the split-K factors are those of a real run): the loss within 2e-5 of fp64, every tensor's
    gradient in relative L2 against fp64 next to the torch-autograd fp32 form of the same update; the native error is at most 4 times the op form's
    per tensor (the margin of DESIGN.md 17 and 23).  In "one_step" m0 is zero everywhere: W_hh's gradient is exactly 0 in fp64 and on the device, and
    that one tensor has no relative error to compare."""
    monkeypatch.delenv("PGTT_PPO_SPLITK", raising=False)
    T, N, B, R, env_list, clears = cases.minibatch(case)
    pi = _policy(21, R)
    envs = torch.tensor(env_list, device="cuda")
    stores = _stores(pi, 21, T, N, clears=clears)
    obs, labels, mem0, clear = stores
    op = copy.deepcopy(pi)
    before = [p.detach().clone() for p in pi.tensors()]
    learner, flat = _learner(pi, stores, B, lr=0.0, use_graph=False)
    cases.check_split_k(case, learner.S)
    loss2 = learner.update(envs).clone()
    torch.cuda.synchronize()
    ob, lb, mb, cb = obs[:, envs], labels[:, envs], mem0[0, envs], clear[:, envs]
    assert int(cb.sum()) == cases.clears_inside(env_list, clears) and int(clear.sum()) == len(set(clears))
    if case == "small":
        assert int(cb.sum()) == 2 and int(cb[1].sum()) == 2
    if case in ("shipped", "wide"):
        assert int(cb[0].sum()) == 2 and int(cb[T - 1].sum()) == 2 and int(cb.all(0).sum()) == 1 and int(clear.sum()) > int(cb.sum())
    if case in ("one_step", "cut"):
        assert bool(cb[T - 1].all()) and int(cb.sum()) == B
    want = rref.update(_P(op), ob, mb, cb, lb)
    heads = op.sequence(ob, mb, cb)
    op_loss = _kl_torch(heads.reshape(T * B, 24), lb.reshape(T * B, 24))
    op_grads = torch.autograd.grad(op_loss, op.tensors())
    l64 = want["loss_2"]
    print(f"sequence update: loss {float(loss2[0]):.7f} fp64 {float(l64[0]):.7f}; action error {float(loss2[1]):.3e} fp64 {float(l64[1]):.3e}")
    assert abs(float(loss2[0]) - float(l64[0])) <= 2e-5 and abs(float(loss2[1]) - float(l64[1])) <= 2e-5
    assert float((rref.f64(learner.head).view(T, B, 24) - want["heads"]).abs().max()) <= 1e-4
    own = float(rref.f64(flat.grad).norm())
    assert abs(float(learner.norm) - own) <= (flat.numel / 64 + 70) * rref.U32 * own and abs(own - want["grad_norm"]) <= 1e-4 * own
    bad = []
    print(f"sequence update [{case}], {T} steps x {B} envs, R = {R}, S = {learner.S}: gradient error against fp64, relative L2")
    for name, p, g64, gop in zip(NAMES, pi.tensors(), want["grads"], op_grads):
        if case == "one_step" and name == "gru_w_hh":                              # m0 = 0 in every row: exactly zero on both sides, no ratio
            assert bool((g64 == 0).all()) and bool((flat.grad_of(p) == 0).all())
            print(f"  {name:9s}: exactly 0 in fp64 and on the device")
            continue
        e_na = float((rref.f64(flat.grad_of(p)) - g64).norm() / g64.norm())
        e_op = float((rref.f64(gop) - g64).norm() / g64.norm())
        print(f"  {name:9s}: op form {e_op:.2e}   native {e_na:.2e}   native / op {e_na / max(e_op, 1e-300):.2f}")
        if e_na > 4 * e_op:
            bad.append((name, e_op, e_na))
    assert not bad, bad
    for a, p in zip(before, pi.tensors()):                                        # learning_rate 0: the parameters keep their bits
        assert torch.equal(a, p)


def test_a_clear_truncates_the_sequence():
    """changing m_init of an env cleared at t = 1 changes that env's heads at t = 0 only: rows t >= 1 are bit for bit equal"""
    T, N, B, R = 3, 6, 6, 16
    pi = _policy(22, R)
    stores = _stores(pi, 22, T, N, clears=[(1, 2)])
    learner, flat = _learner(pi, stores, B, lr=0.0, use_graph=False)
    before = flat.flat.clone()
    learner.update(torch.arange(N, device="cuda"))
    h0 = learner.head.clone().view(T, B, 24)
    learner.m_init[2] += 1.0
    learner.m_init[4] += 1.0
    learner.update(None)                                                          # the fixed buffers as they stand
    h1 = learner.head.view(T, B, 24)
    torch.cuda.synchronize()
    assert not torch.equal(h0[0, 2], h1[0, 2]) and torch.equal(h0[1:, 2], h1[1:, 2])
    assert not torch.equal(h0[0, 4], h1[0, 4]) and not torch.equal(h0[2, 4], h1[2, 4])       # an env that is not cleared carries the change on
    others = [0, 1, 3, 5]
    assert torch.equal(h0[:, others], h1[:, others])
    assert torch.equal(flat.flat, before) and flat.t.tolist() == [2]


def test_graph_replay_gives_the_bits_of_eager_calls():
    """two learners from equal state, one captured at its third call, one eager throughout: after each of five updates on changing minibatches, the
    inputs changed in place before the fifth, the loss, the gradient, the norm and the parameters have equal bits"""
    T, N, B, R = 4, 18, 6, 16
    runs = []
    for use_graph in (True, False):
        pi = _policy(23, R)
        stores = _stores(pi, 23, T, N, noise=(0.3, 0.5), clears=[(0, 1), (2, 5), (1, 12), (3, 17)])
        obs, labels, mem0, clear = stores
        learner, flat = _learner(pi, stores, B, lr=1e-3, use_graph=use_graph)
        perm = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
        rec = []
        for k in range(5):
            if k == 4:
                with torch.no_grad():                                             # the graph reads its inputs in place
                    labels.mul_(0.9); obs.add_(0.01); mem0.mul_(0.5); clear[1, :] = 1
            l2 = learner.update(perm[(k % 3) * B:(k % 3 + 1) * B]).clone()
            torch.cuda.synchronize()
            rec.append((l2, flat.grad.clone(), flat.flat.clone(), learner.norm.clone()))
        assert (learner.graph is not None) == use_graph and flat.t.tolist() == [5]
        runs.append(rec)
    for k, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
    assert not torch.equal(runs[0][0][2], runs[0][4][2]) and all(bool(torch.isfinite(x).all()) for rec in runs[0] for x in rec)


def test_graph_replay_gives_the_bits_of_eager_calls_at_the_shipped_shape(monkeypatch):
    """the same at 51 envs x 20 steps, R = 64 - 24 + 5 T = 124 launches in one graph, the split-K factors of a real run - over four updates on
    changing minibatches, captured at the third: loss, gradient, norm and parameters have equal bits"""
    monkeypatch.delenv("PGTT_PPO_SPLITK", raising=False)
    T, N, B, R, _, clears = cases.minibatch("shipped")
    runs = []
    for use_graph in (True, False):
        pi = _policy(24, R)
        stores = _stores(pi, 24, T, N, noise=(0.3, 0.5), clears=clears)
        learner, flat = _learner(pi, stores, B, lr=1e-3, use_graph=use_graph)
        cases.check_split_k("shipped", learner.S)
        perm = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        rec = []
        for k in range(4):
            l2 = learner.update(perm.roll(7 * k)[:B]).clone()
            torch.cuda.synchronize()
            rec.append((l2, flat.grad.clone(), flat.flat.clone(), learner.norm.clone()))
        assert (learner.graph is not None) == use_graph and flat.t.tolist() == [4]
        runs.append(rec)
    for k, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
    assert not torch.equal(runs[0][0][2], runs[0][3][2]) and all(bool(torch.isfinite(x).all()) for rec in runs[0] for x in rec)


# ------------------------------------------------------------------ a task only a memory can solve
LAG_T, LAG_B, LAG_R, LAG_LR, LAG_UPDATES = 8, 64, 32, 3e-4, 400


def test_the_memory_is_used():
    """64 unrolls of T = 8 whose observations are independent draws (policy177's mean + std z) and whose label at t >= 1 is the teacher's head on the
    observation of t - 1 (at t = 0: on its own).  The recurrent learner (R = 32) and the feed-forward DistillLearner start from the teacher and see
    the same rows, the same learning rate and the same number of updates; the recurrent one ends below the feed-forward one and below its own start.
    The torch-op forms of both separate on these inputs on a CPU (DESIGN.md 24 has the numbers)."""
    teacher = PolicyMLP(P177).cuda()
    T, B, R = LAG_T, LAG_B, LAG_R
    g = torch.Generator(device="cuda").manual_seed(5)
    obs = (teacher.mean + teacher.std * torch.randn(T, B, 171, device="cuda", generator=g)).contiguous()
    own = teacher.head(obs.view(T * B, 171)).view(T, B, 24)
    labels = own.clone()
    labels[1:] = own[:-1]
    labels = labels.contiguous()
    cfg = distill.DistillConfig(learning_rate=LAG_LR, memory=R)
    pi = RecurrentPolicy.from_teacher(teacher, R, seed=0)
    mem0 = torch.zeros(T, B, R, device="cuda")
    clear = torch.zeros(T, B, dtype=torch.uint8, device="cuda")
    clear[0] = 1
    rec = SequenceLearner(pi, learn.FlatParams(pi), obs, labels, mem0, clear, B, cfg)
    net = distill.student_net(teacher, "cuda")
    ff = distill.DistillLearner(net, learn.FlatParams(net), teacher.mean.clone().contiguous(), teacher.std.clone().contiguous(), obs.view(T * B, 171),
                                labels.view(T * B, 24), T * B, distill.DistillConfig(learning_rate=LAG_LR))
    envs, rows = torch.arange(B, device="cuda"), torch.arange(T * B, device="cuda")
    kl_rec = [rec.update(envs)[0].clone() for _ in range(LAG_UPDATES + 1)]       # call k reports the loss before its own step: entry 0 is the start
    kl_ff = [ff.update(rows)[0].clone() for _ in range(LAG_UPDATES + 1)]
    first, last, first_ff, last_ff = float(kl_rec[0]), float(kl_rec[-1]), float(kl_ff[0]), float(kl_ff[-1])
    print(f"lagged labels, {LAG_UPDATES} updates: recurrent KL {first:.4f} -> {last:.4f}; feed-forward KL {first_ff:.4f} -> {last_ff:.4f}")
    assert all(np.isfinite(v) for v in (first, last, first_ff, last_ff))
    assert abs(first - first_ff) <= 1e-3 * first_ff                              # W_m = 0: both start as the teacher
    assert last < last_ff and last < first


# ------------------------------------------------------------------ the roll-out
T = 4


def _env(n=64, seed=3, episode_length=None):
    from phase_guided_terrain_traversal_amd.env import Joystick
    terrain = np.load(LEVEL1)
    variant = np.random.default_rng(0).integers(0, terrain.shape[0], n).astype(np.int32)
    cfg = configs.training_config()
    if episode_length is not None:
        cfg["episode_length"] = episode_length
    env = Joystick("stairs", cfg, num_envs=n, terrain=terrain, device="cuda:0", variant=torch.from_numpy(variant), autoreset=True,
                   depth=dict(width=32, height=24), elevation=dict(grid=32))
    env.reset(seed)
    return env


def _teacher():
    return PolicyMLP(P177).cuda()


def _load(actor, pi):
    actor.load([(m.weight, m.bias) for m in pi.layers], pi.mean, pi.std)
    return actor


def _recurrent_rollout(env, pi, seed=0):
    roll = distill.Rollout(env, pi, env.elevation_obs, T, seed=seed, memory=16)
    student = RecurrentPolicy.from_teacher(pi, 16, seed=1)
    with torch.no_grad():
        student.mem_w.copy_(torch.randn(24, 16, generator=torch.Generator().manual_seed(1)) * 0.2)
    roll.student.load(student.cuda())
    roll.student.reset_memory()
    return roll


def test_rollout_rows_labels_and_clears():
    from phase_guided_terrain_traversal_amd.acting import FusedActor
    env, pi = _env(episode_length=2), _teacher()
    roll = _recurrent_rollout(env, pi)
    assert roll.draw_mask(0.5, torch.Generator(device="cuda").manual_seed(4)) == 0.5
    probe = _load(FusedActor(env, 1, seed=9), pi)
    head = torch.zeros(64, 24, device="cuda")
    seen, want, dones, mems = [], [], [], []
    for t in range(T):
        seen.append(env.elevation_obs.clone())
        probe.act(deterministic=True, head=head, store=False)
        want.append(head.clone())
        roll.step_recurrent(t)
        torch.cuda.synchronize()
        dones.append(env.buffers["done"].clone() > 0)
        mems.append(roll.student.mem.clone())
        mixed = torch.where(roll.mask[:, None], roll.teacher.action, roll.student.action)
        assert torch.equal(roll.action, mixed)
    S = roll.student.storage
    for t in range(T):
        assert torch.equal(S["obs"][t], seen[t]) and torch.equal(roll.labels[t], want[t]), t
    assert bool((S["clear"][0] == 1).all()) and bool((S["mem0"][0] == 0).all())           # the initial clear
    assert any(bool(d.all()) for d in dones[:-1])                                          # episode_length 2: every env is truncated inside the unroll
    for t in range(1, T):
        d = dones[t - 1]
        assert torch.equal(S["clear"][t].bool(), d), t                                     # exactly the envs whose done was set
        assert bool((S["mem0"][t][d] == 0).all()) and torch.equal(S["mem0"][t][~d], mems[t - 1][~d]), t
    assert bool((mems[0] != 0).any()) and bool((roll.teacher.action[roll.mask] != roll.student.action[roll.mask]).any())
    env.close()


def test_rollout_under_the_teacher_is_the_teachers_plain_rollout():
    """beta = (1, 1): the env ends where a plain deterministic FusedActor roll-out of the teacher ends, bit for bit"""
    from phase_guided_terrain_traversal_amd.acting import FusedActor
    a, b, pi = _env(), _env(), _teacher()
    roll = _recurrent_rollout(a, pi)
    assert roll.draw_mask(1.0, torch.Generator(device="cuda").manual_seed(5)) == 1.0
    roll.rollout()
    plain = _load(FusedActor(b, T, seed=7), pi)
    for _ in range(T):
        plain.act(deterministic=True)
        b.step(plain.action)
        plain.record()
    torch.cuda.synchronize()
    for key in ("state", "istate", "obs_state", "obs_priv", "reward", "done"):
        assert torch.equal(a.buffers[key], b.buffers[key]), key
    assert torch.equal(a.elevation_obs, b.elevation_obs)
    a.close(); b.close()


# ------------------------------------------------------------------ end to end
def test_distill_end_to_end_with_a_memory(tmp_path):
    env, pi = _env(), _teacher()
    cfg = distill.DistillConfig(memory=16, iterations=2, unroll_length=T, epochs=1, batch_size=64, learning_rate=1e-4, beta=(1.0, 0.0), seed=2)
    out = distill.distill(env, pi, cfg, obs="elevation")
    torch.cuda.synchronize()
    assert len(out.history) == 2 and [m["drive_share"] for m in out.history] == [1.0, 0.0] and all(m["updates"] == 4 for m in out.history)
    for m in out.history:
        assert all(np.isfinite(v) for v in m.values()), m
        assert m["kl"] >= 0 and m["action_error"] >= 0
    start = RecurrentPolicy.from_teacher(pi, 16, seed=2).arrays()
    assert sorted(out.arrays) == sorted(start) and len(out.arrays) == 2 + 13
    for k in NAMES:
        assert np.isfinite(out.arrays[k]).all() and np.abs(out.arrays[k] - start[k]).max() > 0, k      # every trained tensor moved
    assert np.array_equal(out.arrays["mean"], start["mean"]) and np.array_equal(out.arrays["std"], start["std"])
    path = str(tmp_path / "recurrent_student.npz")
    out.save(path)
    loaded = RecurrentPolicy.load(path)
    loaded.requires_grad_(False)
    actor = out.actor                                                                      # the live RecurrentActor, the final weights loaded
    actor.reset_memory()
    mem, head = torch.zeros(64, 16), torch.zeros(64, 24, device="cuda")
    for t in range(4):
        obs = env.elevation_obs.clone()
        clear = torch.ones(64, dtype=torch.bool) if t == 0 else (env.buffers["done"] > 0).cpu()
        actor.act(head=head)
        torch.cuda.synchronize()
        _, want, mem = loaded.step(obs.cpu(), mem, clear)
        assert float((head.cpu() - want).abs().max()) <= 1e-5, t
        env.step(actor.action)
    print(f"end to end, memory 16: KL {out.history[0]['kl']:.5f} -> {out.history[1]['kl']:.5f}")
    ff = distill.distill(env, pi, distill.DistillConfig(memory=0, iterations=1, unroll_length=T, batch_size=64), obs="elevation")
    ff_path = str(tmp_path / "ff_student.npz")
    ff.save(ff_path)
    assert not any(k.startswith("gru_") or k == "mem_w" for k in np.load(ff_path).files)
    assert PolicyMLP(path).mean.shape[0] == 171 and len(PolicyMLP(path).layers) == 4        # the feed-forward reader still loads the recurrent file
    env.close()


def test_the_evaluator_on_both_kinds_of_file(tmp_path, monkeypatch):
    import evaluate
    cfg = configs.evaluation_config("pgtt")
    cfg["episode_length"] = 10
    monkeypatch.setattr(evaluate.configs, "evaluation_config", lambda method="pgtt": copy.deepcopy(cfg))
    pi = RecurrentPolicy.from_teacher(PolicyMLP(P177), 16, seed=0)
    with torch.no_grad():
        pi.mem_w.copy_(torch.randn(24, 16, generator=torch.Generator().manual_seed(3)) * 0.05)
    path = str(tmp_path / "recurrent.npz")
    pi.save(path)
    args = lambda policy: evaluate.make_parser().parse_args(["--terrain_file", "level1", "--policy", policy])
    rec = evaluate.run_evaluation(args(path), num_eval_envs=16, verbose=False)
    assert rec["num_eval_envs"] == 16 and all(np.isfinite(v) for v in rec.values()) and 0 <= rec["survivors"] <= 16
    assert 0 < rec["avg_episode_length"] <= 10
    ff = evaluate.run_evaluation(args("policy177"), num_eval_envs=16, verbose=False)
    monkeypatch.setattr(evaluate, "recurrent_file", lambda p: False)                        # the parent's path: the new branch is never asked
    old = evaluate.run_evaluation(args("policy177"), num_eval_envs=16, verbose=False)
    assert ff == old
    as_ff = evaluate.run_evaluation(args(path), num_eval_envs=16, verbose=False)            # the recurrent file read as a feed-forward one still runs
    assert all(np.isfinite(v) for v in as_ff.values())
