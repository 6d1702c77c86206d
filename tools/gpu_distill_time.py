"""Time of one distillation minibatch update with the protocol of tools/gpu_learner_time.py: 81920 synthetic rows (observations as
tests/learn_cases.py, labels = the net's own head moved by noise), device events around 32 back-to-back updates after 8 warm-up updates (which
include the native learner's two eager calls and its capture), median [min, max] of 11 such windows, at minibatches of 1024 and 5120, in one job:

    (i)  torch autograd: the same update in PyTorch ops (normalise, four Linear + SiLU, the KL, backward, clip_grad_norm_, fused Adam), eager
    (ii) native: distill.DistillLearner (hand-written HIP on one stream, one graph)

    python tools/gpu_distill_time.py [--out profiles/NAME.txt] [--memory 64]

With --memory R two more rows, the same protocol: one BPTT update of recurrent_policy.SequenceLearner (51 envs x 20 steps = 1020 rows out
of a [20, 4096, .] roll-out, one graph) next to the torch-autograd eager form of the same update (RecurrentPolicy.sequence, the KL, backward,
clip_grad_norm_, fused Adam); and one acting step at 4096 envs, pgtt_learn_recurrent_act next to pgtt_policy_act (deterministic) on the same
observation, with the three trunk launches of the recurrent step timed on their own.

With --ppo only these rows, the same protocol: the sampled acting step pgtt_learn_recurrent_act_sample next to pgtt_learn_recurrent_act
and one pgtt_learn_add_rows launch over 4096 * 24 floats; one update of recurrent_ppo.SequencePPOLearner (51 envs x 20 steps) next to the torch-autograd
eager form of the same update and next to SequenceLearner's distillation update at the same rows.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import learn_cases as cases  # noqa: E402
from gpu_learner_time import window_us  # noqa: E402
from phase_guided_terrain_traversal_amd import distill, learn  # noqa: E402

DIMS = (171, 512, 256, 128, 24)


def make(rows, seed):
    torch.manual_seed(seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    mods = []
    for i in range(4):
        mods.append(torch.nn.Linear(DIMS[i], DIMS[i + 1]))
        if i < 3:
            mods.append(torch.nn.SiLU())
    net = torch.nn.Sequential(*mods).cuda()
    obs, _ = cases.observations(rows, g)
    obs = obs.contiguous()
    mean, std = obs.mean(0).contiguous(), obs.std(0).contiguous()
    with torch.no_grad():
        labels = net((obs - mean) / std)
        labels = (labels + torch.randn(rows, 24, device="cuda", generator=g) * 0.3).contiguous()
    return net, obs, mean, std, labels, g


def kl(head, labels):
    ls, rs, lt, rt = head[:, :12], head[:, 12:], labels[:, :12], labels[:, 12:]
    ss, st = F.softplus(rs) + 1e-3, F.softplus(rt) + 1e-3
    d = lt - ls
    return (torch.log(ss / st) + 0.5 * ((st * st + d * d) / (ss * ss) - 1.0)).sum(-1).mean()


def claim(native, torch_form):
    (mn, ln, hn), (mt, lt, ht) = native, torch_form
    return ("native is faster (its maximum window is below the torch form's minimum)" if hn < lt else
            ("native is slower (its minimum window is above the torch form's maximum)" if ln > ht else "the windows overlap: no claim either way"))


def recurrent_rows(R, T=20, N=4096, b_env=51):
    """the two --memory rows"""
    import numpy as np
    from phase_guided_terrain_traversal_amd import configs
    from phase_guided_terrain_traversal_amd.acting import FusedActor
    from phase_guided_terrain_traversal_amd.env import Joystick
    from phase_guided_terrain_traversal_amd.policy import load_policy
    from phase_guided_terrain_traversal_amd.recurrent_policy import RecurrentActor, RecurrentPolicy, SequenceLearner
    teacher = load_policy("policy177", "cuda:0")
    g = torch.Generator(device="cuda").manual_seed(R)
    obs = (teacher.mean + teacher.std * torch.randn(T, N, 171, device="cuda", generator=g)).contiguous()
    labels = (teacher.head(obs.view(T * N, 171)) + torch.randn(T * N, 24, device="cuda", generator=g) * 0.3).view(T, N, 24).contiguous()
    mem0 = (torch.randn(T, N, R, device="cuda", generator=g) * 0.3).contiguous()
    clear = (torch.rand(T, N, device="cuda", generator=g) < 0.02).to(torch.uint8).contiguous()
    perm = torch.randperm(N, device="cuda", generator=g)
    chunks = [perm[k * b_env:(k + 1) * b_env] for k in range(N // b_env)]
    cfg = distill.DistillConfig(learning_rate=1e-4, max_grad_norm=1.0, memory=R)
    res = []
    for kind in ("torch", "native"):
        pi = RecurrentPolicy.from_teacher(teacher, R, seed=0)
        with torch.no_grad():
            pi.mem_w.normal_(0.0, 0.1, generator=g)
        state = {"k": 0}
        if kind == "native":
            learner = SequenceLearner(pi, learn.FlatParams(pi), obs, labels, mem0, clear, b_env, cfg)

            def update():
                learner.update(chunks[state["k"] % len(chunks)])
                state["k"] += 1
        else:
            opt = torch.optim.Adam(pi.parameters(), lr=cfg.learning_rate, fused=True)

            def update():
                e = chunks[state["k"] % len(chunks)]
                state["k"] += 1
                heads = pi.sequence(obs[:, e], mem0[0, e], clear[:, e])
                loss = kl(heads.reshape(-1, 24), labels[:, e].reshape(-1, 24))
                opt.zero_grad(set_to_none=True)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(pi.parameters(), cfg.max_grad_norm)
                opt.step()
        res.append(window_us(update))
        assert kind == "torch" or learner.graph is not None
        assert all(bool(torch.isfinite(p).all()) for p in pi.parameters())
    (mt, lt, ht), (mn, ln, hn) = res
    lines = [f"memory {R}, {b_env} envs x {T} steps = {b_env * T} rows: (i) torch autograd, eager {mt:9.1f} [{lt:.1f}, {ht:.1f}]   (ii) native, one graph "
             f"{mn:9.1f} [{ln:.1f}, {hn:.1f}]   (i) / (ii) = {mt / mn:.2f} (ratio of medians); " + claim(res[1], res[0])]
    # the acting step
    terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
    variant = np.random.default_rng(0).integers(0, terrain.shape[0], N).astype(np.int32)
    env = Joystick("stairs", configs.training_config(), num_envs=N, terrain=terrain, device="cuda:0", variant=torch.from_numpy(variant), autoreset=True)
    env.reset(0)
    ff = FusedActor(env, 1, seed=0)
    ff.load([(m.weight, m.bias) for m in teacher.layers], teacher.mean, teacher.std)
    rec = RecurrentActor(env, 1, R)
    pi = RecurrentPolicy.from_teacher(teacher, R, seed=0)
    rec.load(pi)
    L, st = learn.lib(), learn._stream(env.device)
    w = rec.work
    bufs = [w[:N * 171], w[N * 171:N * 683], w[N * 683:N * 939], w[N * 939:N * 1067], w[N * 1067:N * 1579]]
    dims = (171, 512, 256, 128)

    def trunk():
        for i in range(3):
            learn.check(L.pgtt_learn_linear_forward(bufs[i].data_ptr(), rec.w[i].data_ptr(), rec.b[i].data_ptr(), N, dims[i], dims[i + 1], 1,
                                                    bufs[i + 1].data_ptr(), bufs[4].data_ptr(), st))
    t_ff = window_us(lambda: ff.act(deterministic=True, store=False))
    t_rec = window_us(lambda: rec.act())
    t_trunk = window_us(trunk)
    lines.append(f"acting step, {N} envs, memory {R}: pgtt_policy_act (deterministic) {t_ff[0]:8.1f} [{t_ff[1]:.1f}, {t_ff[2]:.1f}]   pgtt_learn_recurrent_act "
                 f"{t_rec[0]:8.1f} [{t_rec[1]:.1f}, {t_rec[2]:.1f}]   ratio of medians {t_rec[0] / t_ff[0]:.2f}; its three trunk launches alone "
                 f"{t_trunk[0]:8.1f} [{t_trunk[1]:.1f}, {t_trunk[2]:.1f}], the normalising copy and the recurrent kernel by difference {t_rec[0] - t_trunk[0]:.1f}")
    env.close()
    return lines


def ppo_rows(R, T=20, N=4096, b_env=51):
    """the --ppo rows: the sampled acting step next to the deterministic one and one pgtt_learn_add_rows launch over N * 24 floats
    (the cheapest alternative to fusing the sampling: a sixth launch), and one recurrent PPO update next to its torch-autograd eager form and next to
    the distillation update of SequenceLearner at the same rows"""
    import numpy as np
    from phase_guided_terrain_traversal_amd import configs, ppo, recurrent_ppo
    from phase_guided_terrain_traversal_amd.env import Joystick
    from phase_guided_terrain_traversal_amd.policy import load_policy
    from phase_guided_terrain_traversal_amd.recurrent_policy import RecurrentActor, RecurrentPolicy, SequenceLearner
    fmt = lambda t: f"{t[0]:8.1f} [{t[1]:.1f}, {t[2]:.1f}]"
    teacher = load_policy("policy177", "cuda:0")
    # ---- the acting step
    terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
    variant = np.random.default_rng(0).integers(0, terrain.shape[0], N).astype(np.int32)
    env = Joystick("stairs", configs.training_config(), num_envs=N, terrain=terrain, device="cuda:0", variant=torch.from_numpy(variant), autoreset=True)
    env.reset(0)
    rec = RecurrentActor(env, 1, R)
    rec.load(RecurrentPolicy.from_teacher(teacher, R, seed=0))
    L, st = learn.lib(), learn._stream(env.device)
    a, b, out = (torch.randn(N * 24, device="cuda") for _ in range(3))
    t_det = window_us(lambda: rec.act())
    t_smp = window_us(lambda: rec.act(sample=True))
    t_det_s = window_us(lambda: rec.act(0))
    t_smp_s = window_us(lambda: rec.act(0, sample=True))
    t_add = window_us(lambda: learn.check(L.pgtt_learn_add_rows(a.data_ptr(), b.data_ptr(), N * 24, out.data_ptr(), st)))
    bar = t_det[0] + t_add[0]
    lines = [f"acting step, {N} envs, memory {R}, no storage rows: pgtt_learn_recurrent_act {fmt(t_det)}   pgtt_learn_recurrent_act_sample {fmt(t_smp)}   "
             f"one pgtt_learn_add_rows over {N * 24} floats {fmt(t_add)}   sampled - deterministic {t_smp[0] - t_det[0]:.1f} (medians); the bar of a sixth "
             f"launch {bar:.1f}: the fused sampling is " + ("within it" if t_smp[0] <= bar else "ABOVE it"),
             f"acting step with its storage rows (t = 0): deterministic {fmt(t_det_s)}   sampled {fmt(t_smp_s)}"]
    env.close()
    # ---- one update
    g = torch.Generator(device="cuda").manual_seed(R)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    obs = (teacher.mean + teacher.std * r(T, N, 171)).contiguous()
    head = teacher.head(obs.view(T * N, 171))
    u = (head[:, :12] + (F.softplus(head[:, 12:]) + 1e-3) * r(T * N, 12)).view(T, N, 12).contiguous()
    logp = (ppo.ActorCritic.log_prob(head[:, :12], F.softplus(head[:, 12:]) + 1e-3, u.view(T * N, 12)) + r(T * N) * 0.2).view(T, N).contiguous()
    labels = (head + r(T * N, 24) * 0.3).view(T, N, 24).contiguous()
    mem0 = (r(T, N, R) * 0.3).contiguous()
    clear = (torch.rand(T, N, device="cuda", generator=g) < 0.02).to(torch.uint8).contiguous()
    priv = r(T, N, 215).contiguous()
    adv, ret = r(T, N).contiguous(), r(T, N).contiguous()
    mean_p, std_p = torch.zeros(215, device="cuda"), torch.ones(215, device="cuda")
    perm = torch.randperm(N, device="cuda", generator=g)
    chunks = [perm[k * b_env:(k + 1) * b_env] for k in range(N // b_env)]
    cfg = recurrent_ppo.FinetuneConfig(learning_rate=1e-4, max_grad_norm=1.0)
    res = {}
    for kind in ("torch", "native", "distill"):
        pi = RecurrentPolicy.from_teacher(teacher, R, seed=0)
        with torch.no_grad():
            pi.mem_w.normal_(0.0, 0.1, generator=g)
        state = {"k": 0}
        if kind == "distill":
            model = pi
            learner = SequenceLearner(pi, learn.FlatParams(pi), obs, labels, mem0, clear, b_env, distill.DistillConfig(learning_rate=1e-4, memory=R))
        else:
            model = recurrent_ppo.RecurrentActorCritic(pi, 215).cuda()
        if kind == "native":
            learner = recurrent_ppo.SequencePPOLearner(model, learn.FlatParams(model), obs, u, logp, mem0, clear, priv, adv, ret, mean_p, std_p, b_env, cfg)
        if kind != "torch":
            def update():
                learner.update(chunks[state["k"] % len(chunks)])
                state["k"] += 1
        else:
            opt = torch.optim.Adam(model.parameters(), lr=cfg.learning_rate, fused=True)

            def update():
                e = chunks[state["k"] % len(chunks)]
                state["k"] += 1
                hd = pi.sequence(obs[:, e], mem0[0, e], clear[:, e]).reshape(-1, 24)
                loc, scale = hd[:, :12], F.softplus(hd[:, 12:]) + 1e-3
                lp = ppo.ActorCritic.log_prob(loc, scale, u[:, e].reshape(-1, 12))
                av = adv[:, e].reshape(-1)
                av = (av - av.mean()) / (av.std(unbiased=False) + 1e-8)
                ratio = torch.exp(lp - logp[:, e].reshape(-1))
                pol = -torch.min(ratio * av, torch.clamp(ratio, 1 - cfg.clipping_epsilon, 1 + cfg.clipping_epsilon) * av).mean()
                ent = ppo.ActorCritic.entropy(loc, scale, loc + scale * torch.randn_like(loc)).mean()
                v = model.value((priv[:, e].reshape(-1, 215) - mean_p) / std_p).squeeze(-1)
                loss = pol - cfg.entropy_cost * ent + 0.25 * ((ret[:, e].reshape(-1) - v) ** 2).mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.max_grad_norm)
                opt.step()
        res[kind] = window_us(update)
        assert kind == "torch" or learner.graph is not None
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    lines.append(f"recurrent PPO update, memory {R}, {b_env} envs x {T} steps = {b_env * T} rows: (i) torch autograd, eager {fmt(res['torch'])}   (ii) native, one "
                 f"graph {fmt(res['native'])}   (i) / (ii) = {res['torch'][0] / res['native'][0]:.2f} (ratio of medians); " + claim(res["native"], res["torch"]))
    lines.append(f"the distillation update of SequenceLearner at the same rows {fmt(res['distill'])}; the PPO update's critic, policy loss and eps cost "
                 f"{res['native'][0] - res['distill'][0]:.1f} (difference of medians)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=81920)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--memory", type=int, default=0, help="R > 0: add the recurrent policy's update and acting-step rows (DESIGN.md 24)")
    ap.add_argument("--ppo", action="store_true", help="only the rows of DESIGN.md 25: the sampled acting step and the recurrent PPO update, at --memory (default 64)")
    args = ap.parse_args()
    rows = args.rows
    lines = [f"{rows} synthetic rows; us per update, median [min, max] of 11 windows of 32 updates after 8 warm-up updates",
             f"libpgtt_learn build: {learn.build_info()}"]
    if args.ppo:
        lines = [f"us per call, median [min, max] of 11 windows of 32 calls after 8 warm-up calls; libpgtt_learn build: {learn.build_info()}"]
        lines += ppo_rows(args.memory or 64)
    for mb in (() if args.ppo else (1024, 5120)):
        res = []
        for kind in ("torch", "native"):
            net, obs, mean, std, labels, g = make(rows, mb)
            perm = torch.randperm(rows, device="cuda", generator=g)
            chunks = [perm[k * mb:(k + 1) * mb] for k in range(rows // mb)]
            state = {"k": 0}
            cfg = distill.DistillConfig(learning_rate=1e-4, max_grad_norm=1.0)
            if kind == "native":
                learner = distill.DistillLearner(net, learn.FlatParams(net), mean, std, obs, labels, mb, cfg)

                def update():
                    learner.update(chunks[state["k"] % len(chunks)])
                    state["k"] += 1
            else:
                opt = torch.optim.Adam(net.parameters(), lr=cfg.learning_rate, fused=True)

                def update():
                    idx = chunks[state["k"] % len(chunks)]
                    state["k"] += 1
                    loss = kl(net((obs[idx] - mean) / std), labels[idx])
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(net.parameters(), cfg.max_grad_norm)
                    opt.step()
            res.append(window_us(update))
            assert kind == "torch" or learner.graph is not None
            assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
        (mt, lt, ht), (mn, ln, hn) = res
        lines.append(f"minibatch {mb:5d}: (i) torch autograd, eager {mt:9.1f} [{lt:.1f}, {ht:.1f}]   (ii) native, one graph {mn:9.1f} [{ln:.1f}, {hn:.1f}]   "
                     f"(i) / (ii) = {mt / mn:.2f} (ratio of medians); " +
                     ("native is faster (its maximum window is below the torch form's minimum)" if hn < lt else
                      ("native is slower (its minimum window is above the torch form's maximum)" if ln > ht else "the windows overlap: no claim either way")))
    if args.memory and not args.ppo:
        lines += recurrent_rows(args.memory)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
