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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=81920)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--memory", type=int, default=0, help="R > 0: add the recurrent policy's update and acting-step rows (DESIGN.md 24)")
    args = ap.parse_args()
    rows = args.rows
    lines = [f"{rows} synthetic rows; us per update, median [min, max] of 11 windows of 32 updates after 8 warm-up updates",
             f"libpgtt_learn build: {learn.build_info()}"]
    for mb in (1024, 5120):
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
    if args.memory:
        lines += recurrent_rows(args.memory)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
