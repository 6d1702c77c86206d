"""Time of one distillation minibatch update with the protocol of tools/gpu_learner_time.py: 81920 synthetic rows (observations as
tests/learn_cases.py, labels = the net's own head moved by noise), device events around 32 back-to-back updates after 8 warm-up updates (which
include the native learner's two eager calls and its capture), median [min, max] of 11 such windows, at minibatches of 1024 and 5120, in one job:

    (i)  torch autograd: the same update in PyTorch ops (normalise, four Linear + SiLU, the KL, backward, clip_grad_norm_, fused Adam), eager
    (ii) native: distill.DistillLearner (hand-written HIP on one stream, one graph)

    python tools/gpu_distill_time.py [--out profiles/NAME.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=81920)
    ap.add_argument("--out", type=str, default=None)
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
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
