"""Time of one PPO minibatch update for the three learners, and of GAE, with the protocol of DESIGN.md 14 - 16: a synthetic batch of
81920 rows (tests/learn_cases.py), minibatches of 5120; device events around 32 back-to-back replayed updates after 8 warm-up updates (which include
the two eager calls and the capture), median [min, max] of 11 such windows; all in one job on one card:

    (i)   op form:   ppo._Learner with PGTT_PPO_FUSED=0, one stream, no graph (PyTorch ops only)
    (ii)  product:   ppo._Learner as ppo.train builds it (two HIP kernels, two streams, one graph)
    (iii) native:    learn.NativeLearner (hand-written HIP on one stream, one graph)
    (iv)  ppo.compute_gae and (v) pgtt_learn_gae at T = 20, N = 4096

    python tools/gpu_learner_time.py [--out profiles/NAME.txt]

The native update counts as faster only if its maximum window is below the product path's minimum window."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import learn_cases as cases  # noqa: E402
from phase_guided_terrain_traversal_amd import learn, ppo  # noqa: E402


def window_us(fn, calls=32, warm=8, windows=11):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        e.synchronize()
        out.append(1e3 * s.elapsed_time(e) / calls)
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=81920)
    ap.add_argument("--mb", type=int, default=5120)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    rows, mb = args.rows, args.mb
    res = []
    for name, kind in (("(i)   op form: PyTorch ops, one stream, no graph", "op"), ("(ii)  product: ppo._Learner, two streams, one graph", "product"),
                       ("(iii) native: learn.NativeLearner, one stream, one graph", "native")):
        cases.set_env(kind)
        model, norm_s, norm_p, B, cfg, learner, g = cases.setup(mb, True, kind, rows=rows)
        perm = torch.randperm(rows, device="cuda", generator=g)
        chunks = [perm[k * mb:(k + 1) * mb] for k in range(rows // mb)]
        state = {"k": 0}

        def update():
            learner.update(chunks[state["k"] % len(chunks)])
            state["k"] += 1
        res.append((name, window_us(update)))
        assert kind == "op" or learner.graph is not None
        assert bool(torch.isfinite(learner.loss)) and all(bool(torch.isfinite(p).all()) for p in model.parameters())
        del learner, model, B
    T, N = 20, 4096
    gg = torch.Generator(device="cuda").manual_seed(3)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gg)
    done = (torch.rand(T, N, device="cuda", generator=gg) < 0.02).float()
    trunc = done * (torch.rand(T, N, device="cuda", generator=gg) < 0.3).float()
    rew, val, boot = r(T, N), r(T, N), r(N)
    out = (torch.empty(T, N, device="cuda"), torch.empty(T, N, device="cuda"))
    res.append(("(iv)  ppo.compute_gae, T = 20, N = 4096 (PyTorch ops)", window_us(lambda: ppo.compute_gae(trunc, done * (1.0 - trunc), rew, val, boot, 0.95, 0.97))))
    res.append(("(v)   pgtt_learn_gae, T = 20, N = 4096 (one launch)", window_us(lambda: learn.gae(trunc, done, rew, val, boot, 0.95, 0.97, out=out))))
    lines = [f"{rows} synthetic rows, minibatches of {mb}, clip active; us per call, median [min, max] of 11 windows of 32 calls after 8 warm-up calls",
             f"libpgtt_learn build: {learn.build_info()}"]
    lines += [f"{name:62s} {m:9.1f} [{lo:.1f}, {hi:.1f}]" for name, (m, lo, hi) in res]
    (_, lo2, hi2), (_, lo3, hi3) = res[1][1], res[2][1]
    verdict = "native is faster (its maximum window is below the product path's minimum)" if hi3 < lo2 else \
              ("native is slower (its minimum window is above the product path's maximum)" if lo3 > hi2 else "the windows overlap: no claim either way")
    lines.append(f"update: product / native = {res[1][1][0] / res[2][1][0]:.2f} (ratio of medians), op form / native = {res[0][1][0] / res[2][1][0]:.2f}; {verdict}")
    lines.append(f"gae: compute_gae / pgtt_learn_gae = {res[3][1][0] / res[4][1][0]:.2f} (ratio of medians)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
