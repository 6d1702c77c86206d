"""Cost of the in-run terrain curriculum (include/pgtt.h pgtt_curriculum) -> profiles/r09_curriculum_time.txt.

    python tools/gpu_curriculum_time.py [--n 4096] [--iters 200] [--windows 5] [--parent_tree DIR]

4096 envs, domain randomisation, policy177, auto lane layout, device events around windows of `iters` x (policy forward + pgtt_step) after warm-up.
(a) level4 alone, curriculum off, on this build and - with --parent_tree, a checkout of the parent commit with its libpgtt.so built - on the parent's
    build, the two alternating (each in a process of its own that imports the package of its own tree: the structs of the two ABIs differ);
(b) the five-level ladder level1,4,7,10,13: the step with the curriculum off (labels fixed) and on, and pgtt_curriculum alone (curriculum_kernel + the
    masked reset launches + the restore) when no env finished and when 1 % of the envs did (done flags set by hand; the call leaves them set, so
    every repetition restarts the same envs);
(c) physics_kernel / observe_kernel times (the library's own events) with run-time labels on the ladder table against the grouped hand-out on level4.
    HBM-side bytes and the split of pgtt_curriculum into its seven launches come from profiler runs of their own, for which `--workload` only steps:
        rocprofv3 --kernel-trace --stats -d OUT/kt -o p --output-format csv -- python tools/gpu_curriculum_time.py --workload ladder_curriculum --steps 400
        rocprofv3 --pmc FETCH_SIZE -d OUT/pmc_W_FETCH_SIZE -o p --output-format csv -- python tools/gpu_curriculum_time.py --workload W --steps 60
        (the same with WRITE_SIZE; W = level4 | ladder_fixed | ladder_curriculum), summarised by tools/pmc_summary.py / tools/kernel_stats_top.py."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("PGTT_TIME_TREE", ROOT))          # the child of (a) imports the tree it measures

from phase_guided_terrain_traversal_amd import configs, mjcf, policy  # noqa: E402
from phase_guided_terrain_traversal_amd.env import Joystick  # noqa: E402
from phase_guided_terrain_traversal_amd.randomize import domain_randomize  # noqa: E402

A = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains")
LADDER = ("level1", "level4", "level7", "level10", "level13")


def windows(fn, iters, nwin):
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(nwin):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)          # us per iteration
    return out


def make_level4(n):
    t = np.load(os.path.join(A, "level4.npy"))
    dr = domain_randomize(mjcf.load_model("stairs"), n, seed=1, terrain=t)
    return Joystick("stairs", configs.training_config(), num_envs=n, terrain=t, device="cuda:0", autoreset=True, params=torch.from_numpy(dr["params"]),
                    variant=torch.from_numpy(dr["variant"]), box_friction=torch.from_numpy(dr["box_friction"]))


def make_ladder(n, cur):
    from phase_guided_terrain_traversal_amd import curriculum
    tabs = [np.load(os.path.join(A, f + ".npy")) for f in LADDER]
    table, start = curriculum.stack_levels(tabs)
    dr = domain_randomize(mjcf.load_model("stairs"), n, seed=1, terrain=table, level_start=start, init_level=(0, len(LADDER) - 1))
    kw = dict(curriculum=dict(cur), level=torch.from_numpy(dr["level"])) if cur is not None else {}
    return Joystick("stairs", configs.training_config(), num_envs=n, terrain=tabs, device="cuda:0", autoreset=True, params=torch.from_numpy(dr["params"]),
                    variant=torch.from_numpy(dr["variant"]), box_friction=torch.from_numpy(dr["box_friction"]), **kw)


def policy_step(env, net):
    def fn():
        with torch.no_grad():
            env.step(net(env.buffers["obs_state"]))
    return fn


def child_off(args):
    """(a): level4, curriculum off, on the tree (package + its libpgtt.so) this process imported"""
    net = policy.load_policy("policy177", device="cuda:0")
    env = make_level4(args.n)
    env.reset(0)
    print(json.dumps(windows(policy_step(env, net), args.iters, args.windows)))


def fmt(w):
    return f"{np.mean(w):8.1f} us  (windows {' '.join(f'{x:.1f}' for x in w)}; spread {max(w) - min(w):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit with its libpgtt.so built")
    ap.add_argument("--child", default=None)
    ap.add_argument("--workload", default=None, choices=("level4", "ladder_fixed", "ladder_curriculum"), help="only step this workload (under a profiler)")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_curriculum_time.txt"))
    args = ap.parse_args()
    if args.child == "off":
        return child_off(args)
    if args.workload:
        env = make_level4(args.n) if args.workload == "level4" else make_ladder(args.n, dict(promote_tracking=0.65, demote_length=0.5) if args.workload == "ladder_curriculum" else None)
        env.reset(0)
        fn = policy_step(env, policy.load_policy("policy177", device="cuda:0"))
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return
    n, rows = args.n, []
    libs = [("this build", None)] + ([("parent build", os.path.abspath(args.parent_tree))] if args.parent_tree else [])
    res = {name: [] for name, _ in libs}
    for rnd in range(3):                                            # alternating, a fresh process per library and round
        for name, lib in libs:
            env = dict(os.environ) if lib is None else dict(os.environ, PGTT_TIME_TREE=lib)
            p = subprocess.run([sys.executable, __file__, "--child", "off", "--n", str(n), "--iters", str(args.iters), "--windows", str(args.windows)],
                               env=env, capture_output=True, text=True, timeout=600, check=True)
            res[name] += json.loads(p.stdout.strip().splitlines()[-1])
    rows.append("(a) level4 alone, curriculum off: policy177 forward + pgtt_step, us per iteration, 3 alternating rounds per build")
    for name, _ in libs:
        rows.append(f"    {name:13s} {fmt(res[name])}")
    if len(libs) == 2:
        d = np.mean(res["this build"]) - np.mean(res["parent build"])
        sp = max(max(w) - min(w) for w in res.values())
        rows.append(f"    this - parent = {d:+.2f} us; largest spread between windows of one build {sp:.2f} us -> {'within' if abs(d) <= sp else 'OUTSIDE'} the spread")
    net = policy.load_policy("policy177", device="cuda:0")
    cur = dict(promote_tracking=0.65, demote_length=0.5)
    off, on = make_ladder(n, None), make_ladder(n, cur)
    off.reset(0); on.reset(0)
    rows.append(f"(b) ladder {','.join(LADDER)} ({on.terrain.shape[0]} variants), labels drawn over all levels")
    rows.append(f"    step, curriculum off  {fmt(windows(policy_step(off, net), args.iters, args.windows))}")
    rows.append(f"    step, curriculum on   {fmt(windows(policy_step(on, net), args.iters, args.windows))}")
    st = on.curriculum_stats()
    rows.append(f"      finished episodes in the timed run: {st['finished']} over {(args.windows + 1) * args.iters} steps x {n} envs (promoted {st['promoted']}, demoted {st['demoted']})")
    on.buffers["done"].zero_()
    rows.append(f"    pgtt_curriculum alone, no env finished   {fmt(windows(on.curriculum_step, args.iters, args.windows))}")
    on.buffers["done"][::100] = 1.0
    rows.append(f"    pgtt_curriculum alone, {int(on.buffers['done'].sum())} envs finished {fmt(windows(on.curriculum_step, args.iters, args.windows))}")
    on.buffers["done"].zero_()
    on.reset(0)
    rows.append("(c) kernel times from the library's events (pgtt_enable_timing), policy177, mean over the timed steps")
    l4 = make_level4(n)
    l4.reset(0)
    for name, env in (("level4, grouped labels", l4), ("ladder, fixed unsorted labels", off), ("ladder, run-time labels", on)):
        fn = policy_step(env, net)
        for _ in range(100):
            fn()
        env.enable_timing(True)
        for _ in range(args.iters):
            fn()
        p, o, k = env.kernel_ms_mean()
        env.enable_timing(False)
        rows.append(f"    {name:30s} physics_kernel {p * 1e3:7.1f} us   observe_kernel {o * 1e3:6.1f} us   ({k} steps)")
    rows.append("    HBM-side bytes and the launches of pgtt_curriculum one by one: profiler runs of their own (--workload), appended below")
    text = "\n".join([f"# tools/gpu_curriculum_time.py --n {n} --iters {args.iters} --windows {args.windows}: DR, autoreset, policy177, auto lane layout, {torch.cuda.get_device_name(0)}"] + rows) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
