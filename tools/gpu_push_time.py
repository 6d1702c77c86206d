"""Cost of the torso wrench and of random pushes (include/pgtt.h pgtt_push) -> profiles/r08_push_time.txt.

    python tools/gpu_push_time.py [--n 4096] [--reps 200]

level4 with domain randomisation, auto lane layout.  Rows: physics_kernel with xfrc = NULL, with a bound all-zero xfrc and with pushes on
(pgtt_physics after pgtt_push, timed alone); push_kernel alone; the whole pgtt_step with and without pushes; survivors of policy177 / policy175
on level4 under kicks of 0 - 1.5 m/s (evaluate.run_evaluation)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phase_guided_terrain_traversal_amd import configs, mjcf  # noqa: E402
from phase_guided_terrain_traversal_amd.env import Joystick  # noqa: E402
from phase_guided_terrain_traversal_amd.randomize import domain_randomize  # noqa: E402

PUSH = dict(wait=(1.0, 3.0), duration=(0.05, 0.2), velocity=(0.0, 1.5))


def make(n, terrain, **kw):
    dr = domain_randomize(mjcf.load_model("stairs"), n, seed=1, terrain=terrain)
    return Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", autoreset=True,
                    params=torch.from_numpy(dr["params"]), variant=torch.from_numpy(dr["variant"]),
                    box_friction=torch.from_numpy(dr["box_friction"]), **kw)


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--eval_envs", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_push_time.txt"))
    args = ap.parse_args()
    terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
    n = args.n
    act = torch.zeros(n, 12, device="cuda:0")
    rows = []
    envs = {"xfrc NULL": make(n, terrain), "xfrc zero-filled": make(n, terrain, xfrc=True), "pushes on": make(n, terrain, push=PUSH)}
    for name, env in envs.items():
        env.reset(0)
        for _ in range(100):                       # pushes under way in most envs
            env.step(act)
        # physics alone (the push env's scheduler runs outside the timed launches: pgtt_push is timed on its own below)
        t_phys = timed(lambda: env.physics(act), args.reps)
        env.reset(0)
        t_step = timed(lambda: env.step(act), args.reps)
        rows.append(f"physics_kernel  {name:18s} {t_phys:8.1f} us    pgtt_step {t_step:8.1f} us = {n / t_step:6.2f} M env-steps/s")
    pe = envs["pushes on"]
    t_push = timed(pe.push_step, args.reps * 5)
    rows.append(f"push_kernel     {n} envs           {t_push:8.2f} us per launch")
    nk = int((pe.buffers["push_state"][1] >= 0).sum())
    rows.append(f"                envs kicking at the end of the push run: {nk} of {n}")
    for env in envs.values():
        env.close()
    import evaluate
    for pol, method in (("policy177", "pgtt"), ("policy175", "baseline")):
        for vel in (None, "0,1.5"):
            a = evaluate.make_parser().parse_args(["--policy", pol, "--method", method, "--terrain_file", "level4"] +
                                                  ([] if vel is None else ["--push_velocity", vel]))
            t0 = time.time()
            r = evaluate.run_evaluation(a, num_eval_envs=args.eval_envs, verbose=False)
            rows.append(f"survivors {pol} level4 {'no pushes' if vel is None else 'kicks ' + vel + ' m/s':16s} {r['survivors']:5d} / {r['num_eval_envs']}"
                        f"   (episode reward {r['episode_reward']:.2f}, {time.time() - t0:.1f} s)")
    text = "\n".join([f"# tools/gpu_push_time.py --n {n} --reps {args.reps}: level4, DR, autoreset, auto lane layout, {torch.cuda.get_device_name(0)}"] + rows) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
