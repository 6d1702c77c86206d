"""Distil a student POLICY that reads what the sensors deliver from a teacher policy that was trained on the true height scan
(phase_guided_terrain_traversal_amd/distill.py).  No counterpart in the reference, whose policies read the scan.

    python train_distill.py --teacher policy177 --terrain level4 --obs elevation --elevation --max_seconds 300 --out student_policy.npz
    python evaluate.py --method pgtt --terrain_file level4 --policy student_policy.npz --elevation

Each iteration rolls out `--horizon` steps: the teacher labels every state with its head on the true observation, the student acts on the
perceived one, and the teacher drives a share beta of the envs that moves linearly from b0 to b1 over the iterations (DAgger).  Then `--epochs`
passes of minibatch updates on KL(teacher || student) run over the iteration's rows, all of it hand-written HIP.  The sensor flags are those of
evaluate.py and are read by the same code; `--obs` names the observation they deliver.  Prints the KL, the error of the deterministic action,
the drive share and env-steps/s per iteration.
"""
import argparse
import time

import torch

import evaluate
from phase_guided_terrain_traversal_amd import configs, distill, mjcf
from phase_guided_terrain_traversal_amd.env import Joystick
from phase_guided_terrain_traversal_amd.randomize import domain_randomize

DEVICE = evaluate.DEVICE
NEEDS = {"elevation": "--elevation", "elevation_filled": "--elevation with --elevation_fill", "student": "--student"}


def make_env(args):
    cfg = configs.training_config(args.method)
    model = mjcf.load_model("stairs")
    terrain = evaluate.load_terrain(args.terrain)
    dr = domain_randomize(model, args.num_envs, seed=args.seed, terrain=terrain)
    kw = evaluate.sensor_kwargs(args)
    env = Joystick("stairs", cfg, num_envs=args.num_envs, terrain=terrain, device=DEVICE, autoreset=True, params=torch.from_numpy(dr["params"]),
                   variant=torch.from_numpy(dr["variant"]), box_friction=torch.from_numpy(dr["box_friction"]), **kw)
    if getattr(env, distill.OBS_NAMES[args.obs], None) is None:
        raise SystemExit(f"--obs {args.obs} needs {NEEDS[args.obs]}")
    return env


def run(args):
    torch.manual_seed(args.seed)
    try:
        b0, b1 = (float(v) for v in args.beta.split(","))
    except ValueError:
        raise SystemExit(f"--beta {args.beta}: give b0,b1")
    env = make_env(args)
    env.reset(args.seed)
    cfg = distill.DistillConfig(iterations=args.iters, unroll_length=args.horizon, epochs=args.epochs, batch_size=args.batch_size,
                                learning_rate=args.learning_rate, beta=(b0, b1), seed=args.seed, memory=args.memory)
    t0 = time.time()

    def progress(it, m):
        print(f"iter {it:4d}  beta {m['beta']:.2f}  drive share {m['drive_share']:.3f}  KL {m['kl']:.5f}  action error {m['action_error']:.6f}  "
              f"grad norm {m['grad_norm']:.3f}  {m['env_steps_per_s']:9.0f} env-steps/s  {time.time() - t0:6.1f} s", flush=True)
        if args.max_seconds and time.time() - t0 > args.max_seconds:
            print(f"stopping after iteration {it}: --max_seconds {args.max_seconds}")
            return True
        return False

    student = distill.distill(env, args.teacher, cfg, obs=args.obs, progress_fn=progress)
    student.save(args.out)
    print(f"saved {args.out}")
    env.close()
    return student


def make_parser():
    ap = argparse.ArgumentParser(description="Distil a student policy on perceived observations from a privileged teacher (MI355X-native PGTT env)")
    ap.add_argument("--method", type=str, default="pgtt")
    ap.add_argument("--teacher", type=str, default="policy177", help="an exported policy (.npz path or a shipped one's name) trained on the true observation")
    ap.add_argument("--terrain", type=str, default="level4")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=20, help="steps rolled out (and kept) per iteration")
    ap.add_argument("--beta", type=str, default="1.0,0.0", help="b0,b1: share of the envs the teacher drives, first and last iteration")
    ap.add_argument("--epochs", type=int, default=1, help="passes over an iteration's rows")
    ap.add_argument("--batch_size", type=int, default=1024)
    ap.add_argument("--learning_rate", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--memory", type=int, default=0, metavar="R",
                    help="R > 0: the student is a recurrent policy with a GRU memory of R values (a multiple of 16 in [16, 256]); 0: feed-forward")
    ap.add_argument("--obs", type=str, default="elevation", choices=sorted(distill.OBS_NAMES), help="the perceived observation the student reads")
    evaluate.add_sensor_args(ap)
    ap.add_argument("--max_seconds", type=float, default=0.0, help="stop after the iteration that passes this wall time (0 = never)")
    ap.add_argument("--out", type=str, default="student_policy.npz")
    return ap


if __name__ == "__main__":
    run(make_parser().parse_args())
