"""Fine-tune a recurrent policy with PPO on what the sensors deliver (phase_guided_terrain_traversal_amd/recurrent_ppo.py): the second
stage behind train_distill.py.  No counterpart in the reference, whose policies read the true scan.

    python train_distill.py --teacher policy177 --terrain level10 --obs elevation --elevation --memory 64 --max_seconds 120 --out distilled.npz
    python train_finetune.py --policy distilled.npz --terrain level10 --obs elevation --elevation --max_seconds 120 --out finetuned.npz
    python evaluate.py --method pgtt --terrain_file level10 --policy finetuned.npz --elevation

`--policy` is a recurrent file (recurrent_policy.RecurrentPolicy.save) or a feed-forward one (a shipped policy's name or an .npz of
ppo.export_policy_npz), which is given a GRU memory of `--memory` values with a zero read-out: it starts as the policy it was.  Each iteration rolls
out `--horizon` sampled steps, fits the critic's targets by GAE and runs `--updates_per_batch` passes over `--num_minibatches` groups of whole unrolls;
the first `--critic_warmup` iterations update the critic only.  The sensor flags are those of evaluate.py and are read by the same code; `--obs` names
the observation they deliver (`state`: the true observation).  Writes the 13-tensor file evaluate.py --policy recognises.
"""
import argparse
import os
import time

import torch

import evaluate
from phase_guided_terrain_traversal_amd import configs, distill, mjcf, recurrent_ppo
from phase_guided_terrain_traversal_amd.recurrent_policy import RecurrentPolicy, memory_ok

DEVICE = evaluate.DEVICE
NEEDS = {"elevation": "--elevation", "elevation_filled": "--elevation with --elevation_fill", "student": "--student"}
OBS_CHOICES = sorted(distill.OBS_NAMES) + ["state"]


def load_policy(name: str, memory: int, seed: int = 0) -> RecurrentPolicy:
    """a recurrent file as it is; a feed-forward one through RecurrentPolicy.from_teacher(memory=R): W_m = 0, the policy it was"""
    path = name if os.path.exists(name) else os.path.join(distill.POLICY_DIR, str(name).replace(".npz", "") + ".npz")
    if not os.path.exists(path):
        raise SystemExit(f"--policy {name}: no such file and no shipped policy of that name")
    if evaluate.recurrent_file(path):
        return RecurrentPolicy.load(path)
    if not memory_ok(memory):
        raise SystemExit(f"--memory {memory}: a feed-forward --policy needs a memory that is a multiple of 16 in [16, 256]")
    return RecurrentPolicy.from_teacher(distill.PolicyMLP(path), memory=memory, seed=seed)


def check_args(args, device: str = DEVICE) -> None:
    """what can be refused before an env is built"""
    if args.num_minibatches <= 0 or args.num_envs % args.num_minibatches != 0:
        raise SystemExit(f"--num_minibatches {args.num_minibatches} does not divide --num_envs {args.num_envs}: a minibatch is a set of whole unrolls")
    if torch.device(device).type != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"fine-tuning runs on a GPU only: {device} is not one (or there is none) and there is no CPU form")


def make_env(args):
    from phase_guided_terrain_traversal_amd.env import Joystick
    from phase_guided_terrain_traversal_amd.randomize import domain_randomize
    cfg = configs.training_config(args.method)
    model = mjcf.load_model("stairs")
    terrain = evaluate.load_terrain(args.terrain)
    dr = domain_randomize(model, args.num_envs, seed=args.seed, terrain=terrain)
    env = Joystick("stairs", cfg, num_envs=args.num_envs, terrain=terrain, device=DEVICE, autoreset=True, params=torch.from_numpy(dr["params"]),
                   variant=torch.from_numpy(dr["variant"]), box_friction=torch.from_numpy(dr["box_friction"]), **evaluate.sensor_kwargs(args))
    if args.obs != "state" and getattr(env, distill.OBS_NAMES[args.obs], None) is None:
        raise SystemExit(f"--obs {args.obs} needs {NEEDS[args.obs]}")
    return env


def make_config(args) -> recurrent_ppo.FinetuneConfig:
    return recurrent_ppo.FinetuneConfig(iterations=args.iters, unroll_length=args.horizon, num_minibatches=args.num_minibatches,
                                        num_updates_per_batch=args.updates_per_batch, learning_rate=args.learning_rate, entropy_cost=args.entropy_cost,
                                        critic_warmup_iters=args.critic_warmup, seed=args.seed)


def run(args):
    policy = load_policy(args.policy, args.memory, args.seed)
    check_args(args)
    torch.manual_seed(args.seed)
    env = make_env(args)
    env.reset(args.seed)
    t0 = time.time()

    def progress(it, m):
        print(f"iter {it:4d}  {'policy' if m['policy_updates'] else 'critic'}  episode reward {m['episode_reward']:8.3f}  length {m['episode_length']:7.1f}  "
              f"step reward {m['mean_step_reward']:.4f}  loss {m['policy_loss']:.5f}  entropy {m['entropy']:.3f}  value loss {m['value_loss']:.5f}  "
              f"grad norm {m['grad_norm']:.3f}  {m['env_steps_per_s']:9.0f} env-steps/s  {time.time() - t0:6.1f} s", flush=True)
        if args.max_seconds and time.time() - t0 > args.max_seconds:
            print(f"stopping after iteration {it}: --max_seconds {args.max_seconds}")
            return True
        return False

    obs = env.buffers["obs_state"] if args.obs == "state" else args.obs
    out = recurrent_ppo.finetune(env, policy, make_config(args), obs=obs, progress_fn=progress)
    out.save(args.out)
    print(f"saved {args.out}")
    env.close()
    return out


def make_parser():
    ap = argparse.ArgumentParser(description="Fine-tune a recurrent policy with PPO on perceived observations (MI355X-native PGTT env)")
    ap.add_argument("--method", type=str, default="pgtt")
    ap.add_argument("--policy", type=str, required=True, help="a recurrent policy file, or a feed-forward one (path or a shipped policy's name) that gets --memory")
    ap.add_argument("--memory", type=int, default=64, metavar="R", help="the memory a feed-forward --policy is given (a multiple of 16 in [16, 256])")
    ap.add_argument("--terrain", type=str, default="level4")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=20, help="steps rolled out per iteration: the length of an unroll")
    ap.add_argument("--num_minibatches", type=int, default=32, help="groups of whole unrolls per pass; must divide --num_envs")
    ap.add_argument("--updates_per_batch", type=int, default=4, help="passes over an iteration's unrolls")
    ap.add_argument("--critic_warmup", type=int, default=recurrent_ppo.FinetuneConfig.critic_warmup_iters, help="iterations at the start that update the critic only")
    ap.add_argument("--learning_rate", type=float, default=recurrent_ppo.FinetuneConfig.learning_rate)
    ap.add_argument("--entropy_cost", type=float, default=1e-2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--obs", type=str, default="elevation", choices=OBS_CHOICES, help="the observation the policy reads")
    evaluate.add_sensor_args(ap)
    ap.add_argument("--max_seconds", type=float, default=0.0, help="stop after the iteration that passes this wall time (0 = never)")
    ap.add_argument("--out", type=str, default="finetuned_policy.npz")
    return ap


if __name__ == "__main__":
    run(make_parser().parse_args())
