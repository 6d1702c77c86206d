"""Distil a student perception module (perceive.ScanEstimator: depth image + proprioceptive rows -> the 117 height-scan rows) against the env's own
scan, under a teacher policy that was trained on the privileged scan.  No counterpart in the reference, whose policies read the scan.

    python train_student.py --teacher policy177 --terrain level4 --num_envs 4096 --iters 20 --horizon 16 --beta 1.0,0.0 --out student.npz
    python evaluate.py --method pgtt --terrain_file level4 --policy policy177 --student student.npz

Each iteration rolls out `--horizon` steps (acting.FusedActor, the teacher's tanh-normal samples).  The first beta * N envs act on the true
observation and the rest on env.student_obs - the observation whose scan rows the student estimated, computed by libpgtt_perceive.so inside
env.step - so the data drifts from the teacher's states to the student's own (DAgger); beta moves linearly from b0 to b1 over the iterations.
Every step's (depth, obs, scan_target) is kept; the iteration ends with Adam steps on a Huber loss over minibatches of it (torch autograd on the
ScanEstimator: the library is forward only) and repacks the new weights into the kernel (StudentPerception.load).  It logs the RMSE per band of
scan rows: the 6 x 9 cells ahead of the base, the 9 under it and the 6 x 9 behind it.
"""
import argparse
import os
import time

import numpy as np
import torch

from phase_guided_terrain_traversal_amd import configs, mjcf, perceive
from phase_guided_terrain_traversal_amd.acting import FusedActor
from phase_guided_terrain_traversal_amd.env import Joystick
from phase_guided_terrain_traversal_amd.policy import PolicyMLP, _DIR as POLICY_DIR
from phase_guided_terrain_traversal_amd.randomize import domain_randomize

ROOT = os.path.dirname(os.path.abspath(__file__))
DEVICE = "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0"))
HUBER_DELTA = 0.1            # metres: quadratic inside a decimetre, linear past it (a step edge seen late is an outlier, not the norm)


def load_terrain(spec):
    p = spec if os.path.exists(spec) else os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains",
                                                       os.path.basename(spec).replace(".npy", "") + ".npy")
    return np.load(p)


def load_teacher(spec, device):
    p = spec if os.path.exists(spec) else os.path.join(POLICY_DIR, spec.replace(".npz", "") + ".npz")
    return PolicyMLP(p).to(device)


class Collector:
    """roll-outs of a student env under the teacher; `mix` is the observation the actor reads: the first round(beta N) envs' true rows, the
    others' student rows"""

    def __init__(self, env, teacher, horizon, seed=0):
        assert env.student is not None, "Collector needs Joystick(..., depth=..., student=...)"
        self.env, self.T = env, int(horizon)
        self.mix = torch.zeros_like(env.buffers["obs_state"])
        self.actor = FusedActor(env, self.T, seed=seed, obs=self.mix)
        self.actor.load([(m.weight, m.bias) for m in teacher.layers], teacher.mean, teacher.std)
        self._ids = torch.arange(env.num_envs, device=env.device)[:, None]

    @torch.no_grad()
    def collect(self, beta):
        """-> (depth [T N, H, W], obs [T N, obs_dim], target [T N, 117]) of `horizon` steps, each taken BEFORE the step it precedes"""
        env = self.env
        true_rows = self._ids < round(float(beta) * env.num_envs)
        depth, obs, target = [], [], []
        self.actor.rewind()
        for _ in range(self.T):
            self.mix.copy_(torch.where(true_rows, env.buffers["obs_state"], env.student_obs))
            depth.append(env.depth.clone()); obs.append(env.buffers["obs_state"].clone()); target.append(perceive.scan_target(env))
            self.actor.step()
        return torch.cat(depth), torch.cat(obs), torch.cat(target)


def huber(est, data, batch=4096):
    """mean Huber loss of the estimator on (depth, obs, target), no gradient"""
    depth, obs, target = data
    total = 0.0
    with torch.no_grad():
        for i in range(0, depth.shape[0], batch):
            s = slice(i, i + batch)
            total += float(torch.nn.functional.huber_loss(est(depth[s], obs[s]), target[s], delta=HUBER_DELTA, reduction="sum"))
    return total / target.numel()


def band_rmse(est, data, batch=4096):
    """{"ahead" | "under" | "behind": RMSE in metres over the band's scan rows}"""
    depth, obs, target = data
    sq = torch.zeros(perceive.NSCAN, device=depth.device, dtype=torch.float64)
    with torch.no_grad():
        for i in range(0, depth.shape[0], batch):
            s = slice(i, i + batch)
            sq += ((est(depth[s], obs[s]) - target[s]).double() ** 2).sum(0)
    return {k: float((sq[b].sum() / (depth.shape[0] * len(range(*b.indices(perceive.NSCAN))))).sqrt()) for k, b in perceive.BANDS.items()}


def fit(est, opt, data, steps, batch, generator):
    """`steps` Adam steps on minibatches drawn without replacement (a new permutation when the data runs out) -> mean loss"""
    depth, obs, target = data
    n, total, perm, at = depth.shape[0], 0.0, None, 0
    for _ in range(steps):
        if perm is None or at + batch > n:
            perm, at = torch.randperm(n, device=depth.device, generator=generator), 0
        idx = perm[at:at + batch]; at += batch
        loss = torch.nn.functional.huber_loss(est(depth[idx], obs[idx]), target[idx], delta=HUBER_DELTA)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        total += float(loss.detach())
    return total / max(1, steps)


def make_env(args, est):
    cfg = configs.training_config(args.method)
    model = mjcf.load_model("stairs")
    terrain = load_terrain(args.terrain)
    dr = domain_randomize(model, args.num_envs, seed=args.seed, terrain=terrain)
    noise = dict(sigma=args.depth_noise, dropout=args.depth_dropout, seed=args.seed) if (args.depth_noise > 0 or args.depth_dropout > 0) else None
    return Joystick("stairs", cfg, num_envs=args.num_envs, terrain=terrain, device=DEVICE, autoreset=True, params=torch.from_numpy(dr["params"]),
                    variant=torch.from_numpy(dr["variant"]), box_friction=torch.from_numpy(dr["box_friction"]), depth=dict(noise=noise), student=est)


def run(args):
    torch.manual_seed(args.seed)
    est = (perceive.ScanEstimator.load(args.resume) if args.resume else perceive.ScanEstimator(perceive.config(args.method))).to(DEVICE)
    env = make_env(args, est)
    col = Collector(env, load_teacher(args.teacher, DEVICE), args.horizon, seed=args.seed)
    opt = torch.optim.Adam(est.parameters(), lr=args.learning_rate)
    gen = torch.Generator(device=DEVICE).manual_seed(args.seed)
    b0, b1 = (float(v) for v in args.beta.split(","))
    env.reset(args.seed)
    t0, rm = time.time(), None
    for it in range(args.iters):
        beta = b0 + (b1 - b0) * (it / max(1, args.iters - 1))
        data = col.collect(beta)
        before = huber(est, data)
        n = data[0].shape[0]
        loss = fit(est, opt, data, max(1, args.epochs * n // args.batch_size), min(args.batch_size, n), gen)
        env.student.load(est)
        rm = band_rmse(est, data)
        print(f"iter {it:3d}  beta {beta:.2f}  samples {n}  huber before {before:.5f}  train {loss:.5f}  rmse m  ahead {rm['ahead']:.4f}  under {rm['under']:.4f}  "
              f"behind {rm['behind']:.4f}  {time.time() - t0:6.1f} s", flush=True)
        if args.max_seconds and time.time() - t0 > args.max_seconds:
            print(f"stopping after iteration {it}: --max_seconds {args.max_seconds}")
            break
    est.cpu().save(args.out)
    print(f"saved {args.out}")
    env.close()
    return rm


def make_parser():
    ap = argparse.ArgumentParser(description="Distil a depth-to-height-scan student against the env's scan (MI355X-native PGTT env)")
    ap.add_argument("--method", type=str, default="pgtt")
    ap.add_argument("--teacher", type=str, default="policy177", help="an exported policy (.npz path or a shipped one's name) trained on the true observation")
    ap.add_argument("--terrain", type=str, default="level4")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=16, help="steps rolled out (and kept) per iteration")
    ap.add_argument("--beta", type=str, default="1.0,0.0", help="b0,b1: share of the envs acting on the true observation, first and last iteration")
    ap.add_argument("--epochs", type=int, default=1, help="passes over an iteration's data")
    ap.add_argument("--batch_size", type=int, default=1024)
    ap.add_argument("--learning_rate", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--depth_noise", type=float, default=0.0, help="relative range noise of the camera (DepthCamera noise sigma)")
    ap.add_argument("--depth_dropout", type=float, default=0.0, help="probability that a pixel reads far")
    ap.add_argument("--resume", type=str, default=None, help="continue from a saved student.npz")
    ap.add_argument("--max_seconds", type=float, default=0.0, help="stop after the iteration that passes this wall time (0 = never)")
    ap.add_argument("--out", type=str, default="student.npz")
    return ap


if __name__ == "__main__":
    run(make_parser().parse_args())
