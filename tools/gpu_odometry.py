"""Time and closed loop of the odometry drift, with the timing protocol of DESIGN.md 25: device events, 8 warm-up calls, median
[min, max] of 11 windows of 32 calls, one job.

    python tools/gpu_odometry.py [--out profiles/NAME.txt] [--eval]

Time, at 4096 envs: pgtt_elevation_odometry without points and with 2048 points per env; every timed call is preceded by an elementwise launch
that moves the bases by 1 cm, so that each call makes a real step, and that launch is timed alone too.  Next to them the floor of any separate
launch over the points (a copy of the same bytes) and the same update written in PyTorch ops (its draws from torch.randn, which is cheaper than
Philox blocks keyed per env).
--eval: evaluate.py --method pgtt --policy policy177 --elevation on level4 and level10, 1000 envs, seeds 0, 1 and 2, without drift, with
--odometry_drift at the defaults and at three times the defaults; then the same with --elevation_fill."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import evaluate  # noqa: E402
from phase_guided_terrain_traversal_amd import elevation  # noqa: E402

N, P, DT, DEV = 4096, 2048, 0.02, "cuda:0"
DRIFT = {"none": None, "defaults": "", "3x": ",".join(str(3 * elevation.ODOMETRY_DEFAULTS[k]) for k in ("sigma_xy", "sigma_z", "sigma_yaw", "yaw_bias", "scale"))}


def windows(fn, warm=8, nwin=11, per=32):
    """-> "median [min, max]" in us per call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(nwin):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / per)
    return f"{np.median(out):.1f} [{min(out):.1f}, {max(out):.1f}]"


def torch_update(state, pts, s, with_points):
    """the update of include/pgtt_elevation.h in PyTorch ops on persistent tensors `s`; nobody is cleared"""
    d = elevation.ODOMETRY_DEFAULTS
    b, q = state[0:3].T, state[3:7]
    D = b - s["prev"]
    sl = D.norm(dim=1).sqrt()
    n = torch.randn(N, 4, device=DEV)
    e, psi = s["e"], s["psi"]
    c, sn = psi.cos(), psi.sin()
    Dp = (1 + s["scale_e"])[:, None] * D
    e[:, 0] += (c * Dp[:, 0] - sn * Dp[:, 1]) - D[:, 0] + d["sigma_xy"] * sl * n[:, 0]
    e[:, 1] += (sn * Dp[:, 0] + c * Dp[:, 1]) - D[:, 1] + d["sigma_xy"] * sl * n[:, 1]
    e[:, 2] += (Dp[:, 2] - D[:, 2]) + d["sigma_z"] * sl * n[:, 2]
    psi.add_(s["bias_e"] * DT + d["sigma_yaw"] * DT ** 0.5 * n[:, 3])
    s["prev"].copy_(b)
    pose = s["pose"]
    pose[0:3] = (b + e).T
    ch, sh = (psi / 2).cos(), (psi / 2).sin()
    pose[3], pose[4], pose[5], pose[6] = ch * q[0] - sh * q[3], ch * q[1] - sh * q[2], ch * q[2] + sh * q[1], ch * q[3] + sh * q[0]
    if with_points:
        c, sn = psi.cos()[:, None], psi.sin()[:, None]
        r, out = pts - b[:, None, :], s["points"]
        out[..., 0] = pts[..., 0] + ((c * r[..., 0] - sn * r[..., 1]) - r[..., 0]) + e[:, None, 0]
        out[..., 1] = pts[..., 1] + ((sn * r[..., 0] + c * r[..., 1]) - r[..., 1]) + e[:, None, 1]
        out[..., 2] = pts[..., 2] + e[:, None, 2]
        out[~torch.isfinite(pts).all(-1)] = float("nan")


def times(say):
    L = elevation.lib()
    rng = np.random.default_rng(0)
    state = torch.from_numpy(np.concatenate([rng.uniform(-3, 3, (3, N)), rng.normal(size=(4, N))]).astype(np.float32)).to(DEV)
    pts = torch.from_numpy(rng.uniform(-6, 6, (N, P, 3)).astype(np.float32)).to(DEV)
    out = torch.empty_like(pts)
    stream = torch.cuda.current_stream().cuda_stream
    say(f"{N} envs; us per call, median [min, max] of 11 windows of 32 calls after 8 warm-up calls")
    for p in (0, P):
        h = C.c_void_p()
        cfg = elevation.config_struct(**elevation.PLACEHOLDER_CAMERA)
        elevation.check(L.pgtt_elevation_create(C.byref(cfg), 0, N, C.byref(h)))
        pose, odo, ctr = torch.zeros(7, N, device=DEV), torch.zeros(N, elevation.ODO_WORDS, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        o = elevation.odometry_struct(DT, **elevation.ODOMETRY_DEFAULTS, state=state.data_ptr(), points=pts.data_ptr() if p else None,
                                      points_est=out.data_ptr() if p else None, P=p, pose_est=pose.data_ptr(), odo=odo.data_ptr(), counter=ctr.data_ptr())
        elevation.check(L.pgtt_elevation_bind_odometry(h, C.byref(o)))
        elevation.check(L.pgtt_elevation_odometry(h, None, 1, 0, stream))

        def call():
            state[0:3].add_(0.01)
            L.pgtt_elevation_odometry(h, None, 0, 0, stream)
        say(f"  move + pgtt_elevation_odometry, {p} points per env: {windows(call)}")
        torch.cuda.synchronize()
        assert torch.isfinite(pose).all() and (odo[:, 0:4] != 0).any()
        L.pgtt_elevation_destroy(h)
    say(f"  the move alone:                                    {windows(lambda: state[0:3].add_(0.01))}")
    say(f"  a copy of the points ({2 * pts.numel() * 4 / 1e6:.0f} MB moved):               {windows(lambda: out.copy_(pts))}")
    s = dict(e=torch.zeros(N, 3, device=DEV), psi=torch.zeros(N, device=DEV), prev=state[0:3].T.clone(), pose=torch.zeros(7, N, device=DEV),
             scale_e=torch.rand(N, device=DEV) * 0.04 - 0.02, bias_e=torch.rand(N, device=DEV) * 0.01 - 0.005, points=out)

    def torch_call(with_points):
        state[0:3].add_(0.01)
        torch_update(state, pts, s, with_points)
    say(f"  move + the update in PyTorch ops, 0 points:        {windows(lambda: torch_call(False))}")
    say(f"  move + the update in PyTorch ops, {P} points:     {windows(lambda: torch_call(True))}")


def closed_loop(say):
    for fill in (False, True):
        say(f"evaluate.py --policy policy177 --elevation{' --elevation_fill' if fill else ''}, 1000 envs, seeds 0 / 1 / 2: survivors | reward | tracking lin | "
            "tracking ang | mean |e_xy| (m) | mean |psi| (rad) at the end of the first episode")
        for level in ("level4", "level10"):
            for name, d in DRIFT.items():
                argv = ["--task_name", "stairs", "--method", "pgtt", "--terrain_file", level, "--policy", "policy177", "--elevation"]
                argv += [] if d is None else ["--odometry_drift"] + ([d] if d else [])
                argv += ["--elevation_fill"] if fill else []
                rows = [evaluate.run_evaluation(evaluate.make_parser().parse_args(argv), num_eval_envs=1000, seed=seed, verbose=False) for seed in (0, 1, 2)]
                cols = [("survivors", "%d"), ("episode_reward", "%.2f"), ("tracking_lin_vel", "%.3f"), ("tracking_ang_vel", "%.3f"),
                        ("odometry_e_xy", "%.3f"), ("odometry_psi", "%.3f")]
                say(f"  {level:8s} {name:9s} " + " | ".join(" / ".join(fmt % r[k] for r in rows) for k, fmt in cols if k in rows[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--eval", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say(f"build: {elevation.build_info()}")
    times(say)
    if args.eval:
        closed_loop(say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
