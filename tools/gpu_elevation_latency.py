"""Time and closed loop of the sensor latency, with the timing protocol of DESIGN.md 25: device events, 8 warm-up calls, median
[min, max] of 11 windows of 32 calls, one job.

    python tools/gpu_elevation_latency.py [--out profiles/NAME.txt] [--parent_lib PATH] [--eval] [--seeds 0,1,2]

Time, at 4096 envs, a 64 x 48 image, G = 64: pgtt_elevation() and pgtt_elevation_delayed() at latency 0 and 2 on the same random images and poses;
every timed call is preceded by an elementwise launch that moves the bases by 1 cm, so that the window moves and the capture pose differs from the
current one, and that launch is timed alone too.  Next to them a copy of the images, the floor of the push (the same bytes each way).
--parent_lib: a libpgtt_elevation.so built from the parent commit; its pgtt_elevation() is timed in the same job.
--eval: evaluate.py --method pgtt --policy policy177 --elevation on level4 and level10, 1000 envs, without --sensor_latency and with 0, 2, 4 and
0,4, then the same with --odometry_drift."""
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

N, W, H, G, DEV = 4096, 64, 48, 64, "cuda:0"
CAMERA = dict(width=W, height=H, fovy=58.0, near=0.1, far=3.0, mount_pos=(0.3, 0.0, 0.05), mount_quat=(0.97, 0.0, 0.26, 0.0))
LATENCIES = {"no flag": None, "0": "0", "2": "2", "4": "4", "0,4": "0,4"}


def windows(fn, warm=8, nwin=11, per=32):
    """-> (median, "median [min, max]") in us per call"""
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
    return float(np.median(out)), f"{np.median(out):.1f} [{min(out):.1f}, {max(out):.1f}]"


def times(say, parent_lib=None):
    rng = np.random.default_rng(0)
    quat = np.tile([[1.0], [0.0], [0.0], [0.0]], (1, N)) + 0.05 * rng.normal(size=(4, N))
    state = torch.from_numpy(np.concatenate([rng.uniform(-3, 3, (2, N)), np.full((1, N), 0.4), quat]).astype(np.float32)).to(DEV)
    depth = torch.from_numpy(rng.uniform(0.2, 2.5, (N, H, W)).astype(np.float32)).to(DEV)
    obs = torch.zeros(N, 171, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    cfg = elevation.config_struct(**CAMERA, grid=G, res=0.04, alpha=1.0, self_half=(0.45, 0.25, 0.45), obs_dim=171, scan_row0=38)
    say(f"{N} envs, {W} x {H}, G = {G}; us per call, median [min, max] of 11 windows of 32 calls after 8 warm-up calls")
    move = lambda: state[0:2].add_(0.01)
    t_move, text = windows(move)
    say(f"  the move alone:                               {text}")

    def handle(L, latency=None):
        h = C.c_void_p()
        assert L.pgtt_elevation_create(C.byref(cfg), 0, N, C.byref(h)) == 0
        t = dict(map=torch.full((N, G, G), float("nan"), device=DEV), origin=torch.zeros(N, 2, dtype=torch.int32, device=DEV), est=torch.zeros(N, 117, device=DEV),
                 known=torch.zeros(N, 117, dtype=torch.uint8, device=DEV), obs_out=torch.zeros(N, 171, device=DEV))
        b = elevation.PgttElevationBuffers()
        b.state, b.depth, b.obs = state.data_ptr(), depth.data_ptr(), obs.data_ptr()
        for k, v in t.items():
            setattr(b, k, v.data_ptr())
        assert L.pgtt_elevation_bind(h, C.byref(b)) == 0
        if latency is not None:
            D = latency + 1
            t.update(ring=torch.zeros(D, N, H, W, device=DEV), ring_pose=torch.zeros(D, 7, N, device=DEV), lat=torch.zeros(N, dtype=torch.int32, device=DEV),
                     age=torch.zeros(N, dtype=torch.int32, device=DEV), fused=torch.zeros(N, dtype=torch.uint8, device=DEV),
                     counter=torch.zeros(1, dtype=torch.int64, device=DEV))
            l = elevation.latency_struct(ticks=(latency, latency), ring_data=t["ring"].data_ptr(), ring_pose=t["ring_pose"].data_ptr(), lat=t["lat"].data_ptr(),
                                         age=t["age"].data_ptr(), fused=t["fused"].data_ptr(), counter=t["counter"].data_ptr())
            elevation.check(L.pgtt_elevation_bind_latency(h, C.byref(l)))
        return h, t

    L = elevation.lib()
    libs = [("pgtt_elevation(), this build", L)]
    if parent_lib:
        P = C.CDLL(parent_lib)
        for name in ("pgtt_elevation_create", "pgtt_elevation_bind", "pgtt_elevation", "pgtt_elevation_destroy"):
            getattr(P, name).argtypes = elevation.SIDE.prototypes[name][1]
        P.pgtt_elevation_build_info.restype = C.c_char_p
        say(f"  parent build: {P.pgtt_elevation_build_info().decode()}")
        libs.append(("pgtt_elevation(), the parent's build", P))
    plain = None
    for label, lib in libs:
        h, t = handle(lib)
        lib.pgtt_elevation(h, None, 1, 0, stream)

        def call():
            move()
            lib.pgtt_elevation(h, None, 0, 0, stream)
        us, text = windows(call)
        plain = us if plain is None else plain
        say(f"  move + {label + ':':38s}{text}   net {us - t_move:.1f}")
        lib.pgtt_elevation_destroy(h)
    for latency in (0, 2):
        h, t = handle(L, latency)
        L.pgtt_elevation_delayed(h, None, 1, 0, stream)

        def call():
            move()
            L.pgtt_elevation_delayed(h, None, 0, 0, stream)
        us, text = windows(call)
        torch.cuda.synchronize()
        assert bool(t["fused"].all()) and bool((t["lat"] == latency).all()) and int((~torch.isnan(t["map"])).sum()) > N
        say(f"  move + pgtt_elevation_delayed(), latency {latency}:    {text}   net {us - t_move:.1f}, over the plain tick {us - plain:.1f}")
        L.pgtt_elevation_destroy(h)
    out = torch.empty_like(depth)
    us, text = windows(lambda: out.copy_(depth))
    mb = 2 * depth.numel() * 4 / 1e6
    say(f"  a copy of the images ({mb:.0f} MB moved):           {text}   {mb / us:.2f} TB/s")


def closed_loop(say, seeds):
    cols = [("survivors", "%d"), ("episode_reward", "%.2f"), ("tracking_lin_vel", "%.3f"), ("tracking_ang_vel", "%.3f")]
    for drift in (False, True):
        say(f"evaluate.py --policy policy177 --elevation{' --odometry_drift' if drift else ''} [--sensor_latency X], 1000 envs, seeds "
            f"{' / '.join(map(str, seeds))}: survivors | reward | tracking lin | tracking ang")
        for level in ("level4", "level10"):
            for name, lat in LATENCIES.items():
                argv = ["--task_name", "stairs", "--method", "pgtt", "--terrain_file", level, "--policy", "policy177", "--elevation"]
                argv += (["--odometry_drift"] if drift else []) + ([] if lat is None else ["--sensor_latency", lat])
                rows = [evaluate.run_evaluation(evaluate.make_parser().parse_args(argv), num_eval_envs=1000, seed=seed, verbose=False) for seed in seeds]
                say(f"  {level:8s} latency {name:8s} " + " | ".join(" / ".join(fmt % r[k] for r in rows) for k, fmt in cols))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--no_times", action="store_true")
    ap.add_argument("--seeds", default="0,1,2")
    args = ap.parse_args()
    fh = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        fh = open(args.out, "w")

    def say(text):
        print(text, flush=True)
        if fh:
            fh.write(text + "\n")
            fh.flush()
    say(f"build: {elevation.build_info()}")
    if not args.no_times:
        times(say, args.parent_lib)
    if args.eval:
        closed_loop(say, [int(s) for s in args.seeds.split(",")])


if __name__ == "__main__":
    main()
