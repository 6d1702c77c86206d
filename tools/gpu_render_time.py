"""Time libpgtt_render.so: ms per pgtt_render call and Mpixel/s for 1 / 16 / 64 views at 320x240 and 640x480, shadows on and off
(level4, tracking camera, robot and stairs in frame).  HIP events around a window of calls on the env's stream, after warm-up.
    usage: python tools/gpu_render_time.py [--out profiles/r07_render_time.txt] [--calls 50]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phase_guided_terrain_traversal_amd import configs, native, render  # noqa: E402
from phase_guided_terrain_traversal_amd.env import Joystick  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_render_time.txt"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    n = 64
    terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
    variant = torch.from_numpy(np.random.default_rng(0).integers(0, terrain.shape[0], n).astype(np.int32))
    env = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", variant=variant)
    env.reset(1)
    cam = render.Camera("track", distance=2.2, azimuth=120.0, elevation=-25.0, fovy=45.0)
    rinfo, ninfo = render.build_info(), native.build_info()
    lines = [f"# tools/gpu_render_time.py: pgtt_render (setup + pixel kernels), level4, {n} envs, tracking camera; HIP events over {a.calls} calls "
             f"after {a.warmup} warm-up calls",
             f"# libpgtt_render src={rinfo['src']} flavor={rinfo['flavor']}; libpgtt src={ninfo['src']} flavor={ninfo['flavor']}",
             f"# device {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"{'W x H':>9} {'views':>5} {'shadows':>7} {'ms/call':>9} {'Mpix/s':>9}"]
    for W, H in ((320, 240), (640, 480)):
        for shadows in (True, False):
            r = render.Renderer(env, W, H, shadows=shadows)
            for V in (1, 16, 64):
                ids = list(range(V))
                outs = r.render(ids, camera=cam)
                for _ in range(a.warmup):
                    r.render(ids, camera=cam, outputs={"rgba": outs["rgba"]})
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.calls):
                    r.render(ids, camera=cam, outputs={"rgba": outs["rgba"]})
                e.record()
                torch.cuda.synchronize()
                ms = s.elapsed_time(e) / a.calls
                lines.append(f"{W:>4}x{H:<4} {V:>5} {'on' if shadows else 'off':>7} {ms:9.3f} {V * W * H / ms / 1e3:9.1f}")
                print(lines[-1], flush=True)
            r.close()
    env.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
