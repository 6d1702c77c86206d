"""Time pgtt_render_map next to pgtt_render: ms per call for 4 views of 320x240 (the --video default), shadows on, level4, tracking camera.
The map is a seeded staircase with 20 % holes around each robot at G = 64 and G = 96 (res 0.04), drawn in the belief view.  HIP events around a
window of calls on the env's stream, after warm-up; the two entries are timed alternately, several rounds, and the spread is printed.
    usage: python tools/gpu_render_map_time.py [--out profiles/render_map_time.txt] [--calls 200] [--rounds 5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phase_guided_terrain_traversal_amd import configs, render  # noqa: E402
from phase_guided_terrain_traversal_amd.env import Joystick  # noqa: E402


def staircase(G, rng):
    h = 0.08 * (np.arange(G) // 4)[:, None] + rng.uniform(-0.01, 0.01, (G, G))
    h[rng.random((G, G)) < 0.2] = np.nan
    return h.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_map_time.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    n, V, W, H = 64, 4, 320, 240
    terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
    variant = torch.from_numpy(np.random.default_rng(0).integers(0, terrain.shape[0], n).astype(np.int32))
    env = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", variant=variant)
    env.reset(1)
    cam = render.Camera("track", distance=2.2, azimuth=120.0, elevation=-25.0, fovy=45.0)
    r = render.Renderer(env, W, H, shadows=True)
    ids = list(range(V))
    rng = np.random.default_rng(1)
    xy = env.buffers["state"][0:2].T.cpu().numpy()
    maps = {}
    for G in (64, 96):
        origin = np.ascontiguousarray(np.floor(xy / 0.04).astype(np.int32))
        hm = np.stack([staircase(G, rng) for _ in range(n)])              # the window's content does not depend on where its slots start
        maps[G] = dict(map=torch.from_numpy(hm).cuda(), origin=torch.from_numpy(origin).cuda(), grid=G, res=0.04)
    out = r.render(ids, camera=cam)
    keep = {"rgba": out["rgba"]}
    runs = {"pgtt_render": lambda: r.render(ids, camera=cam, outputs=keep),
            "pgtt_render_map G=64": lambda: r.render_map(ids, maps[64], camera=cam, outputs=keep),
            "pgtt_render_map G=96": lambda: r.render_map(ids, maps[96], camera=cam, outputs=keep)}
    times = {k: [] for k in runs}
    for rnd in range(a.rounds + 1):                                        # round 0 is the warm-up
        for name, fn in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.calls):
                fn()
            e.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(s.elapsed_time(e) / a.calls)
    info = render.build_info()
    lines = [f"# tools/gpu_render_map_time.py: {V} views of {W}x{H}, shadows on, level4, tracking camera; HIP events over {a.calls} calls, {a.rounds} rounds "
             f"after one warm-up round, entries alternating; ms per call (setup + pixel kernel, launch overhead included)",
             f"# libpgtt_render src={info['src']} flavor={info['flavor']}; device {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"{'entry':<24} {'median':>8} {'min':>8} {'max':>8}"]
    for name, t in times.items():
        lines.append(f"{name:<24} {np.median(t):8.4f} {min(t):8.4f} {max(t):8.4f}")
    print("\n".join(lines), flush=True)
    r.close(); env.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
