"""A/B check of two builds of the side library libpgtt_elevation.so: the same seeded inputs, EVERY tensor an ElevationMap owns compared bit for bit
after every call.
   usage: python tools/gpu_ab_elevation.py OLD_DIR NEW_DIR [--out profiles/NAME.txt]
   (OLD_DIR / NEW_DIR hold the two .so files; each build runs in its own process, elevation.SIDE.path set before first use)
No env, no terrain, no libpgtt.so: the inputs are seeded numpy on hand-filled tensors, the Rig of tests/test_gpu_elevation_edges.py.
Workloads, the smallest at which these kernels can go wrong: N = 3 envs (the hold kernel's last workgroup is half empty); G = 24 at res 0.04 with
a 16 x 12 image (16-byte runs of the map and of the image, which wrap rows) and G = 9 at res 0.12 with 5 x 3 (the dword paths), so that both
windows are about a metre and catch the data; depths uniform in [0.5 near, 1.2 far] with about 10 % NaN; P = 300 points (no multiple of 256, more than one pass), about 10 % of the rows NaN or inf; base xy in [-2, 2] with env 1
negative on both axes, roll and pitch non-zero, the quaternion multiplied by 3; six ticks, the base moving inside its cell, 5 cells and 97 cells
between them; tick 0 clear_all, tick 3 clear_mask on env 1, tick 4 use_done with done[2] = 1.  Configurations, each from the image and from
the points: the plain tick with alpha = 1 and 0.5, the self filter on and off; the variance tick at its defaults and with band = 0; the fill with
3 passes and its dense outputs; the clean-up at stride 1 and 2, with and without variance, with the bound layer; latency (0, 2); odometry; and,
from the points, follow_sensor behind a sensor of every = 2, the counter set so that fresh and hold calls alternate (tick 3 is a hold with a
clear)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P, TICKS = 3, 300, 6
SHAPES = ((24, 16, 12, 0.04), (9, 5, 3, 0.12))                            # G, W, H, res: both windows are about a metre, so both catch the data
MOVES = (0.0, 0.3, 5.0, 97.0, 0.3, 5.0)                                   # cells, in front of tick t
TENSORS = ("map", "origin", "est", "known", "obs", "var", "est_var", "filled_est", "filled_dist", "filled_obs", "filled_map", "filled_dist_map",
           "cleared", "bound", "pose_est", "odo", "points_est", "ring", "ring_pose", "latency", "latency_age", "fused", "latency_counter",
           "odo_counter")
VIS = dict(margin=0.05, end_guard=0.06, sigmas=0.0)
CONFIGS = (("plain_a1_self", dict(alpha=1.0)), ("plain_a05_noself", dict(alpha=0.5, self_half=(0.0, 0.0, 0.0))),
           ("var", dict(variance=True)), ("var_band0", dict(variance=dict(band=0.0))),
           ("fill3", dict(fill=3, dense=True)),
           ("vis1", dict(visibility=dict(VIS, stride=1), dense_bound=True)), ("vis2", dict(visibility=dict(VIS, stride=2), dense_bound=True)),
           ("vis1_var", dict(visibility=dict(VIS, stride=1, sigmas=1.0), dense_bound=True, variance=True)),
           ("vis2_var", dict(visibility=dict(VIS, stride=2, sigmas=1.0), dense_bound=True, variance=True)),
           ("latency02", dict(latency=(0, 2))), ("odometry", dict(odometry=True)), ("follow2", dict(follow_sensor=True)))


def child(lib_dir, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from phase_guided_terrain_traversal_amd import elevation
    elevation.SIDE.path = os.path.join(lib_dir, "libpgtt_elevation.so")
    import elevation_edge_cases as ec
    from test_gpu_elevation_edges import Rig
    res = {"info": np.frombuffer(elevation.SIDE.build_info()["src"].encode(), np.uint8)}
    s2 = float(np.sqrt(0.5))
    for G, W, H, RES in SHAPES:
        for source in ("depth", "lidar"):
            for ci, (cname, kw) in enumerate(CONFIGS):
                follow = bool(kw.get("follow_sensor"))
                if follow and source == "depth":
                    continue                                              # the Rig gives the points' sensor a counter, the camera none
                rng = np.random.default_rng(1000 * G + 10 * ci + (source == "lidar"))
                cam = dict(width=W, height=H, fovy=70.0, near=0.2, far=1.0, mount_pos=(0.3, 0.0, 0.05), mount_quat=(s2 * 1.2, 0.0, s2 * 0.8, 0.0))
                vis = kw.get("visibility")
                S = dict(camera=cam if source == "depth" else None, sdx=0.1, sdy=0.08, row0=38, grid=G, res=RES, alpha=kw.get("alpha", 1.0),
                         self_half=kw.get("self_half", (0.25, 0.15, 0.2)), follow=follow, variance=None,
                         visibility=dict(vis, sensor_pos=(0.2, 0.0, 0.1)) if vis else None)
                rig = Rig(N, S, points=P if source == "lidar" else None)
                # the Rig is the suite's way to an env of hand-filled tensors: its env and put() serve, S is what its constructor asks for; its map knows
                # neither fill nor latency nor odometry, so the map under test is made here, with every setting of this tool
                rig.map.close()
                mkw = dict(kw, grid=G, res=RES, alpha=S["alpha"], self_half=S["self_half"])
                if source == "lidar":
                    mkw["source"] = "lidar"
                rig.map = elevation.ElevationMap(rig.env, **mkw)
                base = rng.uniform(-2.0, 2.0, (N, 2))
                base[1] = -np.abs(base[1]) - 0.1
                snaps = {}
                for t in range(TICKS):
                    base = base + MOVES[t] * RES * np.array([1.0, 0.5])
                    rpy = rng.uniform(-0.3, 0.3, (N, 3)) + np.array([0.1, -0.15, 0.0])
                    cr, sr, cp, sp, cy, sy = (f(rpy[:, k] / 2) for k in range(3) for f in (np.cos, np.sin))
                    quat = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], 1)
                    qpos = np.concatenate([base, rng.uniform(0.25, 0.4, (N, 1)), 3.0 * quat], 1)
                    obs = rng.standard_normal((N, ec.OBS_DIM))
                    src = {}
                    if source == "depth":
                        img = rng.uniform(0.5 * cam["near"], 1.2 * cam["far"], (N, H, W))
                        img[rng.random((N, H, W)) < 0.1] = np.nan
                        src["image"] = img
                    else:
                        pts = np.concatenate([base[:, None, :] + rng.uniform(-0.6, 0.6, (N, P, 2)), rng.uniform(-0.3, 0.3, (N, P, 1))], 2)
                        bad = rng.random((N, P))
                        pts[bad < 0.05] = np.nan
                        pts[(bad >= 0.05) & (bad < 0.1), 2] = np.inf
                        src["points"] = pts
                    rig.put(qpos, obs, **src)
                    done = torch.zeros(N, device="cuda")
                    if t == 4:
                        done[2] = 1.0
                    rig.env.buffers["done"].copy_(done)
                    if follow:
                        rig.counter.fill_(1 if t % 2 == 0 else 2)         # every = 2: behind a sensor call that was fresh / was not
                    mask = torch.tensor([0, 1, 0], dtype=torch.uint8) if t == 3 else None
                    rig.map.tick(clear_mask=mask, clear_all=t == 0, use_done=t == 4)
                    torch.cuda.synchronize()
                    for k in TENSORS:
                        if isinstance(getattr(rig.map, k, None), torch.Tensor):
                            snaps.setdefault(k, []).append(getattr(rig.map, k).cpu().numpy().copy())
                for k, v in snaps.items():
                    res[f"G{G}_{source}/{cname}/{k}"] = np.stack(v)
                rig.close()
    np.savez(out, **res)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype.itemsize == 4 else x.view(np.uint8)


def main():
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        return
    old, new = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for tag, d in (("old", old), ("new", new)):
            files.append(os.path.join(tmp, f"ab_{tag}.npz"))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d, files[-1]], check=True, cwd=ROOT)
        A, B = ({k: z[k] for k in z.files} for z in (np.load(files[0]), np.load(files[1])))
    lines = ["# tools/gpu_ab_elevation.py: two builds of libpgtt_elevation.so, every tensor of the map after each of 6 ticks, compared as int32 / uint8",
             f"# old: src={bytes(A['info']).decode()}", f"# new: src={bytes(B['info']).decode()}"]
    keys = sorted(k for k in A if k != "info")
    assert keys == sorted(k for k in B if k != "info")
    ndiff = 0
    for k in keys:
        x, y = A[k], B[k]
        same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(bits(x), bits(y))
        msg = ""
        if not same:
            ndiff += 1
            msg = "   DIFFERENT: shapes"
            if x.shape == y.shape and x.dtype == y.dtype:
                where = np.argwhere(bits(x).reshape(x.shape) != bits(y).reshape(y.shape)) if x.dtype.itemsize == 4 else np.argwhere(x != y)
                first = tuple(int(i) for i in where[0])
                msg = f"   DIFFERENT: {len(where)} of {x.size} entries, the first at (tick, env, ...) = {first}: {x[first]!r} -> {y[first]!r}"
        load = f"finite {int(np.isfinite(x).sum()):6d}" if x.dtype.kind == "f" else f"nonzero {int(np.count_nonzero(x)):5d}"      # does the buffer carry data
        lines.append(f"{k:44s} {str(x.shape):18s} {str(x.dtype):8s} {load}  bit-identical: {same}{msg}")
    lines.append(f"{len(keys)} buffers, {ndiff} different")
    lines.append("ALL BIT-IDENTICAL" if ndiff == 0 else "DIFFERENCES FOUND")
    print("\n".join(lines))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ndiff == 0 else 1)


if __name__ == "__main__":
    main()
