"""A/B check of two builds of the three ray casters libpgtt_render.so, libpgtt_depth.so and libpgtt_lidar.so: the same seeded scenes, EVERY buffer
the three libraries write compared bit for bit (renderer: rgba, depth, segmentation, body_pose; depth camera: the image; LiDAR: ranges, points).
   usage: python tools/gpu_ab_raycast.py OLD_DIR NEW_DIR [--out profiles/NAME.txt]
   (OLD_DIR / NEW_DIR hold the three .so files; each build runs in its own process, render.SIDE.path / depth.SIDE.path / lidar.SIDE.path set
   before first use; libpgtt.so is the checkout's in both)
Workloads, the smallest at which these kernels can go wrong: 8 envs on level4 with domain-randomised params (the qpos0 rows) and per-env
variants, one label out of range, after 5 control steps of seeded small actions; 8 envs on flat ground without params.
Renderer: fixed / track / track_yaw views at 40x30 (partial 16x16 tiles), shadows on and off, 5 markers.  Depth camera: 24x18 and 64x48,
see_robot on and off, mounted on the torso and on a thigh, noise off and sigma = 0.02 / dropout = 0.1, every = 1.  LiDAR: spherical_pattern(32, 8)
(256 rays, one full pass of the workgroup) and a 300-ray table (a partial second pass), the same mounts, see_robot and noise settings, points on."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(lib_dir, out):
    sys.path.insert(0, ROOT)
    import torch
    from phase_guided_terrain_traversal_amd import abi, configs, depth, lidar, mjcf, render
    from phase_guided_terrain_traversal_amd.env import Joystick
    from phase_guided_terrain_traversal_amd.randomize import domain_randomize
    render.SIDE.path = os.path.join(lib_dir, "libpgtt_render.so")
    depth.SIDE.path = os.path.join(lib_dir, "libpgtt_depth.so")
    lidar.SIDE.path = os.path.join(lib_dir, "libpgtt_lidar.so")
    res = {f"info/{m.SIDE.prefix[5:]}": np.frombuffer(m.build_info()["src"].encode(), np.uint8) for m in (render, depth, lidar)}
    n = 8
    for wl in ("level4", "flat"):
        if wl == "level4":
            terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
            dr = domain_randomize(mjcf.load_model("stairs"), n, seed=3, terrain=terrain)
            env = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", variant=torch.from_numpy(dr["variant"]),
                           params=torch.from_numpy(dr["params"]), box_friction=torch.from_numpy(dr["box_friction"]))
        else:
            terrain = None
            env = Joystick("flat_terrain", configs.training_config(), num_envs=n, device="cuda:0")
        env.reset(seed=4)
        g = torch.Generator(device="cuda").manual_seed(7)
        for _ in range(5):
            env.step(torch.tanh(torch.randn(n, 12, device="cuda", generator=g) * 0.3))
        if terrain is not None:
            env.buffers["variant"][n - 1] = terrain.shape[0] + 5          # edited after the last step: both libraries clamp it to T - 1
        torch.cuda.synchronize()
        res[f"{wl}/state"] = env.buffers["state"].cpu().numpy()           # the input: equal by construction, compared all the same
        # renderer: 3 camera modes x 8 envs in one call, 5 markers per view
        cams = [render.Camera(mode, target=(0.3, 0.0, 0.2) if mode == "fixed" else (0.0, 0.0, 0.0), distance=2.0, azimuth=100.0 + 7 * k, elevation=-20.0)
                for k, mode in enumerate(("fixed", "track", "track_yaw"))]
        ids = [e for _ in cams for e in range(n)]
        per_view = [c for c in cams for _ in range(n)]
        base = env.buffers["state"][abi.S_QPOS:abi.S_QPOS + 3].T[ids]                            # [V, 3]
        off = torch.tensor([[0.3, 0.0, 0.1], [-0.2, 0.2, 0.0], [0.0, -0.3, 0.2], [0.5, 0.1, -0.1], [0.1, 0.1, 0.3]], device="cuda")
        markers = torch.cat([base[:, None, :] + off[None], torch.full((len(ids), 5, 1), 0.04, device="cuda")], -1)
        for shadows in (True, False):
            r = render.Renderer(env, 40, 30, shadows=shadows)
            o = r.render(ids, camera=per_view, markers=markers, depth=True, segmentation=True, body_pose=True)
            torch.cuda.synchronize()
            for k in ("rgba", "depth", "segmentation", "body_pose"):
                res[f"{wl}/render_shadows{int(shadows)}/{k}"] = o[k].cpu().numpy()
            r.close()
        # depth camera
        mounts = {"torso": dict(mount_body=0, mount_pos=(0.30, 0.0, 0.05), pitch_deg=30.0),
                  "thigh": dict(mount_body=2, mount_pos=(0.0, 0.06, -0.1), mount_quat=(1.0, 0.0, 0.0, 0.0))}
        for (W, H) in ((24, 18), (64, 48)):
            for see in (True, False):
                for mname, mount in mounts.items():
                    for noise in (None, dict(sigma=0.02, dropout=0.1, seed=11)):
                        cam = depth.DepthCamera(env, **depth.settings(dict(width=W, height=H, see_robot=see, noise=noise, every=1, **mount)))
                        img = cam.tick().clone()
                        img2 = cam.tick().clone()                          # counter = 1: other noise draws
                        torch.cuda.synchronize()
                        tag = f"{wl}/depth_{W}x{H}_robot{int(see)}_{mname}_noise{int(noise is not None)}"
                        res[tag + "/tick0"], res[tag + "/tick1"] = img.cpu().numpy(), img2.cpu().numpy()
                        cam.close()
        # LiDAR
        for pname, pattern in (("256", lidar.spherical_pattern(32, 8)), ("300", lidar.spherical_pattern(30, 10, (-180, 180), (-80, 25)))):
            for see in (True, False):
                for mname, mount in mounts.items():
                    for noise in (None, dict(sigma=0.02, dropout=0.1, seed=11)):
                        place = dict(mount_body=mount["mount_body"], mount_pos=mount["mount_pos"], mount_quat=depth.pitch_quat(mount.get("pitch_deg", 0.0)))
                        lid = lidar.LidarScanner(env, **lidar.settings(dict(pattern=pattern, see_robot=see, noise=noise, every=1, **place)), points=True)
                        tag = f"{wl}/lidar_{pname}_robot{int(see)}_{mname}_noise{int(noise is not None)}"
                        for tick in (0, 1):                                # counter = 1: other noise draws
                            lid.tick()
                            torch.cuda.synchronize()
                            res[f"{tag}/tick{tick}/ranges"], res[f"{tag}/tick{tick}/points"] = lid.ranges.cpu().numpy(), lid.points.cpu().numpy()
                        lid.close()
        env.close()
    np.savez(out, **res)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint8) if x.dtype.itemsize != 4 else x.view(np.uint32)


def main():
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        return
    old, new = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    tmp = tempfile.mkdtemp()
    files = []
    for tag, d in (("old", old), ("new", new)):
        files.append(os.path.join(tmp, f"ab_{tag}.npz"))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d, files[-1]], check=True, cwd=ROOT)
    A, B = np.load(files[0]), np.load(files[1])
    lines = ["# tools/gpu_ab_raycast.py: two builds of libpgtt_render.so / libpgtt_depth.so / libpgtt_lidar.so, every output buffer compared as uint32 / uint8"]
    lines += [f"# {tag}: " + " ".join(f"{k} src={bytes(X['info/' + k]).decode()}" for k in ("render", "depth", "lidar")) for tag, X in (("old", A), ("new", B))]
    keys = sorted(k for k in A.files if not k.startswith("info/"))
    assert keys == sorted(k for k in B.files if not k.startswith("info/"))
    ndiff = 0
    for k in keys:
        x, y = A[k], B[k]
        same = x.shape == y.shape and np.array_equal(bits(x), bits(y))
        msg = ""
        if not same:
            ndiff += 1
            with np.errstate(invalid="ignore"):
                d = np.abs(x.astype(np.float64) - y.astype(np.float64)) if x.shape == y.shape else np.array([np.inf])
            msg = f"   DIFFERENT: max |diff| {np.nanmax(d):.3g}, {int((bits(x) != bits(y)).sum()) if x.shape == y.shape else -1} of {x.size} entries"
        lines.append(f"{k:58s} {str(x.shape):18s} bit-identical: {same}{msg}")
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
