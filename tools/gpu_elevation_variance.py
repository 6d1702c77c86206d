"""Time, accuracy and closed loop of the variance-weighted elevation map, with the protocol of DESIGN.md 16 and the helpers of
tools/gpu_elevation_time.py: 4096 envs, level4 with per-env variants from domain_randomize(seed=0), 64x48 images of the default camera, G = 64, poses
after 40 control steps of small random actions; device events around 20 back-to-back calls after 5 warm-up calls, median [min, max] of 11 windows.

    python tools/gpu_elevation_variance.py [--out profiles/NAME.txt] [--accuracy] [--eval]

Time, in one job: pgtt_elevation (the kernel the variance tick stands next to), pgtt_elevation_var with process = 0 and with the default process
(every known cell's variance is written back), and the camera tick.
--accuracy: policy177 acting on the true observation, 1000 envs, full domain randomisation, auto-reset, the camera with relative range noise sigma =
0, 0.01 and 0.02; after 50 steps, 200 steps of RMSE of est against perceive.scan_target over the known points, per band, and the known share - for the
maximum map with alpha = 1 and alpha = 0.5 and for the variance map (elevation.VARIANCE_DEFAULTS, and with sigma_rel raised to the sensor's sigma),
all four ticked behind the same camera; and the median est_var of the variance map's known scan points whose error is above / below 2 cm.
--eval: evaluate.py --method pgtt --terrain_file level4 --policy policy177 --elevation --sensor_noise 0.02, with and without --elevation_variance."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from gpu_elevation_time import window_us  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, configs, elevation, mjcf, perceive  # noqa: E402
from phase_guided_terrain_traversal_amd.env import Joystick  # noqa: E402
from phase_guided_terrain_traversal_amd.policy import load_policy  # noqa: E402
from phase_guided_terrain_traversal_amd.randomize import domain_randomize  # noqa: E402


def accuracy(terrain, sigma, steps_warm=50, steps=200, n=1000):
    dr = domain_randomize(mjcf.load_model("stairs"), n, seed=0, terrain=terrain)
    kw = dict(params=torch.from_numpy(dr["params"]), variant=torch.from_numpy(dr["variant"]), box_friction=torch.from_numpy(dr["box_friction"]))
    env = Joystick("stairs", configs.evaluation_config("pgtt"), num_envs=n, terrain=terrain, device="cuda:0", autoreset=True,
                   depth=dict(noise=dict(sigma=sigma)) if sigma else {}, elevation=True, **kw)
    maps = {"maximum, alpha = 1": env.elevation_map,
            "maximum, alpha = 0.5": elevation.ElevationMap(env, **{**elevation.DEFAULTS, "alpha": 0.5}),
            "variance, defaults": elevation.ElevationMap(env, **elevation.DEFAULTS, variance=True)}
    if sigma > elevation.VARIANCE_DEFAULTS["sigma_rel"]:
        maps[f"variance, sigma_rel = {sigma}"] = elevation.ElevationMap(env, **elevation.DEFAULTS, variance=dict(sigma_rel=sigma))
    extra = [m for m in maps.values() if m is not env.elevation_map]
    pi = load_policy("policy177", "cuda:0")
    env.reset(0)
    for m in extra:
        m.tick(clear_all=True)
    se = {name: {k: 0.0 for k in perceive.BANDS} for name in maps}
    cnt = {name: {k: 0.0 for k in perceive.BANDS} for name in maps}
    tot = {k: 0.0 for k in perceive.BANDS}
    ev_hi, ev_lo = {name: [] for name in maps}, {name: [] for name in maps}
    with torch.no_grad():
        for t in range(steps_warm + steps):
            _, _, done, _ = env.step(pi(env.buffers["obs_state"]))
            for m in extra:
                m.tick(use_done=True)
            if t < steps_warm:
                continue
            live = (done == 0)[:, None]                                       # a done env's state rows are the new episode's: its target is not this pose's
            target = perceive.scan_target(env)
            for k, sl in perceive.BANDS.items():
                tot[k] += float(live.sum()) * (sl.stop - sl.start)
            for name, m in maps.items():
                err, known = m.est - target, (m.known > 0) & live
                for k, sl in perceive.BANDS.items():
                    se[name][k] += float((err[:, sl] ** 2 * known[:, sl]).sum()); cnt[name][k] += float(known[:, sl].sum())
                if m.variance is not None and t % 10 == 0:
                    ev_hi[name].append(m.est_var[known & (err.abs() > 0.02)].cpu()); ev_lo[name].append(m.est_var[known & (err.abs() <= 0.02)].cpu())
    lines = [f"accuracy, sensor noise sigma = {sigma}: policy177 on the true observation, {n} envs, level4, full DR, steps {steps_warm}..{steps_warm + steps}; "
             "est against perceive.scan_target over the known points: rmse m (known share) per band"]
    for name in maps:
        per = "  ".join(f"{k} {math.sqrt(se[name][k] / max(cnt[name][k], 1)):.4f} ({cnt[name][k] / max(tot[k], 1):.3f})" for k in perceive.BANDS)
        allr = math.sqrt(sum(se[name].values()) / max(sum(cnt[name].values()), 1))
        line = f"  {name:28s} {per}  all {allr:.4f}"
        if ev_hi[name]:
            hi, lo = torch.cat(ev_hi[name]), torch.cat(ev_lo[name])
            line += (f";  median est_var where |error| > 2 cm: {float(hi.median()) if hi.numel() else float('nan'):.2e} m^2 ({hi.numel()} points), "
                     f"<= 2 cm: {float(lo.median()) if lo.numel() else float('nan'):.2e} m^2 ({lo.numel()} points)")
        lines.append(line)
    for m in extra:
        m.close()
    env.close()
    return lines


def evaluation(n=1000, sigma="0.02"):
    import evaluate
    base = ["--method", "pgtt", "--policy", "policy177", "--terrain_file", "level4", "--elevation", "--sensor_noise", sigma]
    lines = [f"evaluate.py {' '.join(base)}: {n} envs, full DR, one deterministic episode"]
    for name, extra in (("maximum map (alpha = 1)", []), ("--elevation_variance", ["--elevation_variance"])):
        r = evaluate.run_evaluation(evaluate.make_parser().parse_args(base + extra), num_eval_envs=n, verbose=False)
        lines.append(f"  {name:24s} survivors {r['survivors']} / {n}, reward {r['episode_reward']:.2f}, length {r['avg_episode_length']:.1f}, "
                     f"tracking lin {r['tracking_lin_vel']:.3f} ang {r['tracking_ang_vel']:.3f}, known scan points {r['known_share']:.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--eval", action="store_true")
    args = ap.parse_args()
    n = args.num_envs
    terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
    dr = domain_randomize(mjcf.load_model("stairs"), n, seed=0, terrain=terrain)
    kw = dict(params=torch.from_numpy(dr["params"]), variant=torch.from_numpy(dr["variant"]), box_friction=torch.from_numpy(dr["box_friction"]))
    env = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", depth={}, elevation=True, **kw)
    em = env.elevation_map
    v0 = elevation.ElevationMap(env, **elevation.DEFAULTS, variance=dict(process=0.0))
    v1 = elevation.ElevationMap(env, **elevation.DEFAULTS, variance=True)
    g = torch.Generator().manual_seed(1)
    env.reset(0)
    for m in (v0, v1):
        m.tick(clear_all=True)
    for _ in range(40):
        env.step((0.2 * torch.randn(n, 12, generator=g)).clamp(-1, 1).cuda())
        for m in (v0, v1):
            m.tick(use_done=True)
    torch.cuda.synchronize()
    rows = [("pgtt_elevation, one launch", window_us(em.tick)),
            ("pgtt_elevation_var, process = 0, one launch", window_us(v0.tick)),
            (f"pgtt_elevation_var, process = {elevation.VARIANCE_DEFAULTS['process']}, one launch", window_us(v1.tick)),
            ("camera tick (force)", window_us(lambda: env.depth_camera.tick(force=True)))]
    c = em.config
    plain = n * (2 * 4 * c.grid ** 2 + 4 * c.width * c.height + 2 * 4 * c.obs_dim + 5 * abi.NSCAN)
    var = plain + n * (2 * 4 * c.grid ** 2 + 4 * abi.NSCAN)
    lines = [f"{n} envs, level4, {c.width}x{c.height}, G = {c.grid}, res = {c.res:.3f}; us per call, median [min, max] of 11 windows of 20 calls",
             f"libpgtt_elevation build: {elevation.build_info()}"]
    lines += [f"{name:60s} {m:9.1f} [{lo:.1f}, {hi:.1f}]" for name, (m, lo, hi) in rows]
    lines.append(f"pgtt_elevation_var / pgtt_elevation = {rows[1][1][0] / rows[0][1][0]:.2f} (process = 0), {rows[2][1][0] / rows[0][1][0]:.2f} (default process)")
    lines.append(f"upper bound of the HBM traffic per call (map, and var, wholly read and written): pgtt_elevation {plain / 1e6:.1f} MB -> "
                 f"{plain / rows[0][1][0] / 1e6:.2f} TB/s; pgtt_elevation_var {var / 1e6:.1f} MB -> {var / rows[2][1][0] / 1e6:.2f} TB/s at the medians; no counter run was made")
    kn = lambda m: float((m.known > 0).float().mean())
    lines.append(f"known share of the scan after 41 ticks: maximum map {kn(em):.3f}, variance map {kn(v1):.3f}")
    v0.close(); v1.close(); env.close()
    if args.accuracy:
        for sigma in (0.0, 0.01, 0.02):
            lines += accuracy(terrain, sigma)
    if args.eval:
        lines += evaluation()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
