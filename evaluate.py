"""CLI mirror of the reference's training/evaluate.py:103-301: take a trained policy, run the evaluator's rollout on one terrain file and
report how many of the evaluation envs get through the episode.

    python evaluate.py --method pgtt --terrain_file level10 --checkpoint_folder checks_stairs/checkpoint_1
    python evaluate.py --method pgtt --terrain_file level13 --policy policy177          (a shipped reference-trained policy)

What the reference does there (training/evaluate.py:133-259): it re-enters Brax's `ppo.train` with `num_timesteps = 1` from a checkpoint
only to harvest the evaluator's metrics - `num_eval_envs = 1000` envs (:151) of the same task with the same domain randomisation,
one episode of `episode_length` control steps under the DETERMINISTIC policy (the mode of the tanh-normal head), statistics of each
env's FIRST episode [UPSTREAM-RECALL: brax.training.acting.Evaluator + envs.training.EvalWrapper] - and returns the number of envs whose
final `termination` reward term is zero (:221-223), i.e. the robots that did not fall.  Here the same rollout runs directly: no learner
is built.  The policy comes from `--checkpoint_folder` (the newest `<env_steps>.pt` of `train.py`, or its `policy<index>.npz`) or from
`--policy` (an .npz path or the name of a shipped policy); with `--student student.npz` (train_student.py) the policy acts on the observation
whose scan rows the student perception module estimated from the onboard depth image, with `--elevation [grid,res,alpha]` on the observation whose
scan rows are sampled from the depth-fused elevation map (elevation.py; nothing to train; `--elevation_source lidar` fuses it from the onboard
LiDAR's points instead, lidar.py; `--elevation_fill [K]` closes the map's holes first and the policy acts on the filled scan; `--sensor_every M`
runs that sensor at one control step in M and lets the map follow it; `--sensor_latency LO[,HI]` fuses every frame LO steps after it was taken, under
the pose of its capture (LO,HI: drawn per env per episode); `--odometry_drift [sigma_xy,sigma_z,sigma_yaw,yaw_bias,scale]` registers the map
with a dead-reckoned pose that drifts, and adds a line with the drift at the end; `--elevation_visibility [margin,end_guard,stride]` cleans the map by
visibility in front of every tick and adds a line with the cells forgotten per step; `--elevation_variance [sigma0,sigma_rel,process,gate,band]` fuses the map by
the variance-weighted update; `--sensor_noise SIGMA[,DROPOUT]` gives the sensor that feeds the map or the student range noise); a `--policy` file that holds a recurrent policy
(train_distill.py --memory, recurrent_policy.py) is stepped with a memory per env, cleared where the previous step ended an episode; the remaining flags of the reference's CLI are accepted and ignored.
"""
import argparse
import os

import numpy as np
import torch

from phase_guided_terrain_traversal_amd import abi, configs, mjcf, ppo
from phase_guided_terrain_traversal_amd.env import Joystick
from phase_guided_terrain_traversal_amd.policy import PolicyMLP, _DIR as POLICY_DIR
from phase_guided_terrain_traversal_amd.randomize import domain_randomize

ROOT = os.path.dirname(os.path.abspath(__file__))
DEVICE = "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0"))
NUM_EVAL_ENVS = 1000                                              # training/evaluate.py:151


def load_terrain(spec):
    p = spec if os.path.exists(spec) else os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains",
                                                       os.path.basename(spec).replace(".npy", "") + ".npy")
    return np.load(p)


def recurrent_file(path):
    """does the .npz hold a recurrent policy (train_distill.py --memory: gru_w_ih next to the feed-forward keys)?"""
    with np.load(path) as d:
        return "gru_w_ih" in d.files


def load_policy_from_args(args, tmp_dir):
    """-> PolicyMLP on DEVICE (a recurrent_policy.RecurrentPolicy for a file that holds one)"""
    if args.policy:
        p = args.policy if os.path.exists(args.policy) else os.path.join(POLICY_DIR, args.policy.replace(".npz", "") + ".npz")
        if recurrent_file(p):
            from phase_guided_terrain_traversal_amd.recurrent_policy import RecurrentPolicy
            return RecurrentPolicy.load(p).to(DEVICE)
        return PolicyMLP(p).to(DEVICE)
    if not args.checkpoint_folder:
        raise SystemExit("give --checkpoint_folder (a train.py checkpoint directory) or --policy")
    steps = [int(f[:-3]) for f in os.listdir(args.checkpoint_folder) if f.endswith(".pt") and f[:-3].isdigit()]
    if steps:                                                     # get_max_numbered_folder, training/evaluate.py:262-272
        ck = torch.load(os.path.join(args.checkpoint_folder, f"{max(steps)}.pt"), map_location="cpu")
        out = os.path.join(tmp_dir, "eval_policy.npz")
        ppo.export_policy_npz(ck, out)
        print(f"Restoring from checkpoint: {os.path.join(args.checkpoint_folder, str(max(steps)))}.pt")
        return PolicyMLP(out).to(DEVICE)
    npz = sorted(f for f in os.listdir(args.checkpoint_folder) if f.startswith("policy") and f.endswith(".npz"))
    if not npz:
        raise SystemExit(f"no <env_steps>.pt or policy*.npz in {args.checkpoint_folder}")
    return PolicyMLP(os.path.join(args.checkpoint_folder, npz[-1])).to(DEVICE)


def resize_nearest(img, height, width):
    """[..., H, W] -> [..., height, width]: output pixel (i, j) takes the input pixel under its centre"""
    H, W = img.shape[-2:]
    rows = ((torch.arange(height, device=img.device) * 2 + 1) * H) // (2 * height)
    cols = ((torch.arange(width, device=img.device) * 2 + 1) * W) // (2 * width)
    return img[..., rows[:, None], cols[None, :]]


class VideoRecorder:
    """--video: renders the first --video_envs evaluation envs with a tracking camera before every --video_every-th control step (frames stay
    on the device: [H, K * W, 3] per frame, the envs side by side, a progress bar of the episode along the bottom rows) and writes them at
    the end (render.save_gif: a GIF, or a PNG sequence where PIL is missing).  Only reads the env."""

    def __init__(self, args, env, episode_length):
        from phase_guided_terrain_traversal_amd.render import Camera, Renderer
        w, h = (int(x) for x in args.video_size.lower().split("x"))
        self.env, self.path, self.every, self.L = env, args.video, max(1, int(args.video_every)), episode_length
        self.ids = list(range(min(int(args.video_envs), env.num_envs)))
        self.scan = bool(args.video_scan)
        self.renderer = Renderer(env, w, h, shadows=True)
        self.camera = Camera("track", target=(0.0, 0.0, 0.0), distance=2.2, azimuth=120.0, elevation=-25.0, fovy=45.0)
        self.frames = []
        self.depth = None
        # --video_elevation MODE: a second tile beside each env's RGB tile, the elevation map drawn from the same camera (Renderer.render_map)
        self.elevation = getattr(args, "video_elevation", None)
        if self.elevation is not None:
            em = env.elevation_map
            if em is None:
                raise SystemExit("--video_elevation draws --elevation's map: give --elevation too")
            if self.elevation == "var" and em.variance is None:
                raise SystemExit("--video_elevation var draws the variance layer: give --elevation_variance too")
            if self.elevation == "filled" and not em.dense:
                raise SystemExit("--video_elevation filled draws the filled map: give --elevation_fill too")
        if getattr(args, "video_depth", False):
            # --video_depth: each env's onboard depth image (the sensor of depth.DEFAULTS, resolution included), grey, scaled to the tile by
            # nearest neighbour and put under its RGB tile
            from phase_guided_terrain_traversal_amd.depth import DepthCamera, settings
            self.depth = DepthCamera(env, **settings())

    def capture(self, t):
        if t % self.every:
            return
        from phase_guided_terrain_traversal_amd.render import scan_points
        markers = None
        if self.scan:
            p = scan_points(self.env, self.ids)
            markers = torch.cat([p, torch.full_like(p[..., :1], 0.012)], -1)
        rgb = self.renderer.render(self.ids, camera=self.camera, markers=markers)["rgb"]
        if self.elevation is not None:
            # height: the belief view; var / filled: tinted by the variance layer / by the pass that filled the cell; overlay: over the true terrain
            kw = {"height": {}, "var": dict(tint="var"), "filled": dict(tint="dist"), "overlay": dict(terrain=True)}[self.elevation]
            belief = self.renderer.render_map(self.ids, self.env.elevation_map, camera=self.camera, markers=markers, **kw)["rgb"]
            rgb = torch.stack([rgb, belief], 1).flatten(0, 1)
        v, h, w, _ = rgb.shape
        frame = rgb.permute(1, 0, 2, 3).reshape(h, v * w, 3).clone()
        bar = max(1, h // 80)
        frame[h - bar:, : int(round(v * w * (t + 1) / self.L))] = 255
        if self.depth is not None:
            d = self.depth.tick(force=True)[self.ids]
            grey = (255 * (1 - (d - self.depth.near) / (self.depth.far - self.depth.near))).clamp(0, 255).to(torch.uint8)
            grey = resize_nearest(grey, h, w * (v // len(self.ids)))             # under the env's tiles, however many it has
            frame = torch.cat([frame, grey.permute(1, 0, 2).reshape(h, v * w, 1).expand(h, v * w, 3)], 0)
        self.frames.append(frame)

    def write(self, verbose=True):
        from phase_guided_terrain_traversal_amd.render import save_gif
        frames = torch.stack(self.frames).cpu().numpy()
        d = os.path.dirname(os.path.abspath(self.path))
        os.makedirs(d, exist_ok=True)
        out = save_gif(self.path, frames, fps=1.0 / (self.env.dt * self.every))
        self.renderer.close()
        if self.depth is not None:
            self.depth.close()
        if verbose:
            print(f"video: {len(frames)} frames of {frames.shape[2]}x{frames.shape[1]} -> {out}")
        return out


def sensor_kwargs(args):
    """the Joystick keywords of the sensor flags (--student, --elevation and what goes with it, --sensor_noise, --sensor_every): what the policy
    is to act on and the sensors that deliver it; {} when none is given.  train_distill.py builds its env from the same flags"""
    kw = {}
    # --sensor_noise SIGMA[,DROPOUT]: the sensor that feeds the student or the map reads noisy ranges (the sensors' noise=dict(sigma, dropout):
    # relative range noise and the probability of a `far` reading); without it they are exact
    noisy = sensor_noise(getattr(args, "sensor_noise", None))
    if getattr(args, "student", None):
        # --student: the policy acts on env.student_obs - the observation whose scan rows a perceive.ScanEstimator estimated from the onboard
        # depth image (the camera of depth.DEFAULTS) - instead of the privileged scan
        kw.update(depth=dict(noisy), student=args.student)
    elev = getattr(args, "elevation", None)
    if getattr(args, "video_elevation", None) is not None:
        if elev is None:
            raise SystemExit("--video_elevation draws --elevation's map beside the scene: give --elevation too")
        if not getattr(args, "video", None):
            raise SystemExit("--video_elevation adds a tile to --video's frames: give --video too")
        if args.video_elevation == "var" and getattr(args, "elevation_variance", None) is None:
            raise SystemExit("--video_elevation var draws the variance layer: give --elevation_variance too")
        if args.video_elevation == "filled" and getattr(args, "elevation_fill", None) is None:
            raise SystemExit("--video_elevation filled draws the filled map: give --elevation_fill too")
    if noisy and elev is None and not getattr(args, "student", None):
        raise SystemExit("--sensor_noise is the noise of the sensor that feeds --elevation's map or --student: give one of them too")
    if getattr(args, "elevation_variance", None) is not None and elev is None:
        raise SystemExit("--elevation_variance says how --elevation's map is fused: give --elevation too")
    if getattr(args, "odometry_drift", None) is not None and elev is None:
        raise SystemExit("--odometry_drift is the drift of the pose --elevation's map is registered with: give --elevation too")
    if getattr(args, "elevation_visibility", None) is not None and elev is None:
        raise SystemExit("--elevation_visibility cleans --elevation's map: give --elevation too")
    if elev is not None:
        # --elevation [grid,res,alpha]: the policy acts on env.elevation_obs - the observation whose scan rows are sampled from the elevation map
        # fused from the onboard depth image (the camera of depth.DEFAULTS; elevation.DEFAULTS where a value is not given)
        if getattr(args, "student", None):
            raise SystemExit("--student and --elevation both say what the policy acts on: give one")
        vals = [v for v in elev.split(",") if v]
        if len(vals) > 3:
            raise SystemExit("--elevation takes at most grid,res,alpha")
        try:
            given = dict(zip(("grid", "res", "alpha"), (int(vals[0]),) + tuple(float(v) for v in vals[1:]))) if vals else True
        except ValueError:
            raise SystemExit(f"--elevation {elev}: grid must be an integer, res and alpha numbers")
        fill = getattr(args, "elevation_fill", None)
        if fill is not None:
            # --elevation_fill [K]: the map's holes are closed behind every tick (K passes, 16 unless given) and the policy acts on
            # env.elevation_filled_obs, the observation whose scan rows are sampled from the filled map
            if fill is not True and not 1 <= fill <= 95:                 # a caller that built the namespace without the parser
                raise SystemExit(f"--elevation_fill {fill}: the number of passes must be in [1, 95]")
            given = dict({} if given is True else given, fill=fill)
            if getattr(args, "video_elevation", None) == "filled":
                given["dense"] = True                                      # the video draws the filled map itself, so the fill keeps it
        source = getattr(args, "elevation_source", "depth")
        # --sensor_every M: the sensor that feeds the map takes new data at one control step in M; for M > 1 the map follows it (follow_sensor):
        # it fuses on those steps and in between samples the held map at the current pose
        every = int(getattr(args, "sensor_every", 1))
        if every < 1:
            raise SystemExit(f"--sensor_every {every}: the sensor's period must be >= 1")
        sensor = dict(noisy) if every == 1 else dict(noisy, every=every)
        if every > 1:
            given = dict({} if given is True else given, follow_sensor=True)
        variance = elevation_variance(getattr(args, "elevation_variance", None))
        if variance is not None:
            # --elevation_variance [sigma0,sigma_rel,process,gate,band]: the map is fused by the variance-weighted update (elevation.VARIANCE_DEFAULTS
            # where a value is not given) instead of the maximum and alpha
            if every > 1:
                raise SystemExit("--elevation_variance behind a slower sensor (--sensor_every > 1) is not built yet")
            given = dict({} if given is True else given, variance=variance)
        drift = odometry_drift(getattr(args, "odometry_drift", None))
        if drift is not None:
            # --odometry_drift [sigma_xy,sigma_z,sigma_yaw,yaw_bias,scale]: the map is registered with a dead-reckoned pose that drifts
            # (elevation.ODOMETRY_DEFAULTS where a value is not given) instead of the simulator's exact one
            given = dict({} if given is True else given, odometry=drift)
        vis = elevation_visibility(getattr(args, "elevation_visibility", None))
        if vis is not None:
            # --elevation_visibility [margin,end_guard,stride]: the map is cleaned by visibility in front of every tick
            # (elevation.VISIBILITY_DEFAULTS where a value is not given)
            if every > 1:
                raise SystemExit("--elevation_visibility behind a slower sensor (--sensor_every > 1) is not built: a hold step must not clean with a stale image")
            given = dict({} if given is True else given, visibility=vis)
        lat = sensor_latency(getattr(args, "sensor_latency", None))
        if lat is not None:
            # --sensor_latency LO[,HI]: every frame is fused LO control steps after it was taken, under the pose of its capture; with HI the latency
            # is drawn per env per episode in [LO, HI]
            for flag, on in (("--sensor_every > 1", every > 1), ("--elevation_variance", variance is not None), ("--elevation_visibility", vis is not None)):
                if on:
                    raise SystemExit(f"--sensor_latency with {flag} is not built")
            given = dict({} if given is True else given, latency=lat)
        if source == "lidar":
            # --elevation_source lidar: the map is fused from the world points of the onboard LiDAR (lidar.DEFAULTS), as the deployed mapping stack's is
            kw.update(lidar=sensor, elevation=dict({} if given is True else given, source="lidar"))
        else:
            kw.update(depth=sensor, elevation=given)
    elif getattr(args, "elevation_source", "depth") != "depth":
        raise SystemExit("--elevation_source says what --elevation is fused from: give --elevation too")
    elif getattr(args, "elevation_fill", None) is not None:
        raise SystemExit("--elevation_fill fills the holes of --elevation's map: give --elevation too")
    elif int(getattr(args, "sensor_every", 1)) != 1:
        raise SystemExit("--sensor_every is the period of the sensor that feeds --elevation's map: give --elevation too")
    elif getattr(args, "sensor_latency", None) is not None:
        raise SystemExit("--sensor_latency is the latency of the sensor that feeds --elevation's map: give --elevation too")
    return kw


def run_evaluation(args, num_eval_envs=NUM_EVAL_ENVS, seed=0, verbose=True):
    """-> dict(survivors, num_eval_envs, episode_reward, avg_episode_length, tracking_lin_vel, tracking_ang_vel)"""
    if args.method not in ("pgtt", "baseline"):
        raise SystemExit("--method must be pgtt (go2/joystick_pgtt.py) or baseline (go2/joystick.py)")
    cfg = configs.evaluation_config(args.method)          # training/evaluate.py:127-129: commands within +-[0.4, 0.4, 0.7]
    model = mjcf.load_model(args.task_name)
    terrain = load_terrain(args.terrain_file) if args.task_name == "stairs" else None
    n = num_eval_envs
    level_start = None
    if args.task_name == "stairs" and getattr(args, "terrain_files", None):
        # the stacked table of a curriculum run, evaluated on ONE fixed level of it (--level), the curriculum off
        from phase_guided_terrain_traversal_amd.curriculum import stack_levels
        terrain, level_start = stack_levels([load_terrain(f) for f in args.terrain_files.split(",")])
    dr = domain_randomize(model, n, seed=seed, terrain=terrain, level_start=level_start,      # the evaluator's env gets the same randomization_fn
                          init_level=int(getattr(args, "level", 0)))
    kw = {"params": torch.from_numpy(dr["params"])}
    if terrain is not None:
        kw.update(variant=torch.from_numpy(dr["variant"]), box_friction=torch.from_numpy(dr["box_friction"]))
    push = configs.push_from_args(args)                           # --push_*: random kicks of the torso (off unless one is given)
    if push is not None:
        kw["push"] = push
    kw.update(sensor_kwargs(args))
    env = Joystick(args.task_name, cfg, num_envs=n, terrain=terrain, device=DEVICE, autoreset=True, **kw)
    if env.elevation_filled_obs is not None:
        acts_on = env.elevation_filled_obs
    elif env.elevation_map is not None:
        acts_on = env.elevation_obs
    elif env.student is not None:
        acts_on = env.student_obs
    else:
        acts_on = env.buffers["obs_state"]
    tmp = os.path.join(ROOT, "plots"); os.makedirs(tmp, exist_ok=True)
    pi = load_policy_from_args(args, tmp)
    if pi.mean.shape[0] != env.observation_size["state"]:
        raise SystemExit(f"the policy reads {pi.mean.shape[0]} observations, the {args.method} task gives {env.observation_size['state']}")
    L = cfg["episode_length"]
    env.reset(seed=seed)
    dev = env.device
    first = torch.ones(n, dtype=torch.bool, device=dev)                           # still inside its first episode
    ret = torch.zeros(n, device=dev); length = torch.zeros(n, device=dev); fell = torch.zeros(n, dtype=torch.bool, device=dev)
    terms = torch.zeros(abi.NMETRIC, n, device=dev)
    known = torch.zeros(n, device=dev)                                            # with a map: the scan points it knew, summed over the first episode
    covered = torch.zeros(n, device=dev)                                          # with a fill: the scan points it knew or filled
    drift = torch.zeros(n, 4, device=dev)                                         # with odometry drift: the error when the first episode ended
    forgot = torch.zeros(n, device=dev)                                           # with visibility clean-up: the cells forgotten, summed over the first episode
    video = VideoRecorder(args, env, L) if getattr(args, "video", None) else None
    recurrent = hasattr(pi, "gru_w_ih")
    if recurrent:
        # a recurrent policy: a [n, R] memory that starts at zero and is cleared for the envs whose previous step ended an episode
        memory, ended = torch.zeros(n, pi.memory, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
        pi.requires_grad_(False)
    for t in range(L):
        if video is not None:
            video.capture(t)
        if env.elevation_map is not None:
            known += env.elevation_known.float().mean(1) * first.float()
        if env.elevation_dist is not None:
            covered += (env.elevation_dist != 255).float().mean(1) * first.float()
        if env.elevation_cleared is not None:
            forgot += env.elevation_cleared.float() * first.float()
        if env.odometry_error is not None:
            # the step that ends an episode clears the env's estimate: keep the error as it stood before that step
            drift = torch.where(first[:, None], env.odometry_error, drift)
        if recurrent:
            action, _, memory = pi.step(acts_on, memory, ended)
            _, reward, done, info = env.step(action)
            ended = done > 0
        else:
            _, reward, done, info = env.step(pi(acts_on))
        w = first.float()
        ret += reward * w; length += w; terms += info["metrics"] * w
        d = done > 0
        fell |= first & d & (env.buffers["frame"][abi.F_UPVECTOR + 2] < 0)
        first &= ~d
    survivors = int((~fell).sum())
    i_lin, i_ang = abi.REWARD_KEYS.index("tracking_lin_vel"), abi.REWARD_KEYS.index("tracking_ang_vel")
    sc = cfg["reward_config"]["scales"]
    out = {"survivors": survivors, "num_eval_envs": n, "episode_reward": float(ret.mean()), "avg_episode_length": float(length.mean()),
           "tracking_lin_vel": float(terms[i_lin].mean()) / (sc["tracking_lin_vel"] * L), "tracking_ang_vel": float(terms[i_ang].mean()) / (sc["tracking_ang_vel"] * L)}
    if env.elevation_map is not None:
        out["known_share"] = float((known / length.clamp(min=1)).mean())          # mean share of the 117 scan points the map knew when the policy acted
    if env.elevation_dist is not None:
        out["covered_share"] = float((covered / length.clamp(min=1)).mean())      # ... that the map knew or the fill reached (dist != 255)
    if env.odometry_error is not None:                                             # at the end of the run: of each env's first episode, before its last step
        out["odometry_e_xy"], out["odometry_psi"] = float(drift[:, :2].norm(dim=1).mean()), float(drift[:, 3].abs().mean())
    if env.elevation_cleared is not None:                                          # cells the clean-up forgot per env and step of the first episode
        out["visibility_cleared_per_step"] = float((forgot / length.clamp(min=1)).mean())
    if video is not None:
        out["video"] = video.write(verbose)
    env.close()
    if verbose:                                                                    # training/evaluate.py:212,226
        print(out["episode_reward"])
        print([survivors])
        if "odometry_e_xy" in out:
            print(f"odometry drift at the end: mean |e_xy| = {out['odometry_e_xy']:.4f} m, mean |psi| = {out['odometry_psi']:.4f} rad")
        if "visibility_cleared_per_step" in out:
            print(f"visibility clean-up: {out['visibility_cleared_per_step']:.3f} cells forgotten per env and step")
    return out


def run_training(args):
    """the name evaluate_multiple.py imports (training/evaluate_multiple.py:7): number of evaluation envs that did not fall"""
    return run_evaluation(args)["survivors"]


def sensor_noise(text):
    """--sensor_noise SIGMA[,DROPOUT] -> {} (not given) or dict(noise=dict(sigma=..., dropout=...)), the sensors' keyword"""
    if text is None:
        return {}
    vals = [v for v in str(text).split(",") if v]
    try:
        nums = [float(v) for v in vals]
    except ValueError:
        nums = []
    if not 1 <= len(nums) <= 2 or nums[0] < 0 or not 0 <= (nums[1] if len(nums) > 1 else 0.0) < 1:
        raise SystemExit(f"--sensor_noise {text}: give SIGMA[,DROPOUT] with SIGMA >= 0 and 0 <= DROPOUT < 1")
    return dict(noise=dict(sigma=nums[0], dropout=nums[1] if len(nums) > 1 else 0.0))


def elevation_variance(text):
    """--elevation_variance [sigma0,sigma_rel,process,gate,band] -> None (not given), True (the flag alone) or a dict of the values given"""
    if text is None:
        return None
    vals = [v for v in str(text).split(",") if v]
    names = ("sigma0", "sigma_rel", "process", "gate", "band")
    if len(vals) > len(names):
        raise SystemExit("--elevation_variance takes at most sigma0,sigma_rel,process,gate,band")
    try:
        return dict(zip(names, (float(v) for v in vals))) if vals else True
    except ValueError:
        raise SystemExit(f"--elevation_variance {text}: the values must be numbers")


def odometry_drift(text):
    """--odometry_drift [sigma_xy,sigma_z,sigma_yaw,yaw_bias,scale] -> None (not given), True (the flag alone) or a dict of the values given"""
    if text is None:
        return None
    vals = [v for v in str(text).split(",") if v]
    names = ("sigma_xy", "sigma_z", "sigma_yaw", "yaw_bias", "scale")
    if len(vals) > len(names):
        raise SystemExit("--odometry_drift takes at most sigma_xy,sigma_z,sigma_yaw,yaw_bias,scale")
    try:
        return dict(zip(names, (float(v) for v in vals))) if vals else True
    except ValueError:
        raise SystemExit(f"--odometry_drift {text}: the values must be numbers")


def elevation_visibility(text):
    """--elevation_visibility [margin,end_guard,stride] -> None (not given), True (the flag alone) or a dict of the values given"""
    if text is None:
        return None
    vals = [v for v in str(text).split(",") if v]
    if len(vals) > 3:
        raise SystemExit("--elevation_visibility takes at most margin,end_guard,stride")
    try:
        return dict(zip(("margin", "end_guard", "stride"), [float(v) for v in vals[:2]] + [int(v) for v in vals[2:]])) if vals else True
    except ValueError:
        raise SystemExit(f"--elevation_visibility {text}: margin and end_guard must be numbers, stride an integer")


def sensor_latency(text):
    """--sensor_latency LO[,HI] -> None (not given) or the pair (LO, HI) of control steps, HI = LO unless given, 0 <= LO <= HI <= 8
    (elevation.MAX_LATENCY)"""
    if text is None:
        return None
    vals = [v for v in str(text).split(",") if v]
    try:
        ticks = [int(v) for v in vals]
    except ValueError:
        ticks = []
    if len(ticks) not in (1, 2) or len(ticks) != len(vals):
        raise SystemExit(f"--sensor_latency {text}: give LO or LO,HI, whole numbers of control steps")
    lo, hi = ticks[0], ticks[-1]
    if not 0 <= lo <= hi <= 8:
        raise SystemExit(f"--sensor_latency {text}: need 0 <= LO <= HI <= 8")
    return (lo, hi)


def fill_passes(text):
    """--elevation_fill K: an integer in [1, 95] (elevation.MAX_FILL); the flag without a value is True, elevation.FILL_PASSES"""
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a number of passes")
    if not 1 <= k <= 95:
        raise argparse.ArgumentTypeError(f"the number of passes must be in [1, 95], not {k}")
    return k


def add_sensor_args(ap):
    """the flags sensor_kwargs reads"""
    ap.add_argument("--student", type=str, default=None, help="a student.npz of train_student.py: the policy acts on the depth camera's estimate of the scan rows")
    ap.add_argument("--elevation", type=str, nargs="?", const="", default=None, metavar="GRID,RES,ALPHA",
                    help="the policy acts on the scan rows sampled from the depth-fused elevation map (elevation.py); optional grid[,res[,alpha]]")
    ap.add_argument("--elevation_source", type=str, default="depth", choices=("depth", "lidar"),
                    help="with --elevation: fuse the map from the depth camera's image (default) or from the onboard LiDAR's points (lidar.py)")
    ap.add_argument("--elevation_fill", type=fill_passes, nargs="?", const=True, default=None, metavar="K",
                    help="with --elevation: close the map's holes with K passes (16 unless given) behind every tick; the policy acts on the filled scan")
    ap.add_argument("--elevation_variance", type=str, nargs="?", const="", default=None, metavar="SIGMA0,SIGMA_REL,PROCESS,GATE,BAND",
                    help="with --elevation: fuse the map by the variance-weighted (Kalman) update instead of the maximum and alpha; optional settings")
    ap.add_argument("--odometry_drift", type=str, nargs="?", const="", default=None, metavar="SIGMA_XY,SIGMA_Z,SIGMA_YAW,YAW_BIAS,SCALE",
                    help="with --elevation: register the map with a dead-reckoned pose that drifts in x, y, z and yaw, not with the exact one; optional settings")
    ap.add_argument("--elevation_visibility", type=str, nargs="?", const="", default=None, metavar="MARGIN,END_GUARD,STRIDE",
                    help="with --elevation: clean the map by visibility in front of every tick (a cell a ray passed below is forgotten); optional settings")
    ap.add_argument("--sensor_noise", type=str, default=None, metavar="SIGMA[,DROPOUT]",
                    help="with --elevation or --student: relative range noise and dropout probability of the sensor that feeds it")
    ap.add_argument("--sensor_every", type=int, default=1, metavar="M",
                    help="with --elevation: the sensor that feeds the map runs at one control step in M; for M > 1 the map follows it, holding in between")
    ap.add_argument("--sensor_latency", type=str, default=None, metavar="LO[,HI]",
                    help="with --elevation: a frame is fused LO control steps after it was taken, under the pose of its capture; LO,HI draws it per env per episode")


def make_parser():
    ap = argparse.ArgumentParser(description="Evaluate a trained policy on one terrain file (MI355X-native PGTT env)")
    ap.add_argument("--method", type=str, default="pgtt")
    ap.add_argument("--task_name", type=str, default="stairs")
    ap.add_argument("--terrain_file", type=str, default="terrains/level1.npy")
    ap.add_argument("--checkpoint_folder", type=str, default=None)
    ap.add_argument("--policy", type=str, default=None, help="an exported policy (.npz path, or the name of a shipped one: policy177, policy175, policy3)")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--discount", type=float, default=0.97)
    ap.add_argument("--learning_rate", type=float, default=3e-4)
    ap.add_argument("--num_minibatches", type=int, default=32)
    ap.add_argument("--num_timesteps", type=int, default=1)
    ap.add_argument("--num_evals", type=int, default=2)
    ap.add_argument("--index", type=int, default=32)
    ap.add_argument("--video", type=str, default=None, help="write a rollout video of the first --video_envs envs here (.gif; a PNG sequence where PIL is missing)")
    ap.add_argument("--video_envs", type=int, default=4)
    ap.add_argument("--video_size", type=str, default="320x240", help="WxH of each env's tile")
    ap.add_argument("--video_every", type=int, default=2, help="one frame every n control steps")
    ap.add_argument("--video_scan", action="store_true", help="overlay the 117 height-scan hits as marker spheres")
    ap.add_argument("--video_depth", action="store_true", help="tile each video env's onboard depth image (grey, near = white) under its RGB tile")
    ap.add_argument("--video_elevation", type=str, nargs="?", const="height", default=None, choices=("height", "var", "filled", "overlay"),
                    help="with --video and --elevation: tile the elevation map, drawn from the same camera, beside each env's RGB tile: coloured by "
                         "height (default), by variance (needs --elevation_variance), the filled map by fill pass (needs --elevation_fill), or "
                         "lifted 1 cm over the true terrain")
    add_sensor_args(ap)
    configs.add_push_args(ap)
    ap.add_argument("--terrain_files", type=str, default=None, help="comma-separated level files stacked into one table (as train.py --terrain_files); evaluated on --level")
    ap.add_argument("--level", type=int, default=0, help="with --terrain_files: the level every evaluation env stands on (no curriculum at evaluation)")
    return ap


if __name__ == "__main__":
    r = run_evaluation(make_parser().parse_args())
    print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
