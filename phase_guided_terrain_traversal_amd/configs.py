"""Task configuration: mirror of the reference's go2/configs.py:6-79 ``default_config()`` plus the
overrides training/train.py:127-129 applies before training (command range, gait frequency).

Plain nested dicts (the reference uses ml_collections.ConfigDict, which is not available here); keys and
values are the reference's.  ``scan_*`` come from go2/go2_constants.py:90-94 and go2/heightmap.py:38.
"""
from __future__ import annotations

import copy
from typing import Any, Dict, Optional


def default_config() -> Dict[str, Any]:
    return dict(
        ctrl_dt=0.02, sim_dt=0.005, episode_length=1000, vel_percentage=0.65, Kp=40.0, Kd=0.5,
        action_repeat=1, action_scale=0.5, history_len=2, history_update_steps=5,
        soft_joint_pos_limit_factor=0.95,
        noise_config=dict(level=1.0, scales=dict(joint_pos=0.03, joint_vel=1.5, gyro=0.2, gravity=0.05,
                                                 linvel=0.1, heightscan=0.01)),
        reward_config=dict(
            scales=dict(tracking_lin_vel=1.0, tracking_ang_vel=0.5, lin_vel_z=-1.0, ang_vel_xy=-0.05,
                        orientation=-0.2, dof_pos_limits=-1.0, pose=-1.0, termination=-1.0,
                        stand_still=-0.0, torques=-0.0002, action_rate=-0.01, energy=-0.0005,
                        feet_clearance=-0.0, feet_height=-0.0, feet_slip=-0.0, feet_air_time=0.0,
                        feet_phase=0.5, feet_swing=0.0, body_height=-0.0, contact=2.0, center=-0.0),
            tracking_sigma=0.2, swing_height=-0.2, base_feet_distance=-0.3, phase_sigma=0.05),
        command_config=dict(u_max=[1.5, 0.8, 1.2], u_min=[-1.5, -0.8, -1.2], b=[0.9, 0.25, 0.5]),
        gait_freq=[2, 6],
        heighmap_size=(13, 9),
        scan_dist_x=0.1, scan_dist_y=0.1, scan_z_offset=0.6,
        autoreset=0,
        method="pgtt",
    )


def baseline_config() -> Dict[str, Any]:
    """go2/configs.py:82-152 ``baseline_config()``: the comparison task go2/joystick.py is trained with."""
    cfg = default_config()
    cfg["reward_config"] = dict(
        scales=dict(tracking_lin_vel=1.0, tracking_ang_vel=0.5, lin_vel_z=-2.0, ang_vel_xy=-0.05,
                    orientation=-0.2, dof_pos_limits=-1.0, pose=-0.2, termination=-1.0,
                    stand_still=-0.5, torques=-0.0002, action_rate=-0.005, energy=-0.0005,
                    feet_clearance=-1.0, feet_height=-0.0, feet_slip=-0.1, feet_air_time=0.1,
                    feet_phase=0.0, feet_swing=0.0, body_height=-0.0, contact=0.0, center=-0.0),
        tracking_sigma=0.25, swing_height=-0.2, base_feet_distance=-0.3, phase_sigma=0.05)
    cfg["method"] = "baseline"
    return cfg


def training_config(method: str = "pgtt") -> Dict[str, Any]:
    """default_config() / baseline_config() with the overrides of training/train.py:120-129."""
    cfg = default_config() if method == "pgtt" else baseline_config()
    cfg["command_config"]["u_max"] = [0.6, 0.6, 1.0]
    cfg["command_config"]["u_min"] = [-0.6, -0.6, -1.0]
    cfg["gait_freq"] = [1, 3]
    return cfg


def evaluation_config(method: str = "pgtt") -> Dict[str, Any]:
    """the evaluator's env of training/evaluate.py:120-129: default_config() / baseline_config() with the NARROWER command range
    u_max = [0.4, 0.4, 0.7], u_min = -u_max and gait_freq = [1, 3] (survivor counts are quoted on these commands, not on training's +-0.6 / 1.0)."""
    cfg = default_config() if method == "pgtt" else baseline_config()
    cfg["command_config"]["u_max"] = [0.4, 0.4, 0.7]
    cfg["command_config"]["u_min"] = [-0.4, -0.4, -0.7]
    cfg["gait_freq"] = [1, 3]
    return cfg


# random pushes (Joystick(push=...), PgttConfig.push_*): MuJoCo Playground's Go2 joystick pert_config ranges, used for the ranges a command line leaves out
PUSH_DEFAULTS = {"wait": (1.0, 3.0), "duration": (0.05, 0.2), "velocity": (0.0, 3.0)}


def add_push_args(ap) -> None:
    """--push_velocity / --push_wait / --push_duration lo,hi of train.py and evaluate.py (none given: no pushes)"""
    ap.add_argument("--push_velocity", type=str, default=None, help="random pushes: torso velocity change of a kick, lo,hi m/s (e.g. 0,1.5)")
    ap.add_argument("--push_wait", type=str, default=None, help="random pushes: seconds between kicks, lo,hi (default 1,3)")
    ap.add_argument("--push_duration", type=str, default=None, help="random pushes: seconds a kick lasts, lo,hi (default 0.05,0.2)")


def push_from_args(args) -> Optional[Dict[str, Any]]:
    """the Joystick(push=...) dict of --push_* (PUSH_DEFAULTS for the ranges not given), or None when none of them is given"""
    given = {k: getattr(args, "push_" + k, None) for k in PUSH_DEFAULTS}
    if all(v is None for v in given.values()):
        return None
    out = {}
    for k, v in given.items():
        if v is None:
            out[k] = PUSH_DEFAULTS[k]
            continue
        parts = [float(x) for x in str(v).split(",")]
        if len(parts) != 2:
            raise ValueError(f"--push_{k} takes lo,hi (got {v!r})")
        out[k] = (parts[0], parts[1])
    return out


def add_curriculum_args(ap) -> None:
    """--terrain_files a,b,c [--curriculum [--curriculum_promote P --curriculum_demote D --curriculum_init lo,hi]] of train.py"""
    ap.add_argument("--terrain_files", type=str, default=None, help="comma-separated level files, easiest first: one stacked terrain table (a ladder of levels)")
    ap.add_argument("--curriculum", action="store_true", help="in-run terrain curriculum over --terrain_files: each finished episode moves its env up / down the ladder")
    ap.add_argument("--curriculum_promote", type=float, default=0.65, help="promote a truncated episode whose mean tracking_lin_vel term reaches this (0..1)")
    ap.add_argument("--curriculum_demote", type=float, default=0.5, help="demote an episode terminated before this share of episode_length (0..1)")
    ap.add_argument("--curriculum_init", type=str, default="0,0", help="initial levels lo,hi (uniform per env)")


def curriculum_from_args(args, ap=None) -> Optional[Dict[str, Any]]:
    """the Joystick(curriculum=...) dict of --curriculum*, or None; --curriculum without --terrain_files is a usage error"""
    if not getattr(args, "curriculum", False):
        return None
    if not getattr(args, "terrain_files", None):
        msg = "--curriculum needs --terrain_files (the ladder of level files)"
        if ap is not None:
            ap.error(msg)
        raise ValueError(msg)
    parts = [int(x) for x in str(args.curriculum_init).split(",")]
    if len(parts) != 2:
        raise ValueError(f"--curriculum_init takes lo,hi (got {args.curriculum_init!r})")
    return {"promote_tracking": float(args.curriculum_promote), "demote_length": float(args.curriculum_demote), "init_level": (parts[0], parts[1])}


def with_overrides(cfg: Dict[str, Any], **kw) -> Dict[str, Any]:
    out = copy.deepcopy(cfg)
    for k, v in kw.items():
        node = out
        parts = k.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    return out
