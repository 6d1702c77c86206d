"""Host-side mirror of the reference env interface (go2/joystick_pgtt.py:35-48, go2/base.py:216-231):

    env = Joystick(task="stairs", config=training_config(), num_envs=4096, terrain=level4, device="cuda:0")
    obs = env.reset(seed)                 # {'state': [N,171], 'privileged_state': [N,215]} torch tensors
    obs, reward, done, info = env.step(action)   # action [N,12] in [-1,1], FR,FL,RR,RL order

The reference env is functional (State pytrees under jax.vmap); this one is the batched, stateful
equivalent: state lives in caller-visible torch tensors (SoA in HBM) and every call enqueues HIP
kernels of libpgtt.so on the current torch stream.  PyTorch is only the allocator / stream provider.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import abi, configs, curriculum as _curriculum, mjcf, native


class Joystick:
    """Batched PGTT joystick env on one GPU.  Properties mirror reference go2/base.py:216-231."""

    def __init__(self, task: str = "flat_terrain", config: Optional[Dict[str, Any]] = None, num_envs: int = 4096,
                 terrain: Optional[np.ndarray] = None, device: str = "cuda:0", params: Optional[torch.Tensor] = None,
                 variant: Optional[torch.Tensor] = None, box_friction: Optional[torch.Tensor] = None,
                 autoreset: bool = False, debug_contacts: bool = False, env_id_offset: int = 0,
                 model: Optional[Dict[str, Any]] = None, layout: Optional[str] = None, observe_form: Optional[str] = None,
                 test_hooks: bool = False, interval_sums: bool = False, push: Optional[Dict[str, Any]] = None, xfrc: bool = False,
                 curriculum: Optional[Dict[str, Any]] = None, level: Optional[torch.Tensor] = None, depth: Optional[Dict[str, Any]] = None, student=None,
                 elevation=None, lidar: Optional[Dict[str, Any]] = None):
        """layout: "auto" | "quad" | "oct" | "hex" lane layout of physics_kernel (PgttConfig.lane_layout; results are bit-identical
        across batch sizes and shards within one layout); observe_form: "fused" | "split"; test_hooks: allow set_test_overrides
        (fixture replay only); interval_sums: keep per-env running sums of the step outputs for a logging trainer (PgttBuffers.interval_sums);
        push: random pushes, dict(wait=(lo, hi) s, duration=(lo, hi) s, velocity=(lo, hi) m/s) (or config["pert_config"] with MuJoCo
        Playground's keys): the step kicks the torso (pgtt_push); xfrc: allocate the torso-wrench buffer without pushes (apply_wrench);
        terrain: one (T, B, 10) table, or a list of level tables (stacked by curriculum.stack_levels; `level_start` says where each begins);
        curriculum: dict(promote_tracking=0.65, demote_length=0.5, init_level=0 | (lo, hi), seed=0[, level_start=...]): the terrain curriculum
        (pgtt_curriculum; needs autoreset): each finished episode moves its env up / down the levels and restarts it on a fresh variant.  With ONE
        stacked table as `terrain`, `level_start` (from curriculum.stack_levels) is required.  level / variant: the initial labels ([N] each), e.g.
        the "level" / "variant" of randomize.domain_randomize(seed=s, level_start=...); default: curriculum.initial_labels(curriculum["seed"], ...),
        the same draws for seed = s.  None: nothing of it is allocated, bound or launched.
        depth: an onboard depth camera (depth.DepthCamera's arguments over depth.DEFAULTS, e.g. dict(width=64, height=48, fovy=58, near=0.1, far=3.0,
        mount_pos=(0.30, 0.0, 0.05), pitch_deg=30, every=1, see_robot=True, noise=dict(sigma=0.0, dropout=0.0)); the mount defaults are placeholders
        for a Go2 head camera - settings, not facts): `env.depth` is the [N, H, W] image, step() ticks the sensor after the step on the same stream,
        reset() ticks it with force.  A side output: the observations and every other buffer are what they are without it.  None: nothing of it
        is allocated, loaded, bound or launched.
        student: a perceive.ScanEstimator or the path of a saved one (needs depth): the student perception module (libpgtt_perceive.so) runs behind
        the camera after every step and reset; `env.student_obs` is the [N, obs_dim] observation with the 117 scan rows replaced by its estimate.  A
        side output like the image.  None: the library is not opened.  A recurrent estimator (perceive.config(memory=R)) keeps a memory per env,
        `env.student_mem` [N, R]: reset() starts the reset envs' memory from zero, step() that of the envs whose episode just ended, as for the map
        below, and the note on a deferred curriculum there applies to it too (`env.student.tick(use_done=True)` after curriculum_step()).
        elevation: True or elevation.ElevationMap's arguments over elevation.DEFAULTS, e.g. dict(grid=64, res=0.04, alpha=1.0) (needs depth, with the
        camera on the torso and every=1): a depth-fused elevation map per env (libpgtt_elevation.so) is ticked behind the camera - after reset() with
        the reset envs' maps cleared, after step() with the maps of the envs whose episode just ended cleared; `env.elevation_obs` is the
        [N, obs_dim] observation with the 117 scan rows sampled from the map, `env.elevation_known` [N, 117] says which of them the map knew,
        `env.elevation_map` is the ElevationMap.  A side output like the image; may be combined with student.  None: the library is not opened.
        elevation=dict(fill=K, ...) (K passes, True = 16; dense=True keeps the filled map too) closes the map's holes behind every tick, on a copy:
        `env.elevation_filled_obs` [N, obs_dim] has the scan rows sampled from the filled map and `env.elevation_dist` [N, 117] uint8 says how each
        was come by (0 measured, p = filled in pass p, 255 unknown); elevation_obs and elevation_known stay what they are without it.
        The map has memory, so what moves an env must clear it: reset() and step() do, set_terrain() forgets every map, but with a deferred
        curriculum (step(action, curriculum=False), then curriculum_step()) the envs are restarted AFTER the step's tick, as they are after the
        camera's - such a caller ticks the camera and then `env.elevation_map.tick(use_done=True)` once more after curriculum_step().
        lidar: an onboard LiDAR (lidar.LidarScanner's arguments over lidar.DEFAULTS, e.g. dict(n_az=128, n_el=16, az_deg=(-180, 180),
        el_deg=(-85, 10), near=0.05, far=3.0, mount_pos=(0.29, 0.0, -0.04), every=1, see_robot=True) or dict(pattern=[R, 3] directions, ...); the
        defaults are placeholders for a chin-mounted hemispherical scanner - settings, not facts): `env.lidar` is the [N, R] range scan,
        `env.lidar_points` the [N, R, 3] world points of its returns, `env.lidar_scanner` the LidarScanner; ticked next to the camera, after every
        step and (with force) reset.  A side output like the image.  None: the library is not opened.
        elevation=dict(source="lidar", ...) fuses the map from the LiDAR's points instead of the image: it needs lidar (with every=1, on any body:
        the points are world points) and no depth; clearing goes exactly as for the camera-fed map.
        elevation=dict(follow_sensor=True, ...) lifts the two `every=1` conditions: the sensor that feeds the map may have any period (depth=dict(every=3),
        or lidar=dict(every=3) with source="lidar"; the camera still sits on the torso).  The map then fuses on the steps on which that sensor takes
        new data - reset() forces one - and on the steps in between it is left as it is, but for the clears, while elevation_obs, elevation_known and
        the filled outputs are sampled from it at the current pose on every step (pgtt_elevation_follow).  With every=1 the bits are those of an env
        without the flag.
        elevation=dict(variance=True | dict(sigma0=..., sigma_rel=..., process=..., gate=..., band=..., max_count=..., var_max=...), ...) replaces the
        maximum-and-alpha fusion by a variance-weighted (Kalman) update per cell (pgtt_elevation_var; elevation.VARIANCE_DEFAULTS): the map keeps a
        variance layer `env.elevation_map.var`, and `env.elevation_var` [N, 117] is the variance at the scan points.  Not with follow_sensor; grid <= 64.
        elevation=dict(odometry=True | dict(sigma_xy=..., sigma_z=..., sigma_yaw=..., yaw_bias=..., scale=..., seed=...), ...) registers the map with a
        dead-reckoned pose that drifts in x, y, z and yaw instead of the simulator's (pgtt_elevation_odometry; elevation.ODOMETRY_DEFAULTS, settings and
        not facts about a robot): `env.odometry_pose` [7, N] is the estimate, `env.odometry_error` [N, 4] its position and yaw error (e_x, e_y, e_z,
        psi), zero after reset() and for an env whose episode just ended.  Works with fill, variance, follow_sensor and both sources.
        obs, state, reward, done, the image and the LiDAR's outputs are what they are without it.
        elevation=dict(visibility=True | dict(margin=..., end_guard=..., stride=..., sigmas=...), ...) cleans the map by visibility in front of every
        tick (pgtt_elevation_visibility; elevation.VISIBILITY_DEFAULTS): a cell that a ray passed below on its way to the ground is forgotten, which
        removes the ghosts a drifting pose leaves.  `env.elevation_cleared` [N] int32 is the number of cells the last step forgot.  With both sources
        (a LiDAR on the torso); not with follow_sensor.  obs, state, reward, done and the sensors' outputs are what they are without it.
        elevation=dict(latency=K | (lo, hi) | dict(ticks=..., seed=...), ...) gives the sensor a latency (pgtt_elevation_delayed;
        elevation.LATENCY_DEFAULTS): every frame is fused K steps after it was taken, under the pose of its capture, while the window and the scan
        follow the current pose; (lo, hi) draws the latency per env per episode.  `env.elevation_latency` [N] int32 is each env's latency and
        `env.elevation_fused` [N] uint8 whether the last step fused a frame: the first K steps of an episode fuse nothing.  With both sources, with
        fill and odometry; not with variance, visibility or follow_sensor.  Latency 0 gives the bits of an env without the key; obs, state,
        reward, done and the sensors' outputs are what they are without it."""
        if student is not None and depth is None:
            raise ValueError("Joystick(student=...) needs depth=dict(...): the student reads the onboard depth image")
        wants_map = elevation is not None and elevation is not False
        map_source = "depth" if not wants_map or elevation is True else dict(elevation).get("source", "depth")
        follows = wants_map and elevation is not True and bool(dict(elevation).get("follow_sensor", False))
        if wants_map and map_source not in ("depth", "lidar"):
            raise ValueError(f"Joystick(elevation=dict(source=...)): source must be 'depth' or 'lidar', not {map_source!r}")
        if wants_map and map_source == "lidar":
            if lidar is None:
                raise ValueError("Joystick(elevation=dict(source='lidar')) needs lidar=dict(...): the elevation map is fused from the LiDAR's points")
            if int(dict(lidar).get("every", 1)) != 1 and not follows:
                raise ValueError("Joystick(elevation=dict(source='lidar')) needs a LiDAR with every=1: the map would fuse a stale scan again at every tick")
        if wants_map and map_source == "depth" and depth is None:
            raise ValueError("Joystick(elevation=...) needs depth=dict(...): the elevation map is fused from the onboard depth image")
        if wants_map and map_source == "depth" and ((int(dict(depth).get("every", 1)) != 1 and not follows) or int(dict(depth).get("mount_body", 0)) != 0):
            raise ValueError("Joystick(elevation=...) needs a camera on the torso (mount_body=0) with every=1: a stale image under a moved pose "
                             "would be unprojected wrongly")
        variance = dict(elevation).get("variance") if wants_map and elevation is not True else None
        if variance is not None and variance is not False:
            if follows:
                raise ValueError("Joystick(elevation=dict(variance=..., follow_sensor=True)): variance behind a slower sensor is not built yet")
            if variance is not True and not isinstance(variance, dict):
                raise ValueError(f"Joystick(elevation=dict(variance=...)): variance must be True or a dict of settings, not {variance!r}")
        latency = dict(elevation).get("latency") if wants_map and elevation is not True else None
        if latency is not None and latency is not False:
            for name in ("variance", "visibility", "follow_sensor"):
                other = dict(elevation).get(name)
                if other is not None and other is not False:
                    raise ValueError(f"Joystick(elevation=dict(latency=..., {name}=...)): latency with {name} is not built")
        self.level_start = None
        if isinstance(terrain, (list, tuple)):
            terrain, self.level_start = _curriculum.stack_levels(terrain)
        self._config = dict(configs.default_config() if config is None else config)
        self._config["autoreset"] = int(autoreset)
        if layout is not None:
            self._config["lane_layout"] = layout
        if observe_form is not None:
            self._config["observe_form"] = observe_form
        if test_hooks:
            self._config["test_hooks"] = True
        if push is not None:
            self._config["push"] = dict(push)
        self.push = abi.push_ranges(self._config)          # None: no pushes
        if curriculum is not None:
            if task != "stairs" or terrain is None:
                raise ValueError("the terrain curriculum needs task='stairs' and a terrain (a list of level tables)")
            given = curriculum.get("level_start")
            if self.level_start is None:
                # one stacked table (curriculum.stack_levels done by the caller, as train.py does): the caller says where its levels begin
                if given is None:
                    raise ValueError("curriculum with one stacked terrain table needs curriculum['level_start'] (what curriculum.stack_levels "
                                     "returned); or pass terrain=[level tables] and let Joystick stack them")
                self.level_start = np.asarray(given, dtype=np.int32)
            elif given is not None and [int(v) for v in given] != [int(v) for v in self.level_start]:
                raise ValueError(f"curriculum['level_start'] {list(given)} does not match the stacked level tables {self.level_start.tolist()}")
            if int(self.level_start[0]) != 0 or int(self.level_start[-1]) != np.asarray(terrain).shape[0]:
                raise ValueError(f"curriculum level_start {self.level_start.tolist()} does not span the terrain table's {np.asarray(terrain).shape[0]} variants")
            self._config["curriculum"] = dict(curriculum, level_start=[int(v) for v in self.level_start])
        self.curriculum = abi.curriculum_settings(self._config)      # None: no curriculum
        self._cur_deferred = False
        self.method = self._config.get("method", "pgtt")     # "pgtt" = go2/joystick_pgtt.py, "baseline" = go2/joystick.py
        self.task = task
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise native.PgttError("Joystick needs a ROCm device (device='cuda:N'); there is no CPU path")
        self._model = mjcf.load_model(task) if model is None else model
        self._ms = abi.model_struct(self._model)
        self._cs = abi.config_struct(self._config)
        self._lib = native.lib()
        self._h = C.c_void_p()
        native.check(self._lib.pgtt_create(C.byref(self._cs), C.byref(self._ms), self.device.index or 0,
                                           self.num_envs, C.byref(self._h)))
        self.env_id_offset = int(env_id_offset)
        self.terrain = None
        if task == "stairs":
            if terrain is None:
                raise ValueError("task='stairs' needs a terrain table (T,B,10), e.g. assets/terrains/level4.npy")
            self.set_terrain(terrain)
        n = self.num_envs
        self.buffers: Dict[str, torch.Tensor] = {}
        for spec in abi.BUFFER_SPECS:
            dt = torch.float32 if spec[2] == np.float32 else torch.int32
            self.buffers[spec[0]] = torch.zeros(abi.buffer_shape(spec, n, self.method), dtype=dt, device=self.device)
        # the 22 metric rows, the reward row and the done row live in ONE [24][N] block, so that a trainer can reduce
        # them over the envs with a single kernel (distributed.MetricReducer.accumulate_block)
        self.step_block = torch.zeros((abi.NMETRIC + 2, n), dtype=torch.float32, device=self.device)
        self.buffers["metrics"] = self.step_block[:abi.NMETRIC]
        self.buffers["reward"] = self.step_block[abi.NMETRIC]
        self.buffers["done"] = self.step_block[abi.NMETRIC + 1]
        # per-env running sums of [22 metrics; reward; done] since the trainer last cleared them: a log interval then costs one
        # reduction over the envs (distributed.MetricReducer.reduce_block), not one per step
        # (opt-in: 24 read-modify-writes per env-step that only a logging loop such as bench.py consumes and clears)
        if interval_sums:
            self.buffers["interval_sums"] = torch.zeros((abi.NMETRIC + 2, n), dtype=torch.float32, device=self.device)
        if params is not None:
            self.buffers["params"] = params.to(self.device, torch.float32).contiguous()
            assert self.buffers["params"].shape == (abi.NPARAM, n)
        if self.curriculum is not None:
            # the curriculum's labels: caller-owned like every buffer, kept by the library after the first reset
            if level is None:
                lv, va = _curriculum.initial_labels(self.curriculum["seed"], self.env_id_offset, n, self.level_start, self.curriculum["init_level"])
                level = torch.from_numpy(lv)
                variant = torch.from_numpy(va) if variant is None else variant
            elif variant is None:
                raise ValueError("Joystick(level=...) needs variant=... as well (each env's variant inside its level)")
            self.buffers["level"] = level.to(self.device, torch.int32).contiguous()
            self.buffers["curriculum_stats"] = torch.zeros(abi.NCSTAT, dtype=torch.int32, device=self.device)
        if variant is not None:
            self.buffers["variant"] = variant.to(self.device, torch.int32).contiguous()
        if box_friction is not None:
            self.buffers["box_friction"] = box_friction.to(self.device, torch.float32).contiguous()
            assert self.buffers["box_friction"].shape == (abi.MAX_BOX, n)
        if debug_contacts:
            self.buffers["dbg_contact"] = torch.zeros((n, abi.NCON * 2), dtype=torch.int32, device=self.device)
            self.buffers["dbg_dist"] = torch.zeros((n, abi.NCON), dtype=torch.float32, device=self.device)
            self.buffers["dbg_niter"] = torch.zeros((n,), dtype=torch.int32, device=self.device)
        # external wrench on the torso ([6][N]: world force, world torque; PgttBuffers.xfrc) and the push scheduler's state ([NPUSH][N])
        if xfrc or self.push is not None:
            self.buffers["xfrc"] = torch.zeros((abi.NXFRC, n), dtype=torch.float32, device=self.device)
        if self.push is not None:
            self.buffers["push_state"] = torch.full((abi.NPUSH, n), -1.0, dtype=torch.float32, device=self.device)
        self._bind()
        if self.curriculum is not None:
            self._set_curriculum()
        self._seed = 0
        self.depth_camera = None
        if depth is not None:
            from . import depth as _depth                     # libpgtt_depth.so is opened only here
            self.depth_camera = _depth.DepthCamera(self, **_depth.settings(depth))
        self.lidar_scanner = None
        if lidar is not None:
            from . import lidar as _lidar                     # libpgtt_lidar.so is opened only here
            self.lidar_scanner = _lidar.LidarScanner(self, **_lidar.settings(lidar))
        self.student = None
        if student is not None:
            from . import perceive as _perceive               # libpgtt_perceive.so is opened only here
            est = _perceive.ScanEstimator.load(student) if isinstance(student, (str, os.PathLike)) else student
            self.student = _perceive.StudentPerception(self, est)
        self.elevation_map = None
        if elevation is not None and elevation is not False:
            from . import elevation as _elevation             # libpgtt_elevation.so is opened only here
            self.elevation_map = _elevation.ElevationMap(self, **_elevation.settings(elevation))

    # ---- reference-compatible properties
    @property
    def dt(self) -> float:
        return self._config["ctrl_dt"]

    @property
    def action_size(self) -> int:
        return abi.NU

    @property
    def observation_size(self) -> Dict[str, int]:
        od, pd = abi.obs_dims(self.method)
        return {"state": od, "privileged_state": pd}

    @property
    def config(self) -> Dict[str, Any]:
        return self._config

    # go2/base.py:216-231 also exposes the compiled model and where it came from.  Here the "MuJoCo model" is the dict of compiled
    # constants (mjcf.compile_mjcf of go2_mjx_feetonly.xml + scene, shipped as assets/go2_<task>.json), and its device form is the
    # PgttModel struct the kernels read.
    @property
    def mj_model(self) -> Dict[str, Any]:
        return self._model

    @property
    def mjx_model(self) -> "abi.PgttModel":
        return self._ms

    @property
    def xml_path(self) -> str:
        return mjcf.asset_path(self.task)

    @property
    def model(self) -> Dict[str, Any]:
        return self._model

    def _bind(self) -> None:
        b = abi.PgttBuffers()
        for name, _ in abi.PgttBuffers._fields_:
            t = self.buffers.get(name)
            setattr(b, name, None if t is None else t.data_ptr())
        native.check(self._lib.pgtt_bind(self._h, C.byref(b)))

    def _set_curriculum(self) -> None:
        cs = abi.curriculum_struct(self.curriculum, self.buffers["level"].data_ptr(), self.buffers["curriculum_stats"].data_ptr())
        native.check(self._lib.pgtt_set_curriculum(self._h, C.byref(cs)))

    @property
    def xfrc(self) -> Optional[torch.Tensor]:
        """[6][N] view of the wrench on each env's torso (rows 0..2 world force, 3..5 world torque, at the torso COM), or None when the env has
        no wrench buffer (Joystick(..., xfrc=True) or push=... allocate it; apply_wrench does on first use)"""
        return self.buffers.get("xfrc")

    def apply_wrench(self, force, torque=None, env_ids=None) -> torch.Tensor:
        """Set the torso wrench that the following steps apply (held until changed; MuJoCo's xfrc_applied[torso]).  force / torque: [3] or
        [len(env_ids), 3] world-frame values (torque None = zero); env_ids: the envs to set (None = all).  Not with random pushes, which own
        the buffer."""
        if self.push is not None:
            raise native.PgttError("apply_wrench: this env has random pushes enabled; the push scheduler writes the wrench")
        if "xfrc" not in self.buffers:
            self.buffers["xfrc"] = torch.zeros((abi.NXFRC, self.num_envs), dtype=torch.float32, device=self.device)
            self._bind()
        x = self.buffers["xfrc"]
        ids = slice(None) if env_ids is None else torch.as_tensor(env_ids, device=self.device, dtype=torch.long)
        f = torch.as_tensor(force, dtype=torch.float32, device=self.device)
        t = torch.zeros_like(f) if torque is None else torch.as_tensor(torque, dtype=torch.float32, device=self.device)
        x[0:3, ids] = f.T if f.ndim == 2 else f[:, None]
        x[3:6, ids] = t.T if t.ndim == 2 else t[:, None]
        return x

    @property
    def depth(self) -> Optional[torch.Tensor]:
        """[N, H, W] float32 image of the onboard depth camera (metres along the optical axis, `far` on a miss), or None without one"""
        return None if self.depth_camera is None else self.depth_camera.image

    @property
    def lidar(self) -> Optional[torch.Tensor]:
        """[N, R] float32 range scan of the onboard LiDAR (metres along the ray, `far` on a miss), or None without one"""
        return None if self.lidar_scanner is None else self.lidar_scanner.ranges

    @property
    def lidar_points(self) -> Optional[torch.Tensor]:
        """[N, R, 3] float32 world points of the LiDAR's returns (NaN where a ray has none), or None without a LiDAR"""
        return None if self.lidar_scanner is None else self.lidar_scanner.points

    @property
    def student_obs(self) -> Optional[torch.Tensor]:
        """[N, obs_dim] float32: the observation with its scan rows replaced by the student's estimate from the depth image, or None without one"""
        return None if self.student is None else self.student.obs

    @property
    def student_mem(self) -> Optional[torch.Tensor]:
        """[N, R] float32: the recurrent student's memory as its last tick left it, or None without a recurrent student"""
        return None if self.student is None else self.student.mem

    @property
    def elevation_obs(self) -> Optional[torch.Tensor]:
        """[N, obs_dim] float32: the observation with its scan rows sampled from the depth-fused elevation map, or None without one"""
        return None if self.elevation_map is None else self.elevation_map.obs

    @property
    def elevation_known(self) -> Optional[torch.Tensor]:
        """[N, 117] uint8: 1 where the elevation map knew the scan point's cell, or None without a map"""
        return None if self.elevation_map is None else self.elevation_map.known

    @property
    def elevation_filled_obs(self) -> Optional[torch.Tensor]:
        """[N, obs_dim] float32: the observation with its scan rows sampled from the hole-filled elevation map, or None without a map that fills"""
        return getattr(self.elevation_map, "filled_obs", None)

    @property
    def elevation_dist(self) -> Optional[torch.Tensor]:
        """[N, 117] uint8: 0 where the scan point's cell was measured, p where pass p filled it, 255 where it is unknown; None without a map that fills"""
        return getattr(self.elevation_map, "filled_dist", None)

    @property
    def elevation_var(self) -> Optional[torch.Tensor]:
        """[N, 117] float32: the variance (m^2) of the elevation map at the scan points, var_max at an unknown one; None without a variance map"""
        return getattr(self.elevation_map, "est_var", None)

    @property
    def odometry_error(self) -> Optional[torch.Tensor]:
        """[N, 4] float32, a view: the error (e_x, e_y, e_z, psi) of the pose the elevation map is registered with; None without odometry drift"""
        odo = getattr(self.elevation_map, "odo", None)
        return None if odo is None else odo[:, :4]

    @property
    def elevation_latency(self) -> Optional[torch.Tensor]:
        """[N] int32: the steps between a frame's capture and its fusion into the elevation map, per env for this episode; None without latency"""
        return getattr(self.elevation_map, "latency", None)

    @property
    def elevation_fused(self) -> Optional[torch.Tensor]:
        """[N] uint8: 1 where the last tick of the elevation map fused a frame, 0 where the frame that was due predates the episode; None without latency"""
        return getattr(self.elevation_map, "fused", None)

    @property
    def elevation_cleared(self) -> Optional[torch.Tensor]:
        """[N] int32, a view: the cells the visibility clean-up forgot in front of the last tick of the elevation map; None without the clean-up"""
        return getattr(self.elevation_map, "cleared", None)

    @property
    def odometry_pose(self) -> Optional[torch.Tensor]:
        """[7, N] float32: the dead-reckoned base pose (position, quaternion wxyz) the elevation map is registered with; None without odometry drift"""
        return getattr(self.elevation_map, "pose_est", None)

    def push_step(self) -> None:
        """the push scheduler alone (pgtt_push): what step() runs first when pushes are on; for callers of physics() / observe()"""
        native.check(self._lib.pgtt_push(self._h, self._stream()))

    @property
    def level(self) -> Optional[torch.Tensor]:
        """[N] int32 view of each env's current curriculum level, or None without a curriculum"""
        return self.buffers.get("level")

    def curriculum_step(self) -> None:
        """the curriculum alone (pgtt_curriculum): what step() runs last when the curriculum is on; for callers of physics() / observe() and of
        step(action, curriculum=False).  The camera, the student and the elevation map were ticked by that step, before this restart: their
        outputs for a restarted env are the old pose's until the next step, and its map - and a recurrent student's memory - keep that one image of
        the old place (see `elevation`)"""
        native.check(self._lib.pgtt_curriculum(self._h, self._stream()))

    def curriculum_stats(self) -> Dict[str, Any]:
        """{"finished_per_level": [L], "promoted", "demoted", "finished", "mean_level"} since the last call; clears the counters (one read-back)"""
        if self.curriculum is None:
            raise native.PgttError("curriculum_stats: this env has no terrain curriculum - create it with Joystick(..., curriculum=dict(...))")
        st = self.buffers["curriculum_stats"]
        s = st.tolist()
        st.zero_()
        L = len(self.level_start) - 1
        return {"finished_per_level": s[:L], "promoted": s[abi.CS_PROMOTED], "demoted": s[abi.CS_DEMOTED], "finished": s[abi.CS_FINISHED],
                "mean_level": float(self.buffers["level"].float().mean())}

    def set_terrain(self, terrain: np.ndarray) -> None:
        """replace the resident terrain table (the depth camera's and the LiDAR's too; an elevation map forgets what it saw of the old one).  The tables are
        reallocated: a graph captured before this call still points at the old ones and must be captured again, not replayed"""
        t = np.ascontiguousarray(terrain, dtype=np.float32)
        assert t.ndim == 3 and t.shape[2] == 10 and t.shape[1] <= abi.MAX_BOX
        native.check(self._lib.pgtt_set_terrain(self._h, t.ctypes.data, t.shape[0], t.shape[1]))
        self.terrain = t
        if getattr(self, "depth_camera", None) is not None:
            self.depth_camera.set_terrain(t)
        if getattr(self, "lidar_scanner", None) is not None:
            self.lidar_scanner.set_terrain(t)
        if getattr(self, "elevation_map", None) is not None:
            self.elevation_map.map.fill_(float("nan"))                # heights of the old terrain: the next tick starts from an empty map
            if getattr(self.elevation_map, "var", None) is not None:
                self.elevation_map.var.fill_(float("nan"))            # the variance layer is NaN where the map is
            if getattr(self.elevation_map, "latency_age", None) is not None:
                self.elevation_map.latency_age.zero_()                # the ring's frames show the old terrain: none of them is due any more

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _obs(self) -> Dict[str, torch.Tensor]:
        return {"state": self.buffers["obs_state"], "privileged_state": self.buffers["obs_priv"]}

    def reset(self, seed: int = 0, mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        self._seed = int(seed)
        mp = None
        if mask is not None:
            mask = mask.to(self.device, torch.uint8).contiguous()
            mp = mask.data_ptr()
        native.check(self._lib.pgtt_reset(self._h, self._seed, self.env_id_offset, mp, self._stream()))
        if self.depth_camera is not None:
            self.depth_camera.tick(force=True)
        if self.lidar_scanner is not None:
            self.lidar_scanner.tick(force=True)
        if self.student is not None:
            if self.student.memory:
                self.student.tick(clear_mask=mask, clear_all=mask is None)
            else:
                self.student.tick()
        if self.elevation_map is not None:
            self.elevation_map.tick(clear_mask=mask, clear_all=mask is None, force=True)
        return self._obs()

    def step(self, action: torch.Tensor, curriculum: bool = True):
        """curriculum=False (only with a curriculum): leave pgtt_curriculum to the caller, who reads done / episode_metrics of the step first and
        then calls curriculum_step() (the restart clears the episode sums; acting.FusedActor records in between)"""
        a = action.to(self.device, torch.float32).contiguous()
        assert a.shape == (self.num_envs, abi.NU)
        if self.curriculum is not None and self._cur_deferred != (not curriculum):
            native.check(self._lib.pgtt_set_curriculum_deferred(self._h, int(not curriculum)))
            self._cur_deferred = not curriculum
        native.check(self._lib.pgtt_step(self._h, a.data_ptr(), self._stream()))
        if self.depth_camera is not None:
            self.depth_camera.tick()
        if self.lidar_scanner is not None:
            self.lidar_scanner.tick()
        if self.student is not None:
            if self.student.memory:
                self.student.tick(use_done=True)
            else:
                self.student.tick()
        if self.elevation_map is not None:
            self.elevation_map.tick(use_done=True, force=False)
        info = {"metrics": self.buffers["metrics"], "episode_metrics": self.buffers["ep_metrics"]}
        return self._obs(), self.buffers["reward"], self.buffers["done"], info

    def physics(self, action: torch.Tensor) -> None:
        a = action.to(self.device, torch.float32).contiguous()
        native.check(self._lib.pgtt_physics(self._h, a.data_ptr(), self._stream()))

    def observe(self, action: torch.Tensor) -> None:
        a = action.to(self.device, torch.float32).contiguous()
        native.check(self._lib.pgtt_observe(self._h, a.data_ptr(), self._stream()))

    def scan(self, yaw: Optional[float] = None) -> torch.Tensor:
        native.check(self._lib.pgtt_scan(self._h, float("nan") if yaw is None else float(yaw), self._stream()))
        return self.buffers["scan_z"]

    def interval_reduce(self, out: torch.Tensor, env_steps: float = 0.0, accumulate: bool = False) -> None:
        """out[k] (+)= sum over the envs of buffers['interval_sums'][k] (k < NMETRIC + 2), out[NMETRIC + 2] (+)= env_steps, the rows cleared:
        one launch (pgtt_interval_reduce)"""
        if "interval_sums" not in self.buffers:
            raise native.PgttError("interval_reduce: this env keeps no interval sums - create it with Joystick(..., interval_sums=True)")
        if not (out.dtype == torch.float32 and out.is_contiguous() and out.numel() == abi.NMETRIC + 3 and out.device == self.buffers["interval_sums"].device):
            raise ValueError(f"interval_reduce: `out` must be {abi.NMETRIC + 3} contiguous float32 values on {self.buffers['interval_sums'].device}")
        native.check(self._lib.pgtt_interval_reduce(self._h, out.data_ptr(), float(env_steps), int(accumulate), self._stream()))

    def set_test_overrides(self, rng_value: Optional[float] = None, scan_preset: bool = False) -> None:
        """test hooks of libpgtt (include/pgtt.h): fixed uniform draws / scan heights taken from buffers['scan_z']"""
        native.check(self._lib.pgtt_set_test_overrides(self._h, float("nan") if rng_value is None else float(rng_value), int(scan_preset)))

    def enable_timing(self, on=True) -> None:
        """False / True / n > 1 = time every n-th step (HIP events around the kernels, on the launch stream)"""
        native.check(self._lib.pgtt_enable_timing(self._h, int(on)))

    def last_kernel_ms(self):
        p, o = C.c_float(), C.c_float()
        native.check(self._lib.pgtt_last_kernel_ms(self._h, C.byref(p), C.byref(o)))
        return p.value, o.value

    def kernel_ms_mean(self):
        """(physics ms, observe ms, steps): mean kernel times over all steps since enable_timing(True)"""
        p, o, k = C.c_float(), C.c_float(), C.c_int()
        native.check(self._lib.pgtt_kernel_ms_mean(self._h, C.byref(p), C.byref(o), C.byref(k)))
        return p.value, o.value, k.value

    def close(self) -> None:
        if getattr(self, "elevation_map", None) is not None:
            self.elevation_map.close()
            self.elevation_map = None
        if getattr(self, "student", None) is not None:
            self.student.close()
            self.student = None
        if getattr(self, "depth_camera", None) is not None:
            self.depth_camera.close()
            self.depth_camera = None
        if getattr(self, "lidar_scanner", None) is not None:
            self.lidar_scanner.close()
            self.lidar_scanner = None
        if getattr(self, "_h", None):
            self._lib.pgtt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
