"""Benchmark of the hot path: env-steps/s of the vectorised Go2 joystick_pgtt step on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--envs 4096] [--workload level4|flat|level13_dr|wfc_dr|curriculum] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one control step (4 physics substeps + 13x9 scan + obs + 21 rewards + bookkeeping, with the
Episode/AutoReset wrapper fused) over the per-GPU batch of synthetic actions.  Workload = BASELINE.json
configs[2]: 4096 Go2 envs per GPU on terrains/level4.npy with the height scan, no DR (the configuration the
metric "env-steps/sec at 4096 envs (Go2, level4 hfield)" is quoted on).  Weak scaling: every GPU owns 4096
envs; the only collective is the 25-float metric all-reduce every 20 steps (RCCL).

Launch: under torchrun the ranks come from the environment; a bare `python bench.py --gpus N` (N > 1) SPAWNS the
N ranks itself (one process per GPU) and refuses when the node has fewer than N devices.

Before the clock starts the whole timed loop body runs at least once per code path whatever --warmup says (one pass
over the action pool with the kernel events recorded on every step, two interval reductions with their fused all-reduce):
nothing in the timed window loads a code object or creates an event for the first time.  `wall_over_kernels` =
ms_per_step / (physics + observe + the interval reduction's share of a step); "cold": true (and exit code 3) when it exceeds 1.5.

Prints ONE JSON line (rank 0).  `roofline` is for the dominant kernel (physics_kernel) with ITS share of the algorithmic work
(1.2 MFLOP, 0.8 KB per env-step), `roofline_observe` / `roofline_step` the scan kernel and the whole step (all from the headline window's
own kernel events, no run of their own).  A plain run does nothing else: set-up, warm-up, the K timed steps, the outputs, the line.

--full adds what takes runs of its own, after the headline window (never part of `value`): `cpu_baseline`, the build's own CPU
restatement (oracle/, kind "port") timed on the host's cores on a bounded sample (--no-cpu-baseline skips it), and with one GPU
`other_configs`: BASELINE configs[1] (flat, 4096), configs[3] (WFC + DR, 8192), level4 at 32768 envs, the seven per-rank workloads of
configs[4] (one curriculum level file each, 4096 envs), the step loop replayed as ONE HIP graph per 20 steps, the roll-out row and the
1-ulp-division side build, 100 steps each (--no-other-configs skips them).

--dump-outputs DIR writes what the last timed step returned to its caller (env.step: observations, reward, done, info) as DIR/<name>.npy,
float32, at most 64 MB in all (above that, the same seeded sample of envs from every array, its indices in DIR/env_index.npy); with
more than one rank each rank writes <name>_rank<r>.npy.  Inputs (reset seed, terrain variants, action pool) are fixed by the arguments,
so two builds can be compared output for output.

`roofline.traffic` / `valu_busy` / `mfma_ops` come from the rocprofv3 --pmc passes committed under profiles/ (hbm_traffic.json, which
records the SHA-256 of the kernel sources it was measured on); when the sources of the library being timed differ they are null and
the line says "profile_stale": true.

`--backend gloo` is a TEST HOOK (tests/test_distributed.py): CPU tensors and a stub env, so that the rank / barrier /
MAX-over-ranks / rank-0-print path of this file runs without a GPU; its line carries "stub": true and is not a result.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic per-env-step figures (restated in DESIGN.md 6): the whole control step, and its split over the two kernels
ALGO_BYTES_PER_ENV_STEP = 3456          # no-DR workload; 4216 with per-env DR params
ALGO_BYTES_PER_ENV_STEP_DR = 4216
ALGO_FLOP_PER_ENV_STEP = 1.6e6          # fp32, dense MJX formulation (the reference's arithmetic): 4 x 0.30 physics + 0.35 scan + task layer
ALGO_FLOP_PHYSICS = 1.2e6               # 4 substeps x 0.30 MFLOP (kinematics, CRBA, factor, RNE, collision, 44-row constraint build, Newton x line search)
ALGO_FLOP_OBSERVE = 0.35e6              # 117 rays x 101 geoms x ~30 (+ < 0.01 MFLOP of task layer)
# physics_kernel's own compulsory rows: reads qpos 19 + qvel 18 + warm start 18 + action 12 = 67, writes qpos 19 + qvel 18 + warm start 18
# + motor targets 12 + sensor frame 65 = 132 floats -> 796 B per env-step (+ 77 DR rows = 308 B and one box-friction row per contact with DR)
ALGO_BYTES_PHYSICS = 4 * (67 + 132)
ALGO_BYTES_PHYSICS_DR = ALGO_BYTES_PHYSICS + 4 * 77
PEAK_FP32_TFLOPS = 157.3                # MI355X fp32 vector peak (MI355X_MICROARCH.md); the fp32 matrix peak is the same number
PEAK_FP32_UNPACKED_TFLOPS = 78.65      # the same vector ALUs issuing UNPACKED fp32 FMAs (one per lane per cycle): the ceiling of an instruction stream without v_pk_*
PEAK_HBM_GBS = 8000.0
CURRICULUM = [1, 2, 3, 4, 7, 10, 13]    # the level files the reference ships (terrains/level*.npy), easiest first
REDUCE_EVERY = 20                       # log interval of the metric all-reduce (unroll length of training/train.py:142)
COLD_RATIO = 1.5
# untimed steps after the reset before the clock starts.  SURVEY 8d asks for 100 (the robots' landing); the DEVICE asks for more: in a fresh
# process the first ~100 control steps (~20 ms of GPU time) run up to 13 % slower than the same steps of a second roll-out in the same
# process (profiles/archive/r03_step_profile.txt: physics_kernel 190 / 178 / 173 / 169 us over the first four blocks of 25 steps, 168 from the
# first block when the roll-out is repeated) - clocks ramping, not the simulation.  BASELINE.md quotes the metric on the steady state, and
# the driver's command times 20 steps: 1500 steps (0.3 s at 4096 envs) put that window where the 300-step default already is.
PRIME_STEPS = 1500


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--envs", type=int, default=4096, help="envs per GPU")
    ap.add_argument("--workload", default="level4", choices=["level4", "flat", "level13_dr", "wfc_dr", "curriculum"])
    ap.add_argument("--stage", type=int, default=None, help="curriculum workload: index into the level list (default: the rank)")
    ap.add_argument("--full", action="store_true", help="also the measurements that take runs of their own: cpu_baseline and other_configs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs as DIR/<name>.npy (float32, <= 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-steps", type=int, default=200)
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="gloo: CPU test hook with a stub env (not a result)")
    ap.add_argument("--layout", default="auto", choices=["auto", "quad", "oct", "hex"], help="lane layout of physics_kernel (PgttConfig.lane_layout)")
    ap.add_argument("--unsorted-variants", action="store_true", help="terrain workloads: randomize.domain_randomize(group_variants=False), i.e. the variants in per-env draw order")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short runs of the other single-GPU configs after the headline window")
    ap.add_argument("--other-steps", type=int, default=100)
    ap.add_argument("--prime-steps", type=int, default=PRIME_STEPS, help="untimed steps after the reset before the W warm-up steps and the clock (device ramp, see PRIME_STEPS)")
    return ap.parse_args(argv)


class StubEnv:
    """CPU stand-in with the surface of env.Joystick that the bench loop touches (test hook for --backend gloo)."""

    def __init__(self, n, rank):
        import torch
        from phase_guided_terrain_traversal_amd import abi
        self.num_envs = n
        self.step_block = torch.zeros((abi.NMETRIC + 2, n), dtype=torch.float32)
        self.buffers = {"done": self.step_block[abi.NMETRIC + 1], "interval_sums": torch.zeros((abi.NMETRIC + 2, n), dtype=torch.float32)}
        self._k, self._timed, self._rank = 0, 0, rank

    def reset(self, seed=0):
        self._k = 0

    def step(self, action):
        self._k += 1
        self.step_block[:-2] = action.mean()
        self.step_block[-2] = 1.0 + self._rank      # "reward": rank-dependent so the all-reduce is checkable
        self.step_block[-1] = 0.0
        self.buffers["interval_sums"] += self.step_block
        if self._timing:
            self._timed += 1
        return None, self.step_block[-2], self.step_block[-1], {}

    _timing = 0

    def enable_timing(self, on=True):
        self._timing, self._timed = int(on), 0

    def kernel_ms_mean(self):
        return 1e-3, 1e-3, max(self._timed, 1)

    def close(self):
        pass


def build_env(args, rank, world, local):
    """the workload of BASELINE.json configs[1..4] on this rank's shard -> (env, terrain, task, dr)"""
    import torch
    from phase_guided_terrain_traversal_amd import configs, mjcf
    from phase_guided_terrain_traversal_amd.env import Joystick
    from phase_guided_terrain_traversal_amd.randomize import domain_randomize
    n = args.envs
    off = rank * n
    assets = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains")
    cfg = dict(configs.training_config(), lane_layout=args.layout)
    kw, terrain, task, dr = {}, None, "stairs", False
    if args.workload == "flat":
        task = "flat_terrain"
    elif args.workload in ("level4", "curriculum"):
        # curriculum (BASELINE configs[4]): GPU r trains on stage r of the reference's level files (terrains/level*.npy)
        level = "level4" if args.workload == "level4" else "level%d" % CURRICULUM[(rank if args.stage is None else args.stage) % len(CURRICULUM)]
        terrain = np.load(os.path.join(assets, level + ".npy"))
        # the variant of every env as the PRODUCT hands it out (randomize.domain_randomize, the call train.py / evaluate.py make; DR itself off
        # in this workload): per-env draws of go2/randomize.py:97-101, ascending within blocks of 4096 global env ids - nothing is sorted here.
        # --unsorted-variants asks the same function for the draw order (the A/B of profiles/hbm_traffic.json).
        kw["variant"] = torch.from_numpy(domain_randomize(mjcf.load_model("stairs"), n, seed=2, terrain=terrain, env_id_offset=off, enable=False,
                                                          group_variants=not args.unsorted_variants, total_envs=n * max(world, 1))["variant"])
    else:
        if args.workload == "wfc_dr":           # BASELINE configs[3]: WFC-generated terrain (host, once) + full randomize.py DR
            from phase_guided_terrain_traversal_amd.terrain_gen import create_random_matrix
            terrain = create_random_matrix(100, 100, 5, 0.05, 0.13, seed=3)
        else:
            terrain = np.load(os.path.join(assets, "level13.npy"))
        dr = True
        out = domain_randomize(mjcf.load_model("stairs"), n, seed=3, terrain=terrain, env_id_offset=off, group_variants=not args.unsorted_variants,
                               total_envs=n * max(world, 1))
        kw = {"variant": torch.from_numpy(out["variant"]), "params": torch.from_numpy(out["params"]),
              "box_friction": torch.from_numpy(out["box_friction"])}
    env = Joystick(task, cfg, num_envs=n, terrain=terrain, device=f"cuda:{local}", autoreset=True, env_id_offset=off, interval_sums=True, **kw)
    return env, cfg, terrain, task, dr


WORKLOAD_TEXT = {
    "level4": "4096 Go2 envs/GPU, terrains/level4.npy (100 variants x 100 boxes) + 13x9 height scan, no DR (BASELINE configs[2])",
    "flat": "4096 Go2 envs/GPU, plane only, no DR (BASELINE configs[1])",
    "level13_dr": "Go2 envs/GPU, level13 + full randomize.py DR (BASELINE configs[3] shape)",
    "curriculum": "Go2 envs/GPU, rank r on stage r of terrains/level{1,2,3,4,7,10,13}.npy + height scan, no DR (BASELINE configs[4])",
    "wfc_dr": "Go2 envs/GPU, WFC-generated stairs (terrain_gen.py, 100 variants) + full randomize.py DR (BASELINE configs[3])"}
# the other single-GPU configurations of BASELINE.json, timed for a few steps after the headline window (world == 1 only)
OTHER_CONFIGS = [("flat", 4096, "BASELINE configs[1]"), ("wfc_dr", 8192, "BASELINE configs[3]"), ("level4", 32768, "single-GPU saturation of configs[2]")]


def timed_window(env, n, steps, warmup, dev, rank, world, stub, sync, prime_steps=PRIME_STEPS, keep_outputs=False):
    """prime every code path, W untimed warm-up steps, then EXACTLY `steps` steps between barrier + synchronize on both sides.
    -> dict(dt = max-over-ranks wall seconds, ranks, physics_ms, observe_ms, launches, gemv_ms, env_steps
    [, outputs = host copies of what the last timed step returned, keep_outputs only])"""
    import torch
    import torch.distributed as dist
    from phase_guided_terrain_traversal_amd.distributed import MetricReducer
    env.reset(seed=0)
    g = torch.Generator(device=dev); g.manual_seed(1 + rank)
    pool = [torch.tanh(torch.randn(n, 12, generator=g, device=dev) * 0.6) for _ in range(32)]   # tanh(N(0,0.6)), SURVEY 8d
    reducer = MetricReducer(dev)
    env_steps_seen = torch.zeros((), dtype=torch.float64, device=dev)     # sum of the all-reduced env-step counts
    sums = env.buffers["interval_sums"]          # [22 metrics; reward; done][N] running sums kept by the step kernels

    native_reduce = hasattr(env, "interval_reduce")        # the stub env of the gloo test hook has no library behind it

    def flush(nsteps):
        out = reducer.reduce_env(env, float(nsteps) * n) if native_reduce else reducer.reduce_block(sums, float(nsteps) * n)
        env_steps_seen.add_(out["env_steps"])

    last = [None]

    def run(k0, k1):
        for k in range(k0, k1):
            last[0] = env.step(pool[k % len(pool)])
            if (k + 1) % REDUCE_EVERY == 0:
                flush(REDUCE_EVERY)

    # ---- prime 1: every code path of the timed loop, whatever --warmup is (the driver runs --steps 20 --warmup 5)
    env.enable_timing(1)                                   # events recorded around the kernels of EVERY step
    untimed = max(len(pool), 2 * REDUCE_EVERY) + (100 if stub else prime_steps) + warmup     # every step taken before the clock starts
    run(0, max(len(pool), 2 * REDUCE_EVERY))               # full pass over the pool, >= 2 all-reduces
    sync()
    env.kernel_ms_mean()                                   # the read-back path of the event ring
    gemv_ms = 0.0
    if not stub:                                           # duration of one interval reduction (one launch + all-reduce), spread over its steps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(8):
            flush(0)
        e1.record(); sync()
        gemv_ms = e0.elapsed_time(e1) / 8 / REDUCE_EVERY
    # the exact sequence that stands between the warm-up steps and the clock, once, here: the first use of a torch op loads its code object
    # (~50 ms of host time each; a kernel trace of the driver's command showed the device idle for 100 ms right before the timed window
    # - and physics_kernel at 175 us instead of 166 us inside it, the clocks having dropped)
    sums.zero_(); reducer.reduce(); env_steps_seen.zero_()
    env.enable_timing(8)
    if world > 1:
        dist.barrier()
    sync()
    # ---- prime 2 + the W untimed warm-up steps of the contract, back to back: the device enters the timed window the way it runs a
    # roll-out - busy.  A gap of host-bound work here (event read-back, the eight timed reductions above) used to let it clock down just
    # before the clock started: a 20-step window then read physics_kernel at 180 us against 168 us in the 300-step window.
    env.enable_timing(8)          # every 8th step: an event record costs a few us of GPU idle
    import gc
    gc.collect(); gc_was = gc.isenabled(); gc.disable()          # no collection from here to the end of the timed window (see below)
    run(0, (100 if stub else prime_steps) + warmup)
    sums.zero_(); reducer.reduce(); env_steps_seen.zero_()               # counters back to zero (enqueued behind the warm-up steps)
    # timing counters back to zero: means are over the timed steps only - steps 4, 12, 20, ... of a long window, three steps of a short one
    # (a timed step is ~10 us longer: three event records)
    env.enable_timing(8 if steps >= 64 else (max(2, steps // 3) if steps >= 6 else 1))       # a short window still holds >= 3 samples
    if world > 1:
        dist.barrier()
    sync()
    # The window opens on an EMPTY queue (the contract's synchronize): for its first ~100 us the device runs only as far ahead as the host has launched,
    # so a host pause there - a generation-2 garbage collection, a preemption - is device idle time inside a 3.7 ms window (seen once in five runs of the
    # driver's command: 0.45 ms, 19.5 M instead of 21.8 - 22.4 M with every side row of the same line at its usual value).  No collection inside the window
    # (what `timeit` does).  (A real-time priority for the launching thread was considered and left out: a spinning FIFO thread can starve the runtime's own
    # helper threads.)  The collector is switched off before the priming steps above (a collection right here would be 10 - 50 ms of device idle time in
    # front of the window - the clocks drop) and back on behind the window.
    t0 = time.perf_counter()
    run(0, steps)
    sync()
    dt_own = time.perf_counter() - t0          # this rank's own K steps done (before it waits for the others)
    if gc_was:
        gc.enable()
    if world > 1:
        dist.barrier()
    sync()
    dt = time.perf_counter() - t0
    outputs = step_outputs(last[0]) if keep_outputs else None      # before the tail reduction below touches any buffer
    ranks, ranks_dt = 1, [dt_own]
    if steps % REDUCE_EVERY:
        flush(steps % REDUCE_EVERY)                    # the tail of the last interval (outside the clock)
    if world > 1:
        t = torch.tensor([dt, 1.0], device=dev, dtype=torch.float64)
        tm = t.clone(); dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        ts = t.clone(); dist.all_reduce(ts, op=dist.ReduceOp.SUM)
        # every rank's OWN time for its K steps, in rank order, taken before the closing barrier (the clock `dt` is taken after it and is the MAX
        # over ranks): a slow GCD or a straggling process shows as one long entry
        each = torch.zeros(world, device=dev, dtype=torch.float64); each[rank] = dt_own
        dist.all_reduce(each, op=dist.ReduceOp.SUM)
        dt, ranks, ranks_dt = float(tm[0].item()), int(round(float(ts[1].item()))), [float(x) for x in each.tolist()]
    phys_ms, obs_ms, ntimed = env.kernel_ms_mean()
    env.enable_timing(False)
    return {"dt": dt, "ranks": ranks, "ranks_dt": ranks_dt, "untimed_steps": untimed, "physics_ms": phys_ms, "observe_ms": obs_ms, "launches": ntimed, "gemv_ms": gemv_ms,
            "env_steps": float(env_steps_seen.item()), "done_frac": float(env.buffers["done"].mean().item()), "outputs": outputs}


DUMP_BYTES = 64 * 10 ** 6              # --dump-outputs: every file of one run together, .npy headers included


def step_outputs(ret):
    """env.step's return (obs dict, reward, done, info dict) -> {name: host float32 array}: obs_state, obs_privileged_state, reward, done,
    info_metrics, info_episode_metrics (the stub env of the gloo hook returns reward and done only)"""
    obs, reward, done, info = ret
    named = [(f"obs_{k}", v) for k, v in (obs or {}).items()] + [("reward", reward), ("done", done)] + [(f"info_{k}", v) for k, v in (info or {}).items()]
    return {k: v.detach().cpu().numpy().astype(np.float32) for k, v in named if v is not None}


def dump_outputs(out_dir, outputs, n, rank, world):
    """DIR/<name>.npy for every output (<name>_rank<r>.npy with several ranks).  The env axis is the one of length n (the last one of the
    [rows][N] arrays, the first one otherwise); above this rank's share of DUMP_BYTES every array keeps the same seeded sample of envs."""
    os.makedirs(out_dir, exist_ok=True)
    suffix = f"_rank{rank}" if world > 1 else ""
    total = sum(a.nbytes for a in outputs.values())
    budget = DUMP_BYTES // max(world, 1) - 8 * n - 256 * (len(outputs) + 1)       # room for env_index.npy and the headers
    if total > budget:
        keep = np.sort(np.random.default_rng(0).choice(n, max(1, int(n * budget / total)), replace=False))
        outputs = {k: np.take(a, keep, axis=a.ndim - 1 if a.shape[-1] == n else 0) for k, a in outputs.items()}
        np.save(os.path.join(out_dir, f"env_index{suffix}.npy"), keep.astype(np.float64))
    for k, a in outputs.items():
        np.save(os.path.join(out_dir, f"{k}{suffix}.npy"), np.ascontiguousarray(a))


def profile_record(workload, n):
    """counter figures measured with rocprofv3 --pmc on the same command and committed under profiles/ (hbm_traffic.json,
    tools/collect_profiles.py): HBM bytes per physics_kernel launch, VALU-busy share of the wave cycles.  -> (record, stale): the file
    carries the SHA-256 of the kernel sources its counters were measured on (native.source_sha256); when the library being timed was
    built from other sources the record is withheld ({}, True).  ({}, False) when nothing was measured for this workload."""
    from phase_guided_terrain_traversal_amd import native
    tpath = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    try:
        allrec = json.load(open(tpath))
    except Exception:
        return {}, False
    rec = allrec.get(f"{workload}_{n}", {})
    if not rec:
        return {}, False
    src = allrec.get("_source", {})
    try:
        # the guard is what the LOADED library says it was built from (pgtt_build_info(): the source hash csrc/Makefile embedded, and the build
        # flavour - a stale libpgtt.so, or PGTT_LIB pointing at a side build made from the same sources with other flags, is caught; a relink of
        # the same objects is not mistaken for another kernel).
        info = native.build_info()
        if src.get("csrc_sha256") != info.get("src") or info.get("flavor") != "product":
            return {}, True
    except Exception:
        return {}, True
    return rec, False


def isa_static():
    """static instruction mix of the headline kernel (profiles/isa_static.json, tools/isa_static.py), quoted only for the build it was counted on"""
    from phase_guided_terrain_traversal_amd import native
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "isa_static.json")))
        return d if d.get("csrc_sha256") == native.build_info().get("src") else {}
    except Exception:
        return {}


def rooflines(w, workload, n, dr, ms_per_step):
    """`roofline` (dominant kernel = physics_kernel, its OWN share of the algorithmic work), `roofline_observe`, `roofline_step`
    (whole step over the wall time per step) and `roofline_hbm`.  Flops are the dense-MJX count of SURVEY 8d - the arithmetic of the
    reference, not what this formulation executes (arrowhead M / H: about a quarter) - so `valu_busy` from the counters is the
    better reading of how busy the machine is."""
    rec, stale = profile_record(workload, n)
    traffic = rec.get("physics_bytes_per_launch")
    pf, of = ALGO_FLOP_PHYSICS * n, ALGO_FLOP_OBSERVE * n
    pb = (ALGO_BYTES_PHYSICS_DR if dr else ALGO_BYTES_PHYSICS) * n
    sb = (ALGO_BYTES_PER_ENV_STEP_DR if dr else ALGO_BYTES_PER_ENV_STEP) * n

    def line(bound, work, ms, peak, unit, scale, **extra):
        a = work / (ms * 1e-3) / scale
        return dict({"bound": bound, "achieved": a, "peak": peak, "unit": unit, "frac": a / peak}, **extra)
    isa = isa_static() if (workload, n, dr) == ("level4", 4096, False) else {}
    return {
        "roofline": line("valu_fp32", pf, w["physics_ms"], PEAK_FP32_TFLOPS, "TFLOP/s", 1e12, traffic=traffic, kernel="physics_kernel",
                         algorithmic_flop_per_env_step=ALGO_FLOP_PHYSICS, algorithmic_bytes_per_launch=pb,
                         traffic_over_algorithmic=(traffic / pb if traffic else None), valu_busy=rec.get("valu_busy"), mfma_ops=rec.get("mfma_ops"),
                         profile_stale=stale,
                         # the stated peak assumes packed fp32 (v_pk_fma_f32: two FMAs per lane per issue); this kernel's stream is almost all unpacked
                         # (-fno-slp-vectorize: pairing the scalar chains costs more registers than it saves issues), so the unpacked ceiling is the fairer one
                         frac_unpacked_ceiling=pf / (w["physics_ms"] * 1e-3) / 1e12 / PEAK_FP32_UNPACKED_TFLOPS, peak_unpacked=PEAK_FP32_UNPACKED_TFLOPS,
                         valu_packed_share=isa.get("valu_packed_share"),
                         note="FP32 vector-ALU issue / latency bound (SURVEY 8d): physics share of the dense-MJX count, 4 x 0.30 MFLOP per env-step; "
                              "MFMA deliberately unused (DESIGN 5.1); valu_busy = SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES from profiles/; valu_packed_share = "
                              "static share of v_pk_* among the kernel's vector-ALU instructions (profiles/isa_static.json)"),
        "roofline_observe": line("valu_fp32", of, w["observe_ms"], PEAK_FP32_TFLOPS, "TFLOP/s", 1e12, kernel="observe_kernel",
                                 algorithmic_flop_per_env_step=ALGO_FLOP_OBSERVE),
        "roofline_step": line("valu_fp32", ALGO_FLOP_PER_ENV_STEP * n, ms_per_step, PEAK_FP32_TFLOPS, "TFLOP/s", 1e12,
                              algorithmic_flop_per_env_step=ALGO_FLOP_PER_ENV_STEP, over="ms_per_step (wall)"),
        "roofline_hbm": line("hbm", pb, w["physics_ms"], PEAK_HBM_GBS, "GB/s", 1e9, traffic=traffic, kernel="physics_kernel",
                             step_algorithmic_bytes_per_launch=sb, step_GBps=sb / (ms_per_step * 1e-3) / 1e9),
    }


def other_configs(args, local, dev, sync):
    """configs[1], configs[3] and the single-GPU saturation point, a few steps each (same priming + barrier discipline as the
    headline; builder-side series with 200+ steps live under profiles/).  Never part of `value`."""
    import copy
    rows = []
    for workload, n, what in OTHER_CONFIGS:
        a2 = copy.copy(args); a2.workload, a2.envs = workload, n
        t0 = time.perf_counter()
        env, cfg, terrain, task, dr = build_env(a2, 0, 1, local)
        w = timed_window(env, n, args.other_steps, 5, dev, 0, 1, False, sync, args.prime_steps)
        env.close()
        ms = 1e3 * w["dt"] / args.other_steps
        r = rooflines(w, workload, n, dr, ms)
        rows.append({"workload": workload, "envs": n, "what": what, "value": w["env_steps"] / w["dt"], "unit": "env-steps/s", "steps": args.other_steps,
                     "ms_per_step": ms, "kernels_ms": {"physics_kernel": w["physics_ms"], "observe_kernel": w["observe_ms"]},
                     "wall_over_kernels": ms / (w["physics_ms"] + w["observe_ms"] + w["gemv_ms"]),
                     "roofline_frac_physics": r["roofline"]["frac"], "traffic": r["roofline"]["traffic"], "lane_layout": args.layout,
                     "setup_s": time.perf_counter() - t0 - w["dt"]})
    # BASELINE configs[4], one rank's share at a time: 4096 envs on each level file of the reference's curriculum (training/training.sh:31-58)
    for stage, lvl in enumerate(CURRICULUM):
        a2 = copy.copy(args); a2.workload, a2.envs, a2.stage = "curriculum", 4096, stage
        t0 = time.perf_counter()
        env, cfg, terrain, task, dr = build_env(a2, 0, 1, local)
        w = timed_window(env, 4096, args.other_steps, 5, dev, 0, 1, False, sync, min(args.prime_steps, 300))
        env.close()
        ms = 1e3 * w["dt"] / args.other_steps
        rows.append({"workload": "curriculum", "envs": 4096, "stage": stage, "level": f"level{lvl}", "what": "BASELINE configs[4], one rank's workload",
                     "value": w["env_steps"] / w["dt"], "unit": "env-steps/s", "steps": args.other_steps, "ms_per_step": ms,
                     "kernels_ms": {"physics_kernel": w["physics_ms"], "observe_kernel": w["observe_ms"]}, "terrain_variants": int(terrain.shape[0]),
                     "lane_layout": args.layout, "setup_s": time.perf_counter() - t0 - w["dt"]})
    rows.append(graph_row(args, local, dev, sync))
    rows.append(rollout_row(args, local, dev, sync))
    rows.append(fastdiv_build_row(args))
    return rows


def graph_row(args, local, dev, sync):
    """the headline step loop as the reference runs its own: ONE device program per unroll (training/train.py:142 jits 20 env steps into a single
    XLA executable).  Here: REDUCE_EVERY = 20 control steps (20 different action batches of the pool) + the interval reduction captured once
    into a HIP graph, the timed window = replays of it.  No per-step launch gap, no event records: what is left is the kernels.  Never part of `value`."""
    import copy
    import torch
    a2 = copy.copy(args); a2.workload, a2.envs = "level4", 4096
    n, T = a2.envs, REDUCE_EVERY
    replays = max(1, max(200, args.other_steps) // T)
    row = {"workload": "graph", "envs": n, "what": f"headline workload, {T} control steps + interval reduction captured as ONE HIP graph, {replays} replays",
           "steps": replays * T, "steps_per_graph": T, "lane_layout": args.layout}
    env = None
    try:
        t0 = time.perf_counter()
        env, cfg, terrain, task, dr = build_env(a2, 0, 1, local)
        env.reset(seed=0)
        g = torch.Generator(device=dev); g.manual_seed(1)
        pool = [torch.tanh(torch.randn(n, 12, generator=g, device=dev) * 0.6) for _ in range(T)]
        out = torch.zeros(env.buffers["interval_sums"].shape[0] + 1, dtype=torch.float32, device=dev)
        total = torch.zeros_like(out)

        def unroll():
            for k in range(T):
                env.step(pool[k])
            env.interval_reduce(out, float(T) * n)
            total.add_(out)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            unroll()
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            unroll()
        for _ in range(max(1, min(args.prime_steps, 1500) // T)):
            graph.replay()
        total.zero_()
        sync()
        t1 = time.perf_counter()
        for _ in range(replays):
            graph.replay()
        sync()
        dt = time.perf_counter() - t1
        counted = float(total[-1].item())
        row.update(value=counted / dt, unit="env-steps/s", ms_per_step=1e3 * dt / (replays * T), env_steps_counted=counted,
                   env_steps_expected=float(n) * replays * T, setup_s=time.perf_counter() - t0 - dt)
    except Exception as e:          # a side row must never cost the headline line
        row["skipped"] = f"{type(e).__name__}: {e}"
        try:
            torch.cuda.synchronize()          # a poisoned capture surfaces HERE, not in the row that runs next
        except Exception as e2:
            row["skipped"] += f" / then {type(e2).__name__}: {e2}"
    finally:
        if env is not None:
            env.close()
    return row


def rollout_row(args, local, dev, sync):
    """the hot path inside the loop its caller runs (training/train.py:135-161 -> Brax generate_unroll): the reference-trained policy177
    (deploy/policy_net.py:36-71: normalise, 171-512-256-128-24 SiLU MLP, tanh-normal head) SAMPLES an action for every env, the env steps,
    reward / done / truncation and the finished-episode sums are recorded - four launches per acting step (acting.FusedActor: pgtt_policy_act
    on fp32 MFMA, physics_kernel, observe_kernel, pgtt_rollout_record), ONE captured HIP graph replayed per step, roll-outs of 20 steps
    (unroll_length).  Headline workload, same priming discipline.  Never part of `value`."""
    import copy
    import torch
    from phase_guided_terrain_traversal_amd import policy
    from phase_guided_terrain_traversal_amd.acting import FusedActor
    a2 = copy.copy(args); a2.workload, a2.envs = "level4", 4096
    T, steps = REDUCE_EVERY, max(200, args.other_steps)
    row = {"workload": "rollout", "envs": a2.envs, "what": "policy177 forward + sample + env.step + bookkeeping, one HIP graph per acting step, level4 (N1: caller of the hot path)",
           "steps": steps, "unroll_length": T, "lane_layout": args.layout, "launches_per_step": 4}
    env = None
    try:
        t0 = time.perf_counter()
        env, cfg, terrain, task, dr = build_env(a2, 0, 1, local)
        net = policy.load_policy("policy177", device=f"cuda:{local}")
        fa = FusedActor(env, T=T, seed=1)
        fa.load([(l.weight, l.bias) for l in net.layers], net.mean, net.std)
        env.reset(seed=0)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fa.step()
        torch.cuda.current_stream(dev).wait_stream(side)
        fa.rewind()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fa.step()
        fa.rewind()

        def run(k):
            for i in range(k):
                g.replay()
                if (i + 1) % T == 0:
                    fa.rewind()                     # the learner would consume the [T, N] batch here
        run(max(args.prime_steps, T) // T * T)
        fa.episode_sums.zero_()
        sync()
        t1 = time.perf_counter()
        run(steps // T * T)
        sync()
        dt = time.perf_counter() - t1
        n_steps = steps // T * T
        es = fa.episode_sums.cpu().numpy()
        row.update(value=a2.envs * n_steps / dt, unit="env-steps/s", steps=n_steps, ms_per_step=1e3 * dt / n_steps,
                   episodes_finished=float(es[-1]), mean_episode_length=float(es[-2] / max(es[-1], 1.0)), setup_s=time.perf_counter() - t0 - dt)
    except Exception as e:          # a caller-side row must never cost the headline line
        row["skipped"] = f"{type(e).__name__}: {e}"
        try:
            torch.cuda.synchronize()
        except Exception as e2:
            row["skipped"] += f" / then {type(e2).__name__}: {e2}"
    finally:
        if env is not None:
            env.close()
    return row


def fastdiv_build_row(args):
    """the headline workload once more on libpgtt_fastdiv.so (csrc/Makefile `make fastdiv`: fp32 division / square root as v_rcp / v_sqrt + one
    refinement, 1 ulp - the product rounds them correctly, as XLA does for the reference) in a process of its own (PGTT_LIB is read when the
    package loads its library): what correct rounding costs stays visible in the driver's line.  Never part of `value`."""
    lib = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "libpgtt_fastdiv.so")
    row = {"workload": args.workload, "envs": args.envs, "what": "headline workload on the 1-ulp division / square-root side build (libpgtt_fastdiv.so; NOT the product)",
           "fp32_div_sqrt": "1ulp", "steps": args.other_steps, "lane_layout": args.layout}
    if not os.path.exists(lib):
        return dict(row, skipped="libpgtt_fastdiv.so not built (__graft_entry__.build() makes it)")
    cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.other_steps), "--warmup", "5", "--envs", str(args.envs), "--workload", args.workload,
           "--layout", args.layout, "--prime-steps", str(args.prime_steps), "--no-cpu-baseline", "--no-other-configs"] + (["--unsorted-variants"] if args.unsorted_variants else [])
    try:
        t0 = time.perf_counter()
        r = subprocess.run(cmd, env=dict(os.environ, PGTT_LIB=lib), capture_output=True, text=True, timeout=600)
        d = json.loads(r.stdout.strip().splitlines()[-1])
        return dict(row, value=d["value"], unit=d["unit"], ms_per_step=d["ms_per_step"], kernels_ms={k: d["kernels_ms"][k] for k in ("physics_kernel", "observe_kernel")},
                    wall_over_kernels=d["wall_over_kernels"], roofline_frac_physics=d["roofline"]["frac"], setup_s=time.perf_counter() - t0)
    except Exception as e:          # a side build must never cost the headline line
        return dict(row, skipped=f"{type(e).__name__}: {e}")


def worker(args):
    import torch
    import torch.distributed as dist
    from phase_guided_terrain_traversal_amd.distributed import MetricReducer, init_from_env

    stub = args.backend == "gloo"
    rank, local, world = init_from_env(args.backend)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torchrun --nproc-per-node {args.gpus} "
                         f"(or run `python bench.py --gpus {args.gpus}` without a torchrun environment: it spawns the ranks)")
    if stub:
        dev = torch.device("cpu")
        env, cfg, terrain, task, dr = StubEnv(args.envs, rank), None, None, "stub", False
        sync = lambda: None
    else:
        if not torch.cuda.is_available() or torch.cuda.device_count() <= local:
            raise SystemExit(f"rank {rank}: no GPU {local} (device_count = {torch.cuda.device_count() if torch.cuda.is_available() else 0}); "
                             "the bench has no CPU path")
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
        env, cfg, terrain, task, dr = build_env(args, rank, world, local)
        sync = torch.cuda.synchronize
    n = args.envs
    w = timed_window(env, n, args.steps, args.warmup, dev, rank, world, stub, sync, args.prime_steps, keep_outputs=args.dump_outputs is not None)
    dt, ranks, env_steps = w["dt"], w["ranks"], w["env_steps"]
    env.close()
    if args.dump_outputs is not None:
        dump_outputs(args.dump_outputs, w["outputs"], n, rank, world)

    rc = 0
    if rank == 0:
        value = env_steps / dt               # env-steps the all-reduce counted over ALL ranks / max-over-ranks wall time
        ms_per_step = 1e3 * dt / args.steps
        kern = w["physics_ms"] + w["observe_ms"] + w["gemv_ms"]
        ratio = ms_per_step / kern
        out = {
            "metric": "env-steps/sec at 4096 envs (Go2, level4 hfield), 1/2/4/8 MI355X",
            "value": value, "unit": "env-steps/s", "n_gpus": ranks, "steps": args.steps, "warmup": args.warmup, "untimed_steps": w["untimed_steps"],
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": WORKLOAD_TEXT[args.workload],
                       "envs_per_gpu": n, "substeps": 4, "autoreset": True, "actions": "tanh(N(0,0.6)) iid", "parallelism": f"env-shard x{world}",
                       "lane_layout": args.layout, "prime_steps": args.prime_steps, "untimed_steps_before_clock": w["untimed_steps"],
                       "terrain_variants": ("per-env draws in draw order (--unsorted-variants)" if args.unsorted_variants else
                                            "randomize.domain_randomize default: per-env draws, ascending within blocks of 4096 global env ids"),
                       "collective": f"fused {MetricReducer.SIZE}-float all-reduce every {REDUCE_EVERY} steps ({args.backend})"},
            "env_steps_allreduced": env_steps, "env_steps_expected": float(n) * world * args.steps,
            "kernels_ms": {"physics_kernel": w["physics_ms"], "observe_kernel": w["observe_ms"], "interval_reduce_per_step": w["gemv_ms"], "launches": w["launches"]},
            "ranks_dt": w["ranks_dt"], "wall_over_kernels": ratio, "cold": bool(ratio > COLD_RATIO),
            "done_fraction_last_step": w["done_frac"],
        }
        if stub:
            out.update(stub=True, roofline=None, roofline_hbm=None, kernels_ms=None)
        else:
            out.update(rooflines(w, args.workload, n, dr, ms_per_step))
        if env_steps != float(n) * world * args.steps or ranks != world:
            out["error"] = f"all-reduce saw {env_steps} env-steps from {ranks} ranks, expected {float(n) * world * args.steps} from {world}"
            rc = 4
        if world == 1 and not stub and args.full and not args.no_other_configs:
            out["other_configs"] = other_configs(args, local, dev, sync)
        if world == 1 and args.full and not args.no_cpu_baseline and not stub:
            out["cpu_baseline"] = cpu_baseline(args, cfg, terrain, task, n)
        print(json.dumps(out), flush=True)
        if out["cold"] and not stub:
            print(f"bench.py: wall time is {ratio:.2f} x the kernel time: the timed window is not kernel-bound (cold code or host-bound launch loop)", file=sys.stderr)
            rc = rc or 3
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return rc


def host_cores():
    """Usable host cores: the smaller of the affinity mask and the cgroup CPU quota (the GPU box shows 256 CPUs
    but grants a 16-CPU quota)."""
    c = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            c = min(c, max(1, int(round(int(q) / int(p)))))
    except Exception:
        pass
    return c


def cpu_baseline(args, cfg, terrain, task, n):
    """The build's CPU restatement (oracle/, fp32, OpenMP over envs) on a bounded sample of the same workload.
    Built ON THIS HOST with -O3 -march=native (`make -C oracle fast`), which cannot travel between
    machines; when no compiler is at hand the portable -O2 build the tests use is timed and the line says so."""
    from oracle import oracle
    from phase_guided_terrain_traversal_amd import abi, mjcf
    cores = host_cores()
    flags = oracle.use_fast_build()
    cfg2 = dict(cfg); cfg2["autoreset"] = 1
    cs, ms = abi.config_struct(cfg2), abi.model_struct(mjcf.load_model(task))
    hb = oracle.HostBuffers(n, with_variant=terrain is not None, debug=False)
    if terrain is not None:
        from phase_guided_terrain_traversal_amd.randomize import domain_randomize
        hb["variant"][:] = domain_randomize(mjcf.load_model("stairs"), n, seed=2, terrain=terrain, enable=False, group_variants=not args.unsorted_variants)["variant"]
    oracle.reset(cs, ms, terrain, hb, seed=0, nthreads=cores)
    rng = np.random.default_rng(1)
    acts = [np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32) for _ in range(8)]
    for k in range(3):
        oracle.step(cs, ms, terrain, hb, acts[k % 8], seed=0, nthreads=cores)
    t0 = time.perf_counter()
    for k in range(args.cpu_sample_steps):
        oracle.step(cs, ms, terrain, hb, acts[k % 8], seed=0, nthreads=cores)
    dt = time.perf_counter() - t0
    return {"value": n * args.cpu_sample_steps / dt, "unit": "env-steps/s", "cores": cores, "per_core": n * args.cpu_sample_steps / dt / cores, "kind": "port",
            "sample": f"{n} envs x {args.cpu_sample_steps} control steps of the same workload ({args.workload}), fp32 oracle ({flags}), OpenMP over envs, {dt:.1f} s"}


def _spawned(i, argv, port, n):
    os.environ.update(RANK=str(i), LOCAL_RANK=str(i), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    rc = worker(parse_args(argv))
    if rc:
        sys.exit(rc)


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` outside torchrun: one process per GPU, rendezvous on 127.0.0.1"""
    import torch
    import torch.multiprocessing as mp
    if args.backend == "nccl":
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: this node has {have} GPU(s); refusing to run fewer ranks than asked for")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_spawned, args=(argv, port, args.gpus), nprocs=args.gpus, join=True)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args, argv)
        return 0
    return worker(args)


if __name__ == "__main__":
    sys.exit(main())
