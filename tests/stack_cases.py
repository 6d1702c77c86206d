"""The full sensing stacks of one control step and the schedule they are walked through: what tests/test_gpu_stack.py runs on the GPU and
tests/test_stack_cases.py shows, without one, to be what it claims.  No test functions, no GPU.

A stack is a dict of Joystick keyword arguments (STACKS); kwargs() adds what every stack shares - task `stairs`, episode_length 6, autoreset, N = 37
envs at env_id_offset 1000 (ragged for the quad, oct and hex lane layouts alike), full domain randomisation - or the rows [lo, hi) of it as a shard.
The image and ray counts leave the 256-lane loops a partly filled last pass; the camera's 260 pixels are a multiple of 4 (the ring's 16-byte
copies) and the LiDAR's 810 floats per frame are not (its dword copies).  The camera-fed maps are given a cell size that puts ground the camera sees
inside the window (2.4 m of 10 cm cells, 1.8 m of 20 cm cells: at the default 4 cm the self filter's 0.45 m box covers all a window of 9 or 24
cells holds in front of the robot, and the map stays empty), and the first one keeps the clean-up's bound layer, whose floats show which pose the
rays were cast from.

The schedule is integers alone.  schedule(name) lists the 20 calls - reset(seed), three steps, reset(seed + 1, mask = odd envs), a warm-up step, R = 14
measured steps - and says for each, from episode_length, the mask, the sensors' `every` and the ring's size, which envs it clears, which sensors take
new data, which ring slot it pushes and, through the Philox draw of include/pgtt_elevation.h, every env's latency and `fused` flag.  Every device
counter of the stack (the camera's, the LiDAR's, the odometry's, the ring's) stands at the call's index when the call is made."""
import os

import numpy as np
import torch

import depth_reference as dref

from phase_guided_terrain_traversal_amd import configs, curriculum, mjcf, perceive
from phase_guided_terrain_traversal_amd.randomize import domain_randomize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERRAINS = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains")
N, OFFSET, EPISODE = 37, 1000, 6
EAGER, R = 3, 14                                   # steps between the two resets, measured steps
SEED, DR_SEED, ACTION_SEED = 5, 3, 11
RS_LATENCY = 35                                    # include/pgtt_elevation.h
PUSH = dict(wait=(0.05, 0.3), duration=(0.04, 0.3), velocity=(0.0, 1.5))                           # tests/test_gpu_push.py
CURRICULUM = dict(promote_tracking=0.3, demote_length=0.6, init_level=(0, 2), seed=8)               # tests/test_gpu_curriculum.py
LADDER_NAMES = ("level1", "level2", "level4")                                                       # its three levels: 100 + 50 + 100 variants


def _level(name):
    return np.load(os.path.join(TERRAINS, name + ".npy"))


def ladder():
    return [_level(n) for n in LADDER_NAMES]


def student(height, width, memory, seed):
    """a small estimator for height x width images, He-normal weights and biases 0.1 N(0, 1) as tests/test_gpu_perceive_memory.py draws them (the
    GRU's two matrices too); memory = 0: feed-forward"""
    est = perceive.ScanEstimator(perceive.config(memory=memory, height=height, width=width, conv=[(16, 5, 2), (32, 3, 1)], hidden=64))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        pairs = [(m.weight, m.bias) for m in est.layers()]
        if memory:
            pairs += [(est.gru.weight_ih, est.gru.bias_ih), (est.gru.weight_hh, est.gru.bias_hh)]
        for w, b in pairs:
            w.copy_(torch.randn(w.shape, generator=g) * (2.0 / w[0].numel()) ** 0.5)
            b.copy_(torch.randn(b.shape, generator=g) * 0.1)
    return est


STACKS = {
    "camera": dict(
        depth=dict(width=20, height=13, noise=dict(sigma=0.01, dropout=0.02, seed=3)),
        student=student(13, 20, 32, 14),
        elevation=dict(grid=24, res=0.1, variance=True, visibility=True, dense_bound=True, odometry=dict(sigma_xy=0.2, sigma_yaw=0.1, seed=5), fill=4,
                       dense=True),
        push=PUSH, interval_sums=True),
    "late_lidar": dict(
        lidar=dict(n_az=30, n_el=9, noise=dict(sigma=0.01, dropout=0.02, seed=7)),
        elevation=dict(grid=24, source="lidar", latency=(0, 2), odometry=True, fill=4),
        curriculum=dict(CURRICULUM)),
    "slow_camera": dict(
        depth=dict(width=21, height=13, every=3),
        lidar=dict(n_az=16, n_el=6, every=2),
        student=student(13, 21, 0, 15),
        elevation=dict(grid=9, res=0.2, follow_sensor=True, odometry=True, fill=2)),
}


def config():
    return configs.with_overrides(configs.training_config(), episode_length=EPISODE)


def randomisation(name):
    """the domain randomisation of all N envs of a stack, drawn by global env id: rows of it are a shard's"""
    if "curriculum" in STACKS[name]:
        table, start = curriculum.stack_levels(ladder())
        return domain_randomize(mjcf.load_model("stairs"), N, seed=DR_SEED, terrain=table, env_id_offset=OFFSET, total_envs=OFFSET + N,
                                level_start=start, init_level=CURRICULUM["init_level"])
    return domain_randomize(mjcf.load_model("stairs"), N, seed=DR_SEED, terrain=_level("level4"), env_id_offset=OFFSET, total_envs=OFFSET + N)


def kwargs(name, lo=0, hi=N, offset=None, device="cuda:0", without=()):
    """Joystick's keyword arguments for the envs [lo, hi) of stack `name`: their rows of the randomisation, their global ids (`offset` overrides
    the id of row lo, for a control that must fail); `without`: keys of the stack to leave out (a twin without its map)"""
    dr = randomisation(name)
    kw = {k: v for k, v in STACKS[name].items() if k not in without}
    kw.update(task="stairs", config=config(), num_envs=hi - lo, device=device, autoreset=True, env_id_offset=OFFSET + lo if offset is None else offset,
              terrain=ladder() if "curriculum" in kw else _level("level4"),
              params=torch.from_numpy(np.ascontiguousarray(dr["params"][:, lo:hi])),
              box_friction=torch.from_numpy(np.ascontiguousarray(dr["box_friction"][:, lo:hi])),
              variant=torch.from_numpy(np.ascontiguousarray(dr["variant"][lo:hi])))
    if "curriculum" in kw:
        kw["level"] = torch.from_numpy(np.ascontiguousarray(dr["level"][lo:hi]))
    return kw


def odd_mask():
    return (np.arange(N) % 2 == 1).astype(np.uint8)


def actions():
    """[EAGER + 1 + R, N, 12] float32: tanh(0.6 normal) from one fixed generator, in the order the steps are made"""
    rng = np.random.default_rng(ACTION_SEED)
    return np.tanh(0.6 * rng.normal(size=(EAGER + 1 + R, N, 12))).astype(np.float32)


def latency_draw(seed, gids, counter, lo, hi):
    """the header's integer rule: lat = lo + ((w0 * (hi - lo + 1)) >> 32), w0 = word 0 of the Philox block (gid, (uint32) counter, RS_LATENCY, 0)
    under the key (seed lo, seed hi) -> [len(gids)] ints"""
    ctr = np.zeros((len(gids), 4), np.uint32)
    ctr[:, 0] = np.asarray([int(g) & 0xFFFFFFFF for g in gids], np.uint32)
    ctr[:, 1], ctr[:, 2] = int(counter) & 0xFFFFFFFF, RS_LATENCY
    w = dref.philox4x32_10((int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF), ctr)
    return np.array([int(lo) + ((int(w0) * (int(hi) - int(lo) + 1)) >> 32) for w0 in w[:, 0]], np.int64)


def latency_replay(clears, lo, hi, D, seed, gids):
    """the ring's bookkeeping over calls 0, 1, ... that clear the envs clears[c] ([calls, n] bool; call c finds the counter at c)
    -> (lat, age, fused), each [calls, n], as the call leaves them: a cleared env draws its latency and starts at age 0, every call pushes one frame
    (age saturates at D), and a frame is fused when lat < age"""
    clears = np.asarray(clears, bool)
    lat, age = np.zeros(clears.shape[1], np.int64), np.zeros(clears.shape[1], np.int64)
    out = [], [], []
    for c, clear in enumerate(clears):
        if clear.any():
            lat[clear] = latency_draw(seed, np.asarray(gids)[clear], c, lo, hi)
            age[clear] = 0
        age = np.minimum(age + 1, D)
        for o, v in zip(out, (lat, age, lat < age)):
            o.append(v.copy())
    return tuple(np.stack(o) for o in out)


def latency_range(name):
    """(lo, hi, D, seed) of a stack's latency, or None"""
    lat = STACKS[name]["elevation"].get("latency")
    if lat is None:
        return None
    lo, hi = (lat, lat) if isinstance(lat, int) else lat
    return int(lo), int(hi), int(hi) + 1, 0


def schedule(name, n=N, offset=OFFSET):
    """the calls of the walk and what each must do, for the envs with the global ids offset .. offset + n - 1 counted from OFFSET (a shard's rows of
    the whole) -> dict:
        calls      [(kind, step index or None)] with kind "reset" | "step": 20 entries; the k-th step takes actions()[k]
        measured   the indices of the R measured calls
        mask       [n] uint8, the second reset's
        clears     [calls, n] bool: the envs a call clears - a reset's mask, a step's truncations (an env that falls earlier ends its episode
                   earlier than this says: the device's done flag is set AT LEAST where clears says)
        fresh      {"depth" | "lidar": [calls] bool}: the sensor takes new data (a reset forces it; a step when counter mod every == 0)
        map_fresh  [calls] bool: `fresh` of the sensor that feeds the map
        slot       [calls] ring slot pushed (counter mod D), None without a latency;  wraps [calls] bool: the slot is 0 again
        latency, fused   [calls, n] from latency_replay under `clears`, None without a latency"""
    stack = STACKS[name]
    first = offset - OFFSET
    mask = odd_mask()[first:first + n]
    calls = [("reset", None)] + [("step", k) for k in range(EAGER)] + [("reset", None)] + [("step", k) for k in range(EAGER, EAGER + 1 + R)]
    measured = list(range(len(calls) - R, len(calls)))
    clears, steps = np.zeros((len(calls), n), bool), np.zeros(n, np.int64)
    resets = 0
    for c, (kind, _) in enumerate(calls):
        if kind == "reset":
            clears[c] = True if resets == 0 else mask != 0
            resets += 1
            steps[clears[c]] = 0
        else:
            steps += 1
            clears[c] = steps >= EPISODE                  # the AutoReset wrapper: the step that makes it episode_length ends the episode
            steps[clears[c]] = 0
    fresh = {}
    for key in ("depth", "lidar"):
        if key in stack:
            every = int(stack[key].get("every", 1))
            fresh[key] = np.array([kind == "reset" or c % every == 0 for c, (kind, _) in enumerate(calls)])
    source = stack["elevation"].get("source", "depth")
    out = dict(calls=calls, measured=measured, mask=mask, clears=clears, fresh=fresh, map_fresh=fresh[source], slot=None, wraps=np.zeros(len(calls), bool),
               latency=None, fused=None)
    rng = latency_range(name)
    if rng is not None:
        lo, hi, D, seed = rng
        out["slot"] = np.arange(len(calls)) % D
        out["wraps"] = (out["slot"] == 0) & (np.arange(len(calls)) > 0)
        out["latency"], _, out["fused"] = latency_replay(clears, lo, hi, D, seed, offset + np.arange(n))
    return out
