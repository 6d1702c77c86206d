"""In-run terrain curriculum, host side: the stacked multi-level terrain table, the initial per-env labels, and a plain numpy
restatement of the decision rule that `curriculum_kernel` (csrc/pgtt_curriculum.hip, `pgtt_curriculum` in include/pgtt.h) applies on the GPU.

    table, level_start = stack_levels([level1, level4, level7])         # (sum T_l, B, 10), level l owns variants [level_start[l], level_start[l + 1])
    env = Joystick("stairs", cfg, terrain=[level1, level4, level7], curriculum=dict(promote_tracking=0.65, demote_length=0.5, init_level=0),
                   autoreset=True, ...)

The rule, per env and at the end of each episode (the "game-inspired" curriculum of legged_gym / Isaac Lab, on the sums the step keeps anyway):
a TRUNCATED episode (it reached episode_length) whose mean unscaled tracking_lin_vel term is at least `promote_tracking` moves the env one level
up; an episode TERMINATED before `demote_length * episode_length` steps moves it one level down; both clamp at the ends of the ladder.  The env
then restarts from a fresh `Joystick.reset` on a variant drawn uniformly inside its (new) level.  `replay` is documentation and the host reference
of the tests; nothing on the hot path calls it.  The reference (go2/, training/) has no curriculum: its ladder is three runs of training.sh.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from . import abi

PARK = 100.0            # unused boxes of a variant sit at (PARK + k) m on all three axes (terrain_gen.create_random_matrix, the shipped level files)


def stack_levels(tables: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """L level tables (T_l, B_l, 10) -> ((sum T_l, max B_l, 10) float32 table, level_start [L + 1] int32).  A level with fewer boxes per variant is
    padded with parked unit boxes (identity quaternion, half sizes 1, centre 100 + k m: beyond the 50 m within which pgtt_set_terrain takes a box
    for a placed one).  The levels' own rows are copied bit for bit."""
    tables = [np.asarray(t) for t in tables]
    if not 1 <= len(tables) <= abi.MAX_LEVELS:
        raise ValueError(f"stack_levels: 1 .. {abi.MAX_LEVELS} levels, got {len(tables)}")
    for t in tables:
        if t.ndim != 3 or t.shape[2] != 10 or t.shape[0] < 1 or not 1 <= t.shape[1] <= abi.MAX_BOX:
            raise ValueError(f"stack_levels: a level table is (T >= 1, 1 <= B <= {abi.MAX_BOX}, 10), got {t.shape}")
    B = max(t.shape[1] for t in tables)
    level_start = np.concatenate([[0], np.cumsum([t.shape[0] for t in tables])]).astype(np.int32)
    out = np.empty((int(level_start[-1]), B, 10), dtype=np.float32)
    for t, v0 in zip(tables, level_start[:-1]):
        T, b = t.shape[:2]
        out[v0:v0 + T, :b] = t.astype(np.float32, copy=False)
        if b < B:
            k = (np.arange(T)[:, None] * B + np.arange(b, B)[None, :]).astype(np.float32)
            pad = np.ones((T, B - b, 10), dtype=np.float32)
            pad[..., :3] = (PARK + k)[..., None]
            pad[..., 3:7] = [1, 0, 0, 0]
            out[v0:v0 + T, b:] = pad
    return out, level_start


def pick_variant(u, level, level_start) -> np.ndarray:
    """level_start[l] + min(int(u * T_l), T_l - 1) in fp32, the kernel's expression"""
    ls = np.asarray(level_start, dtype=np.int64)
    level = np.asarray(level, dtype=np.int64)
    T = ls[level + 1] - ls[level]
    k = (np.asarray(u, dtype=np.float32) * T.astype(np.float32)).astype(np.int64)
    return (ls[level] + np.minimum(k, T - 1)).astype(np.int32)


def replay(done, ep_steps, ep_metrics, level, variant, u, level_start, episode_length: int, tracking_scale: float,
           promote_tracking: float = 0.65, demote_length: float = 0.5) -> Dict[str, np.ndarray]:
    """What pgtt_curriculum decides for one batch.  done [N] (non-zero = the step just taken finished the episode), ep_steps [N]
    (istate[I_EP_STEPS]), ep_metrics [NMETRIC + 2, N] (the episode sums as the step left them), level / variant [N], u [N] the uniform draws
    uniform(seed, global env id, epoch after the step, RS_CURRICULUM, 0).  Returns the new level and variant (unchanged where done == 0), the
    reset mask and the increments of PgttCurriculum.stats.  fp32 where the kernel computes in fp32."""
    f32 = np.float32
    L = len(level_start) - 1
    fin = np.asarray(done) != 0
    steps = np.asarray(ep_steps, dtype=np.int64)
    lvl = np.clip(np.asarray(level, dtype=np.int64), 0, L - 1)
    epm = np.asarray(ep_metrics, dtype=f32)
    length, scale = epm[abi.NMETRIC + 1], f32(tracking_scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        trk = np.where((length > 0) & (scale != 0), epm[abi.REWARD_KEYS.index("tracking_lin_vel")] / (length * scale), f32(0)).astype(f32)
    truncated = steps >= int(episode_length)
    up = fin & truncated & (trk >= f32(promote_tracking))
    down = fin & ~truncated & (steps.astype(f32) < f32(demote_length) * f32(episode_length))
    new = np.where(up, np.minimum(lvl + 1, L - 1), np.where(down, np.maximum(lvl - 1, 0), lvl))
    stats = np.zeros(abi.NCSTAT, dtype=np.int32)
    stats[:L] = np.bincount(lvl[fin], minlength=L)                  # counted on the level the episode was played on
    stats[abi.CS_PROMOTED] = int((fin & (new > lvl)).sum())         # moves, not attempts the clamp swallowed
    stats[abi.CS_DEMOTED] = int((fin & (new < lvl)).sum())
    stats[abi.CS_FINISHED] = int(fin.sum())
    return {"level": np.where(fin, new, np.asarray(level)).astype(np.int32),
            "variant": np.where(fin, pick_variant(u, new, level_start), np.asarray(variant)).astype(np.int32),
            "mask": fin.astype(np.uint8), "stats": stats}


def initial_labels(seed: int, first_env: int, n: int, level_start, init_level=0) -> Tuple[np.ndarray, np.ndarray]:
    """(level [n], variant [n]) int32 of the envs with GLOBAL ids first_env .. first_env + n - 1: `init_level` an int (every env there) or (lo, hi)
    (uniform over lo .. hi inclusive), the variant uniform inside the env's level.  ONE numpy Philox stream per seed in which env e owns one counter
    step, so a shard draws what the full batch draws."""
    L = len(level_start) - 1
    lo, hi = (int(init_level), int(init_level)) if np.isscalar(init_level) else (int(init_level[0]), int(init_level[1]))
    if not 0 <= lo <= hi < L:
        raise ValueError(f"curriculum init_level {init_level!r} outside the ladder's levels 0 .. {L - 1}")
    bg = np.random.Philox(key=[int(seed), 0x5047_4355])
    bg.advance(int(first_env))
    U = np.random.Generator(bg).random((n, 4))
    level = np.minimum(lo + (U[:, 0] * (hi - lo + 1)).astype(np.int64), hi)
    return level.astype(np.int32), pick_variant(U[:, 1].astype(np.float32), level, level_start)
