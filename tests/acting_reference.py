"""An fp64 statement of the two acting kernels (policy_act_kernel, rollout_record_kernel), written from include/pgtt_train.h and the comment
header of csrc/pgtt_policy.hip and from nothing in acting.py or ppo.py.  A helper module like depth_reference.py and ppo_reference.py:
test_acting_reference.py holds it to facts that do not come from the kernel (CPU), test_gpu_acting_edges.py holds the kernels to it.
numpy in, numpy fp64 out; the head formulas are ppo_reference's (torch.float64 inside).

    draw     Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter ((env_id_offset + e) mod 2^32, draw & 0xffffffff,
             (draw >> 32) ^ 0x50475454, j >> 1) -> words w0 .. w3;   u1 = ((float)(w0 >> 8) + 0.5f) 2^-24,   u2 = (float)(w1 >> 8) 2^-24,
             theta = 6.28318530717958648f u2 (fp32),   r = sqrt(-2 ln u1),   eps_j = r cos(theta) (j even) | r sin(theta) (j odd)
    head     out = MLP((obs - mean) / std),   loc, raw = out[:12], out[12:],   scale = softplus(raw) + 1e-3,   u = loc + scale eps (or loc),
             act = tanh(u),   logp = ppo_reference.log_prob
    record   row t = counters[0] (only if 0 <= t < T): reward * reward_scaling, done, truncation = ep_steps >= L and not (up_z < 0);
             episode_sums[0 .. 23] += sum over done envs of ep_metrics[k], [24] += their count;   both counters + 1
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_reference  # noqa: E402
from depth_reference import philox4x32_10  # noqa: E402

A = 12                                   # actuators
NSUMS = 25                               # 22 metric sums, return, length, count
DRAW_DOMAIN = 0x50475454                 # xor'ed into the high counter word
TWO_PI_F32 = np.float32(6.28318530717958648)
F32_2M24 = np.float32(2.0 ** -24)


# ---------------------------------------------------------------- the draws
def uniforms(w0, w1):
    """the two uniforms of a Philox block, in float32 as the header states them: u1 = ((float)(w0 >> 8) + 0.5f) 2^-24 in (0, 1] (the + 0.5f is a
    tie for w0 >> 8 >= 2^23 and goes to the even neighbour, so u1 == 1 for w0 >> 8 == 2^24 - 1), u2 = (float)(w1 >> 8) 2^-24 in [0, 1)"""
    w0, w1 = np.asarray(w0, np.uint32), np.asarray(w1, np.uint32)
    u1 = ((w0 >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * F32_2M24
    u2 = (w1 >> np.uint32(8)).astype(np.float32) * F32_2M24
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    return u1, u2


def box_muller(w0, w1):
    """words -> (r, eps of the even actuator, eps of the odd one), fp64 past the float32 uniforms and the float32 angle"""
    u1, u2 = uniforms(w0, w1)
    theta = (TWO_PI_F32 * u2).astype(np.float32).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    return r, r * np.cos(theta), r * np.sin(theta)


def counters_of(env_id_offset, draw_counter, n_envs):
    """[n, 6, 4] uint32 Philox counters of a step: one block per (env, actuator pair)"""
    c = np.zeros((n_envs, A // 2, 4), np.uint32)
    env = np.array([(int(env_id_offset) + e) & 0xFFFFFFFF for e in range(n_envs)], np.uint32)
    draw = int(draw_counter) & 0xFFFFFFFFFFFFFFFF
    c[..., 0] = env[:, None]
    c[..., 1] = draw & 0xFFFFFFFF
    c[..., 2] = ((draw >> 32) ^ DRAW_DOMAIN) & 0xFFFFFFFF
    c[..., 3] = np.arange(A // 2, dtype=np.uint32)[None, :]
    return c


def draws(seed, env_id_offset, draw_counter, n_envs):
    """the standard-normal draws of one step -> (eps64 [n, 12], r [n, 12]); r is the Box-Muller radius of the element's pair"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), counters_of(env_id_offset, draw_counter, n_envs))
    r, even, odd = box_muller(w[..., 0], w[..., 1])
    eps = np.stack([even, odd], -1).reshape(n_envs, A)
    return eps, np.repeat(r, 2, axis=-1)


# ---------------------------------------------------------------- the network and its head
def _t(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def mlp(obs, mean, std, layers):
    """(obs - mean) / std through the SiLU MLP; layers = [(W [out, in], b [out])] x 4 -> head [n, 24] = (loc | raw)"""
    x = (_t(obs) - _t(mean)) / _t(std)
    return ppo_reference.silu_mlp(x, [(_t(w), _t(b)) for w, b in layers]).numpy()


def scale_of(raw):
    return (ppo_reference.softplus(_t(raw)) + 1e-3).numpy()


def head_logp(loc, raw, u):
    """tanh-normal log-probability of the pre-tanh sample u under (loc, raw) -> (logp [n], mag [n]): ppo_reference.log_prob, not restated"""
    logp, mag = ppo_reference.log_prob(torch.cat([_t(loc), _t(raw)], -1), _t(u))
    return logp.numpy(), mag.numpy()


# ---------------------------------------------------------------- the bookkeeping after the env step
def record(reward, done, ep_steps, up_z, ep_metrics, reward_scaling, episode_length, store_rows, counters, episode_sums):
    """one call of pgtt_rollout_record -> dict: row (the storage row it writes, or None: counters[0] outside [0, store_rows)), rew / done / trunc
    [N] (what that row receives), episode_sums [25] and counters [2] after the call.  -0.0 < 0 is false: an env at up_z = -0.0 has not fallen."""
    reward, done, up_z = (np.asarray(x, np.float64) for x in (reward, done, up_z))
    epm = np.asarray(ep_metrics, np.float64)
    t = int(counters[0])
    fallen = up_z < 0.0
    trunc = (np.asarray(ep_steps) >= int(episode_length)) & ~fallen
    ended = done != 0.0
    sums = np.array(episode_sums, np.float64)
    assert epm.shape[0] == NSUMS - 1 and sums.shape == (NSUMS,)
    sums[:NSUMS - 1] += (epm * done)[:, ended].sum(1)
    sums[NSUMS - 1] += done[ended].sum()
    return {"row": t if 0 <= t < int(store_rows) else None, "rew": reward * np.float64(np.float32(reward_scaling)), "done": done,
            "trunc": trunc.astype(np.float64), "episode_sums": sums, "counters": np.array([t + 1, int(counters[1]) + 1], np.int64)}
