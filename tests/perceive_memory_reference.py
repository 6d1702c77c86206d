"""The recurrent form of include/pgtt_perceive.h restated in numpy fp64, from the header's text: steps 1 - 4 and the hidden layer are
perceive_reference's, the GRU cell and the output layer are written out gate by gate.  It calls no torch and knows nothing of the packed layouts.

    cfg:  the config dict of perceive.config with memory = R
    net:  perceive_reference's "conv" and "fc1", and "w_ih" [3R, hidden], "b_ih" [3R], "w_hh" [3R, R], "b_hh" [3R] (gate order r, u, n),
          "out": (w [117, R], b [117])
"""
import numpy as np

import perceive_reference as ref

NSCAN = ref.NSCAN


def sigmoid(v):
    t = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def hidden(cfg, net, depth, obs):
    """-> (latent [N, F], h [N, hidden]): steps 1 - 4 and h = silu(W1 z + b1)"""
    obs = np.asarray(obs, dtype=np.float64)
    lat = ref.latent(cfg, net, depth)
    z = np.concatenate([lat, obs[:, list(cfg["prop_rows"])]], axis=1)
    w1, b1 = (np.asarray(a, dtype=np.float64) for a in net["fc1"])
    return lat, ref.silu(z @ w1.T + b1)


def cell(net, h, m0):
    """the GRU cell: h [N, hidden], m0 [N, R] -> m1 [N, R]"""
    w_ih, b_ih, w_hh, b_hh = (np.asarray(net[k], dtype=np.float64) for k in ("w_ih", "b_ih", "w_hh", "b_hh"))
    R = w_hh.shape[1]
    gi, gh = h @ w_ih.T + b_ih, m0 @ w_hh.T + b_hh
    r = sigmoid(gi[:, :R] + gh[:, :R])
    u = sigmoid(gi[:, R:2 * R] + gh[:, R:2 * R])
    n = np.tanh(gi[:, 2 * R:] + r * gh[:, 2 * R:])
    return (1.0 - u) * n + u * m0


def step(cfg, net, depth, obs, mem, clear=None):
    """one tick -> (latent [N, F], mem1 [N, R], est [N, 117], obs_out [N, obs_dim]); clear [N]: non-zero reads the env's memory as zero"""
    obs = np.asarray(obs, dtype=np.float64)
    m0 = np.array(mem, dtype=np.float64)
    if clear is not None:
        m0[np.asarray(clear) != 0] = 0.0
    lat, h = hidden(cfg, net, depth, obs)
    m1 = cell(net, h, m0)
    w, b = (np.asarray(a, dtype=np.float64) for a in net["out"])
    est = m1 @ w.T + b
    out = obs.copy()
    out[:, cfg["scan_row0"]:cfg["scan_row0"] + NSCAN] = est
    return lat, m1, est, out


def sequence(cfg, net, depth, obs, mem0, clear=None):
    """T ticks: depth [T, N, H, W], obs [T, N, obs_dim], clear [T, N] or None -> (mem [T, N, R], est [T, N, 117]) after every tick"""
    mem, ms, es = np.asarray(mem0, dtype=np.float64), [], []
    for t in range(len(depth)):
        _, mem, est, _ = step(cfg, net, depth[t], obs[t], mem, None if clear is None else clear[t])
        ms.append(mem); es.append(est)
    return np.stack(ms), np.stack(es)
