"""The student perception function of include/pgtt_perceive.h restated in numpy fp64, from the header's text: explicit loops over the kernel window
and einsum over the channels.  It calls no torch and knows nothing of the packed layouts.

    cfg:  the config dict of perceive.config (height, width, near, far, conv = [(out_ch, kernel, stride)], prop_rows, hidden, obs_dim, scan_row0)
    net:  {"conv": [(w [O, C, k, k], b [O])], "fc1": (w [hidden, F + n_prop], b), "fc2": (w [117, hidden], b)} - anything np.asarray takes
"""
import numpy as np

NSCAN = 117


def preprocess(depth, near, far):
    """step 1: clamp to [near, far] (a NaN reads as far), scale to [-0.5, 0.5]"""
    d = np.array(depth, dtype=np.float64)
    d[np.isnan(d)] = far
    return (np.minimum(np.maximum(d, near), far) - near) / (far - near) - 0.5


def silu(v):
    return v / (1.0 + np.exp(-v))


def conv(x, w, b, stride):
    """x [N, C, H, W], w [O, C, k, k] -> silu(conv + b) [N, O, H', W']: no padding, no dilation"""
    w, b = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
    k = w.shape[2]
    ho, wo = (x.shape[2] - k) // stride + 1, (x.shape[3] - k) // stride + 1
    y = np.zeros((x.shape[0], w.shape[0], ho, wo))
    for di in range(k):
        for dj in range(k):
            win = x[:, :, di:di + stride * (ho - 1) + 1:stride, dj:dj + stride * (wo - 1) + 1:stride]
            y += np.einsum("nchw,oc->nohw", win, w[:, :, di, dj])
    return silu(y + b[None, :, None, None])


def latent(cfg, net, depth):
    """steps 1-3 -> [N, F], flattened in [C][H][W] order"""
    x = preprocess(depth, cfg["near"], cfg["far"])[:, None]
    for (w, b), (_, _, s) in zip(net["conv"], cfg["conv"]):
        x = conv(x, w, b, s)
    return x.reshape(x.shape[0], -1)


def forward(cfg, net, depth, obs):
    """-> (latent [N, F], est [N, 117], obs_out [N, obs_dim]) in fp64"""
    obs = np.asarray(obs, dtype=np.float64)
    lat = latent(cfg, net, depth)
    z = np.concatenate([lat, obs[:, list(cfg["prop_rows"])]], axis=1)
    w1, b1 = (np.asarray(a, dtype=np.float64) for a in net["fc1"])
    w2, b2 = (np.asarray(a, dtype=np.float64) for a in net["fc2"])
    est = silu(z @ w1.T + b1) @ w2.T + b2
    out = obs.copy()
    out[:, cfg["scan_row0"]:cfg["scan_row0"] + NSCAN] = est
    return lat, est, out
