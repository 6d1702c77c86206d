"""The student perception kernels (include/pgtt_perceive.h) at the sizes their contract allows: the envelope nets, the exact cases, the rounding
cases with a bar per element, the recurrent cases and the config sweep that tests/test_perceive_edge_cases.py (CPU: are the cases what they claim
to be?) and tests/test_gpu_perceive_edges.py (GPU: do the kernels compute them?) share.  numpy and CPU torch only: no library is loaded, no GPU
is needed.

The exact cases.  near = 0, far = 2 and depths in {0, 1, 2} (a NaN and a +inf read as far) make the preprocessed pixels {-0.5, 0, 0.5}; every weight
and every bias is an integer, so every value of the net is a half-integer.  One layer of a case is DENSE (integer weights in [-3, 3], or {-1, 0, 1}
where the bound asks for it; the bias the smallest power of two that keeps every pre-activation >= 20), every other layer is a PASS-THROUGH (row o
one-hot at position (7 o + 3) mod its input width, bias 32).  The builder works in int64 on twice the values and asserts, for every layer,
sum |w| |x| + |b| < 2^23: every product and every partial sum, in any order, is then a half-integer that fp32 holds exactly.  It also asserts
that every pre-activation of a SiLU layer is >= 20, where silu(v) = v / (1 + expf(-v)) returns v as bits in fp32: expf(-20) < 2^-24, the sum
rounds to 1, and the division is correctly rounded.  A dropped, doubled or misplaced term, a wrong pad or a wrong tile remainder changes bits.

The rounding cases.  He-initialised weights, uniform depth in [0, 3.5], the usual near and far, against fp64 with a bar per element carried
through the layers (bars()), from the constants tests/test_gpu_learn_kernels.py derives, u = 2^-24:
    e_z = (K + 2) u (|W| |x| + |b|) + |W| e_x     a K-term fp32 dot product in any order and the bias, and what the input's error becomes
    e_y = 1.1 e_z + 6 u |y|                       |silu'| <= 1.1; one expf at 2 ulp, one add, one divide
    e_x = 4 u                                     the preprocessed image: four roundings on values of at most 1
The bar of `latent` is e_y of the last conv, the bar of `est` is e_z of the second linear layer.  Nothing is fitted to a kernel."""
from functools import lru_cache

import numpy as np
import torch

import perceive_reference as ref

from phase_guided_terrain_traversal_amd import perceive

U = 2.0 ** -24
NSCAN = 117
LIMIT = 2 ** 23                                            # the bound of an exact case: sum |w| |x| + |b| stays below it
SILU_EXACT_FROM = 20                                       # silu(v) == v as fp32 bits for every half-integer v in [20, 2^23]
D = perceive.DEFAULTS


def _net(height, width, conv, **kw):
    return dict(D, height=height, width=width, conv=list(conv), **kw)


# 64 rows: every proprioceptive row of the default net and ten that point into the scan rows
PROP64 = list(range(38)) + list(range(155, 171)) + list(range(38, 48))
NETS = {
    "deep5": _net(13, 17, [(64, 5, 1), (64, 5, 1), (64, 5, 2)], prop_rows=PROP64),
    "budget1": _net(120, 128, [(16, 3, 2)]),
    "budget3": _net(12, 22, [(64, 5, 1), (64, 3, 1), (16, 3, 1)]),
    "min3": _net(3, 3, [(16, 3, 1)]),
    "wide": _net(5, 256, [(16, 5, 2)], hidden=144),
    "tall": _net(256, 5, [(16, 5, 2)], hidden=272),
    "two": _net(20, 28, [(48, 3, 2), (64, 3, 1)]),
    "allscan": _net(9, 11, [(16, 5, 2)], obs_dim=117, scan_row0=0, prop_rows=[0, 116, 3, 3]),
}
# name -> (shapes after each conv, lds_bytes, F): the issue's table, by hand
TABLE = {
    "deep5": ([(64, 9, 13), (64, 5, 9), (64, 1, 3)], 4 * (64 * 5 * 9 + 64 * 9 * 13), 192),
    "budget1": ([(16, 59, 63)], 61440, 59472),
    "budget3": ([(64, 8, 18), (64, 6, 16), (16, 4, 14)], 61440, 896),
    "min3": ([(16, 1, 1)], 36, 16),
    "wide": ([(16, 1, 126)], 5120, 2016),
    "tall": ([(16, 126, 1)], 5120, 2016),
    "two": ([(48, 9, 13), (64, 7, 11)], 4 * (20 * 28 + 48 * 9 * 13), 4928),
    "allscan": ([(16, 3, 4)], 396, 192),
}


def cut(cfg, l):
    """the net cut to its first l convs"""
    return dict(cfg, conv=cfg["conv"][:l])


# the variants: cut trunks, Kin one below and one past the 256-wide staging chunk, the hidden widths 16 and 128 (144, 272 and 512 are above)
VARIANTS = {
    "deep5:1": cut(NETS["deep5"], 1),
    "deep5:2": cut(NETS["deep5"], 2),
    "budget3:1": cut(NETS["budget3"], 1),
    "budget3:2": cut(NETS["budget3"], 2),
    "two:1": cut(NETS["two"], 1),
    "deep5-k255": dict(NETS["deep5"], prop_rows=PROP64[:-1]),
    # deep5's first two convs on a 10 x 10 image: 64 x 6 x 6, 64 x 2 x 2, F = 256 and one row more.  (deep5 cut to two convs has F = 2880 = 11 * 256 + 64:
    # no n_prop <= 64 puts its Kin one past a chunk, so the image shrinks instead of the row count growing.)
    "deep5-k257": _net(10, 10, [(64, 5, 1), (64, 5, 1)], prop_rows=[7]),
    "wide-h16": dict(NETS["wide"], hidden=16),
    "allscan-h128": dict(NETS["allscan"], hidden=128),
}
TABLE.update({
    "deep5:1": ([(64, 9, 13)], 4 * 221, 7488), "deep5:2": ([(64, 9, 13), (64, 5, 9)], 4 * (221 + 7488), 2880),
    "budget3:1": ([(64, 8, 18)], 4 * 264, 9216), "budget3:2": ([(64, 8, 18), (64, 6, 16)], 4 * (264 + 9216), 6144),
    "two:1": ([(48, 9, 13)], 4 * 560, 5616), "deep5-k255": TABLE["deep5"], "deep5-k257": ([(64, 6, 6), (64, 2, 2)], 4 * (100 + 2304), 256),
    "wide-h16": TABLE["wide"], "allscan-h128": TABLE["allscan"],
})
ALL = dict(NETS, **VARIANTS)
# envs per net: 1, 15, 16, 17 and 33 all occur; a net with a large F runs at most 3
ENVS = {"deep5": 17, "budget1": 3, "budget3": 3, "min3": 33, "wide": 15, "tall": 3, "two": 3, "allscan": 16, "deep5:1": 3, "deep5:2": 3,
        "budget3:1": 3, "budget3:2": 3, "two:1": 3, "deep5-k255": 16, "deep5-k257": 1, "wide-h16": 33, "allscan-h128": 17}


def latent_dim(cfg):
    c, h, w = perceive.conv_shapes(cfg)[-1]
    return c * h * w


def kin(cfg):
    return latent_dim(cfg) + len(cfg["prop_rows"])


def assert_envelope():
    """every net is one check_config accepts, with the shapes, the LDS bytes and the F of the table"""
    for name, cfg in ALL.items():
        perceive.check_config(cfg)
        shapes, lds, F = TABLE[name]
        assert perceive.conv_shapes(cfg)[1:] == shapes, (name, perceive.conv_shapes(cfg))
        assert perceive.lds_bytes(cfg) == lds and lds <= perceive.LDS_BYTES, (name, perceive.lds_bytes(cfg))
        assert latent_dim(cfg) == F, (name, latent_dim(cfg))
    assert kin(ALL["deep5"]) == 256 and kin(ALL["deep5-k255"]) == 255 and kin(ALL["deep5-k257"]) == 257
    assert -(-kin(ALL["budget1"]) // 256) == 233
    assert sorted({c["hidden"] for c in ALL.values()}) == [16, 128, 144, 272, 512] and {1, 15, 16, 17, 33} <= set(ENVS.values())
    assert all(ENVS[k] <= 3 for k in ALL if latent_dim(ALL[k]) > 2048) and set(ENVS) == set(ALL)


assert_envelope()


def layer_names(cfg):
    return [f"conv{l}" for l in range(len(cfg["conv"]))] + ["fc1", "fc2"]


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int32)


# ---------------------------------------------------------------- integer arithmetic (int64, on twice the values where they are half-integers)
def patches(x, k, s):
    """x [N, C, H, W] -> [N, P, C k k]: the conv's input as rows, k index = (c * k + di) * k + dj, pixels in [H_out][W_out] order"""
    v = np.lib.stride_tricks.sliding_window_view(x, (k, k), axis=(2, 3))[:, :, ::s, ::s]
    n, c, ho, wo = v.shape[:4]
    return np.ascontiguousarray(v.transpose(0, 2, 3, 1, 4, 5)).reshape(n, ho * wo, c * k * k), ho, wo


def imatmul(x, w):
    """x [..., K] int64, w [O, K] int8 -> x w^T in int64, K in blocks so that no int64 copy of a large w is made"""
    out = np.zeros(x.shape[:-1] + (w.shape[0],), np.int64)
    for k0 in range(0, w.shape[1], 4096):
        out += x[..., k0:k0 + 4096] @ w[:, k0:k0 + 4096].T.astype(np.int64)
    return out


def one_hot_positions(rows, width):
    return (7 * np.arange(rows) + 3) % width


class Layer:
    """one layer of an exact case: `pos` [O] (a pass-through: row o is one-hot at pos[o]) or `w` [O, K] int8 (dense), and an integer bias"""

    def __init__(self, rows, width, bias, w=None):
        self.rows, self.width, self.bias, self.w = rows, width, int(bias), w
        self.pos = None if w is not None else one_hot_positions(rows, width)

    def product(self, x):
        """x [..., K] int64 -> (W x, |W| |x|) without the bias"""
        if self.w is None:
            return x[..., self.pos], np.abs(x[..., self.pos])
        return imatmul(x, self.w), imatmul(np.abs(x), np.abs(self.w))

    def dense(self):
        """[O, K] fp32"""
        if self.w is not None:
            return self.w.astype(np.float32)
        m = np.zeros((self.rows, self.width), np.float32)
        m[np.arange(self.rows), self.pos] = 1.0
        return m


def exact_inputs(cfg, n, rng):
    """depth in {0, 1, 2} with a NaN and a +inf on a few pixels of every env, obs small integers (on the prop_rows too) -> (depth, obs) fp32 and
    twice the preprocessed image as int64"""
    h, w = cfg["height"], cfg["width"]
    d = rng.integers(0, 3, (n, h * w)).astype(np.float32)
    x2 = (d.astype(np.int64) - 1)                               # 2 * (d / 2 - 0.5)
    d[:, 1::11] = np.nan
    d[:, 4::13] = np.inf
    x2[:, 1::11] = 1
    x2[:, 4::13] = 1
    obs = rng.integers(-3, 4, (n, cfg["obs_dim"])).astype(np.float32)
    return d.reshape(n, h, w), obs, x2.reshape(n, 1, h, w)


def exact_case(name):
    """name = "<net>/<layer>": the net of ALL with that layer dense and every other layer a pass-through ->
    dict(name, net, cfg, n, dense, layers [Layer], depth, obs, latent, est, obs_out (the expectation, fp32), bound, min_pre)"""
    net_name, dense = name.split("/")
    cfg = dict(ALL[net_name], near=0.0, far=2.0)
    names = layer_names(cfg)
    n = ENVS[net_name]
    rng = np.random.default_rng(sum(name.encode()) + 1000 * names.index(dense))
    depth, obs, x = exact_inputs(cfg, n, rng)
    shapes = perceive.conv_shapes(cfg)
    widths = [shapes[l][0] * k * k for l, (_, k, _) in enumerate(cfg["conv"])] + [kin(cfg), cfg["hidden"]]
    rows = [co for co, _, _ in cfg["conv"]] + [cfg["hidden"], NSCAN]
    layers, bound, min_pre, small = [], 0, None, False
    for l, lname in enumerate(names):
        if lname == "fc1":                                      # z = latent followed by obs[prop_rows], twice of each
            lat2 = x.reshape(n, -1)
            x = np.concatenate([lat2, 2 * obs[:, cfg["prop_rows"]].astype(np.int64)], axis=1)
        if l < len(cfg["conv"]):
            _, k, s = cfg["conv"][l]
            rows_in, ho, wo = patches(x, k, s)
        else:
            rows_in = x
        assert rows_in.shape[-1] == widths[l]
        for mag in (3, 1):
            if lname == dense:
                layer = Layer(rows[l], widths[l], 0, rng.integers(-mag, mag + 1, (rows[l], widths[l])).astype(np.int8))
            else:
                layer = Layer(rows[l], widths[l], 32)
            z2, a2 = layer.product(rows_in)
            if lname == dense:                                  # the smallest power of two that keeps every pre-activation >= 20
                b = 1
                while 2 * b + int(z2.min()) < 2 * SILU_EXACT_FROM:
                    b *= 2
                layer.bias = b
            this = (int(a2.max()) + 2 * abs(layer.bias) + 1) // 2        # sum |w| |x| + |b|, rounded up
            if this < LIMIT or lname != dense or mag == 1:
                small = small or (lname == dense and mag == 1)
                break
        z2 = z2 + 2 * layer.bias
        bound = max(bound, this)
        if lname != "fc2":                                      # a SiLU layer
            m = int(z2.min())
            min_pre = m / 2 if min_pre is None else min(min_pre, m / 2)
        layers.append(layer)
        x = z2.reshape(n, ho, wo, rows[l]).transpose(0, 3, 1, 2) if l < len(cfg["conv"]) else z2
    assert bound < LIMIT and min_pre >= SILU_EXACT_FROM, (name, bound, min_pre)      # the conditions the exactness rests on
    est = (x / 2).astype(np.float32)
    out = obs.copy()
    out[:, cfg["scan_row0"]:cfg["scan_row0"] + NSCAN] = est
    return dict(name=name, net=net_name, cfg=cfg, n=n, dense=dense, layers=layers, depth=depth, obs=obs, latent=(lat2 / 2).astype(np.float32), est=est,
                obs_out=out, bound=bound, min_pre=min_pre, small_weights=small)


def exact_names():
    """one case per layer of every envelope net and variant.  A conv that is not the last layer of its net is also the last layer of the net cut
    there ("deep5:2/conv1"): every one of its outputs is then observed in `latent`."""
    return [f"{net}/{layer}" for net, cfg in ALL.items() for layer in layer_names(cfg)]


def estimator_of(case):
    """the ScanEstimator that holds an exact case's weights"""
    est = perceive.ScanEstimator(case["cfg"])
    with torch.no_grad():
        for m, layer in zip(est.layers(), case["layers"]):
            m.weight.copy_(torch.from_numpy(layer.dense()).view(m.weight.shape))
            m.bias.fill_(float(layer.bias))
    return est


def where_wrong(case, key, got):
    """'' or a message that names the first wrong element of `got` against the expectation: for the latent, its channel and pixel"""
    want = case[key]
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(-1))
    if not len(bad):
        return ""
    e, j = divmod(int(bad[0]), want.shape[1])
    msg = f"{case['name']} {key}: {len(bad)} of {want.size} wrong, first env {e} element {j}: got {got[e, j]!r}, want {want[e, j]!r}"
    if key == "latent":
        c, h, w = perceive.conv_shapes(case["cfg"])[-1]
        ch, p = divmod(j, h * w)
        msg += f" (channel {ch} = tile {ch // 16} row {ch % 16}, pixel {p} = ({p // w}, {p % w}) = tile {p // 16} column {p % 16})"
    elif key == "est":
        msg += f" (tile {j // 16} row {j % 16}, env column {e % 16} of group {e // 16})"
    return msg


# ---------------------------------------------------------------- rounding cases
def he_init(est, seed):
    """He-normal weights, biases 0.1 N(0, 1): tests/test_gpu_perceive.py's, and the same for a GRU's two matrices"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        pairs = [(m.weight, m.bias) for m in est.layers()]
        if est.memory:
            pairs += [(est.gru.weight_ih, est.gru.bias_ih), (est.gru.weight_hh, est.gru.bias_hh)]
        for w, b in pairs:
            w.copy_(torch.randn(w.shape, generator=g) * (2.0 / w[0].numel()) ** 0.5)
            b.copy_(torch.randn(b.shape, generator=g) * 0.1)
    return est


def net_of(est):
    """the reference's view of an estimator (tests/perceive_reference.py, tests/perceive_memory_reference.py)"""
    f64 = lambda t: t.detach().double().cpu().numpy()
    net = {"conv": [(f64(c.weight), f64(c.bias)) for c in est.convs], "fc1": (f64(est.fc1.weight), f64(est.fc1.bias))}
    if est.memory:
        net.update(w_ih=f64(est.gru.weight_ih), b_ih=f64(est.gru.bias_ih), w_hh=f64(est.gru.weight_hh), b_hh=f64(est.gru.bias_hh),
                   out=(f64(est.fc2.weight), f64(est.fc2.bias)))
    else:
        net["fc2"] = (f64(est.fc2.weight), f64(est.fc2.bias))
    return net


def random_inputs(cfg, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 3.5, (n, cfg["height"], cfg["width"])).astype(np.float32), rng.normal(size=(n, cfg["obs_dim"])).astype(np.float32))


ROUNDING = list(ALL)


def rounding_case(name):
    """-> (cfg, estimator, depth, obs): the usual near and far"""
    cfg, n = ALL[name], ENVS[name]
    est = he_init(perceive.ScanEstimator(cfg), 31)
    depth, obs = random_inputs(cfg, n, 37)
    return cfg, est, depth, obs


def _linear_conv(x, w, stride):
    """sum_{c, di, dj} w x without bias or activation (perceive_reference.conv's loop)"""
    k = w.shape[2]
    ho, wo = (x.shape[2] - k) // stride + 1, (x.shape[3] - k) // stride + 1
    y = np.zeros((x.shape[0], w.shape[0], ho, wo))
    for di in range(k):
        for dj in range(k):
            win = x[:, :, di:di + stride * (ho - 1) + 1:stride, dj:dj + stride * (wo - 1) + 1:stride]
            y += np.einsum("nchw,oc->nohw", win, w[:, :, di, dj])
    return y


def bars(cfg, net, depth, obs):
    """the fp64 forward with the module docstring's bar per element -> (latent, e_latent, est, e_est)"""
    x = ref.preprocess(depth, cfg["near"], cfg["far"])[:, None]
    ex = np.full_like(x, 4 * U)
    for (w, b), (_, _, s) in zip(net["conv"], cfg["conv"]):
        K = w[0].size
        bb = b[None, :, None, None]
        z = _linear_conv(x, w, s) + bb
        ez = (K + 2) * U * (_linear_conv(np.abs(x), np.abs(w), s) + np.abs(bb)) + _linear_conv(ex, np.abs(w), s)
        x = ref.silu(z)
        ex = 1.1 * ez + 6 * U * np.abs(x)
    lat, elat = x.reshape(len(x), -1), ex.reshape(len(x), -1)
    prop = np.asarray(obs, np.float64)[:, list(cfg["prop_rows"])]
    z, ez = np.concatenate([lat, prop], axis=1), np.concatenate([elat, np.zeros_like(prop)], axis=1)      # the observation is exact
    (w1, b1), (w2, b2) = net["fc1"], net["fc2"]
    eh = (w1.shape[1] + 2) * U * (np.abs(z) @ np.abs(w1).T + np.abs(b1)) + ez @ np.abs(w1).T
    h = ref.silu(z @ w1.T + b1)
    eh = 1.1 * eh + 6 * U * np.abs(h)
    est = h @ w2.T + b2
    eest = (w2.shape[1] + 2) * U * (np.abs(h) @ np.abs(w2).T + np.abs(b2)) + eh @ np.abs(w2).T
    return lat, elat, est, eest


def ratios(cfg, net, depth, obs, got_latent, got_est):
    """worst error / bar of (latent, est) for the per-element bar, and of (latent, est) for the project's forward bar, one number per tensor:
    2e-5 * (1 + max |want|) (tests/test_gpu_perceive.py)"""
    lat, elat, est, eest = bars(cfg, net, depth, obs)
    flat = lambda got, want: float(np.abs(got - want).max() / (2e-5 * (1 + np.abs(want).max())))
    return float((np.abs(got_latent - lat) / elat).max()), float((np.abs(got_est - est) / eest).max()), flat(got_latent, lat), flat(got_est, est)


# ---------------------------------------------------------------- the recurrent twins
RECURRENT_ROUNDING = [(net, r) for net in ("deep5", "budget3", "wide", "tall", "two", "allscan") for r in (16, 256)]
RECURRENT_EXACT = [(net, 256 if i % 2 else 16) for i, net in enumerate(NETS)]


def recurrent_exact_case(net_name, memory):
    """u = 1 exactly: the update gate's rows of b_ih are 64 and of w_ih, w_hh and b_hh zero, so m1 = (1 - 1) n + 1 m0 = m0 as bits whatever the
    trunk, the hidden layer and the other gates compute; W_out, b_out and m0 are small integers, so est = W_out m0 + b_out is exact.  Every third
    env is cleared: its memory reads as zero, so est = b_out and mem = 0.
    -> dict(cfg, n, est (the estimator), depth, obs, mem0, clear [N] uint8, want_mem, want_est, want_obs)"""
    cfg, n, R = dict(NETS[net_name], memory=memory), ENVS[net_name], memory
    est = he_init(perceive.ScanEstimator(cfg), 41)
    rng = np.random.default_rng(43 + memory)
    with torch.no_grad():
        est.gru.weight_ih[R:2 * R].zero_(); est.gru.weight_hh[R:2 * R].zero_(); est.gru.bias_hh[R:2 * R].zero_()
        est.gru.bias_ih[R:2 * R] = 64.0
        est.fc2.weight.copy_(torch.from_numpy(rng.integers(-3, 4, (NSCAN, R)).astype(np.float32)))
        est.fc2.bias.copy_(torch.from_numpy(rng.integers(-3, 4, NSCAN).astype(np.float32)))
    depth, obs = random_inputs(cfg, n, 47)
    mem0 = rng.integers(-3, 4, (n, R)).astype(np.float32)
    clear = (np.arange(n) % 3 == 2).astype(np.uint8)
    m = np.where(clear[:, None] != 0, 0, mem0.astype(np.int64))
    want_est = (m @ est.fc2.weight.detach().numpy().astype(np.int64).T + est.fc2.bias.detach().numpy().astype(np.int64)).astype(np.float32)
    out = obs.copy()
    out[:, cfg["scan_row0"]:cfg["scan_row0"] + NSCAN] = want_est
    return dict(cfg=cfg, n=n, est=est, depth=depth, obs=obs, mem0=mem0, clear=clear, want_mem=m.astype(np.float32), want_est=want_est, want_obs=out)


# ---------------------------------------------------------------- the host checks' sweep
def sweep_configs(count=2000, seed=5):
    """random configs around the edges of the ranges of pgtt_perceive.h, from a fixed seed.  Four draws in five of every field come from its legal
    values alone, so that a fair share of the configs is accepted."""
    rng = np.random.default_rng(seed)
    pick = lambda legal, near: int(rng.choice(legal if rng.random() < 0.8 else legal + near))
    out = []
    for _ in range(count):
        h, w = (int(v) for v in (rng.integers(1, 257, 2) if rng.random() < 0.5 else rng.integers(3, 60, 2)))
        conv = [(pick([16, 32, 48, 64], [0, 8, 24, 80]), pick([3, 5], [1, 4, 7]), pick([1, 2], [0, 3])) for _ in range(pick([1, 2, 3], [0, 4]))]
        n_prop = pick([0, 64], [])
        od = pick([117, 171], [100, 116])
        row0 = pick([0], [38, 54, 55])
        rows = [int(r) for r in rng.integers(0, od + (rng.random() < 0.1), n_prop)]
        out.append(dict(height=h, width=w, near=0.1, far=3.0, conv=conv, prop_rows=rows, hidden=pick([16, 512], [0, 8, 500, 528]), obs_dim=od,
                        scan_row0=row0))
    return out


def accepted(cfg):
    try:
        perceive.check_config(cfg)
        return True
    except ValueError:
        return False


@lru_cache(maxsize=None)
def sweep():
    """-> [(cfg, accepted by perceive.check_config)]: built once, read only"""
    return [(c, accepted(c)) for c in sweep_configs()]
