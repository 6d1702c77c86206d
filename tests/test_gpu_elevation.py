"""libpgtt_elevation.so on the GPU: the kernel against the fp64 statement of tests/elevation_reference.py, batch independence, determinism, the
three ways of clearing, degenerate images, the env integration and graph capture.

The bar is the project's forward bar: |device - reference| <= 2e-5 (1 + |reference|), on the map cells and on the scan rows.  A
cell's value is a maximum over the pixels that fall into it, so a pixel on a cell border can change a cell by far more than a rounding error;
the reference says how far every pixel is from the nearest border (and from changing sides of the self-filter box), and a cell that a pixel
within 2e-5 m of a border could have entered or left is left out (elevation_reference.doubtful_cells), from that tick on.  Scan points within
2e-5 m of a border, or in such a cell, are left out likewise.  At most 5 % of the touched cells and 5 % of the scan points may be left out.

`est` is `z - min z`.  It is held to the bar as it stands whenever the minimum is a compared point for the reference and for the device, which is so in
all but 2 of the 111 env-ticks with a known compared point; in those two a left-out point is the minimum on one side, every `est` moves by the
difference, and `est` is held to the bar up to that common offset (it is held up to a common offset always).

Measured shares (pooled over the envs and ticks of a case, 13 cases): test_parity's docstring."""
import os
import sys
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_reference as ref  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, configs, depth as depth_mod, elevation  # noqa: E402
from phase_guided_terrain_traversal_amd.acting import FusedActor  # noqa: E402
from phase_guided_terrain_traversal_amd.env import Joystick  # noqa: E402
from phase_guided_terrain_traversal_amd.policy import load_policy  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL4 = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy")
EPS = 2e-5
RES = 0.04
NTICK = 3
VARIANTS = [0, 2, 7]                             # of level4; variant 3 puts a wall on the line y = 0, a cell border: a column of pixels in doubt
FAR_CELLS = 97                                   # a move of more than G cells for every G <= 96


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return a.view(np.int32) if a.dtype == np.float32 else a


def make_env(n, seed, variant=None, **kw):
    terrain = np.load(LEVEL4)
    if variant is None:
        variant = np.random.default_rng(0).integers(0, terrain.shape[0], n)
    env = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0",
                   variant=torch.from_numpy(np.asarray(variant, np.int32)), **kw)
    env.reset(seed)
    return env


@lru_cache(maxsize=None)
def recorded(width, height):
    """NTICK consecutive (state [NSTATE, 3], image [3, H, W], obs [3, 171]) of three envs on three variants of level4, as numpy: the poses after six
    small random actions (roll and pitch are non-zero), env 2 placed at negative x and y, and between the ticks each base moved by hand - by less
    than a cell (inside its cell: the origin stays, the pose and the image change), by five cells, by more than G cells - with the image taken again
    from the moved pose.  A base sits at fraction (0.37, 0.61) of its cell, after a small move at (0.57, 0.41): the origin is never in doubt.
    Computed once per image size and shared."""
    env = make_env(3, 11, variant=VARIANTS, depth=dict(width=width, height=height))
    rng = np.random.default_rng(5)
    for _ in range(6):
        env.step(torch.from_numpy(np.tanh(rng.normal(size=(3, 12)) * 0.4).astype(np.float32)).cuda())
    S = env.buffers["state"]
    xy = S[0:2].cpu().numpy().astype(float)                                      # [2, 3]
    xy[:, 2] = (-1.3, -0.7)
    cells = np.floor(xy / RES)                                                   # [2, 3]: each base's cell; the moves are whole cells ...
    frac = np.tile(np.array([[0.37], [0.61]]), (1, 3))                           # ... or, for the small one, another place inside the cell
    small, several, far = None, np.array([5, -3]), np.array([FAR_CELLS, 0])
    moves = [None, (small, several, far), (-several, -far, small)]
    out = []
    for t in range(NTICK):
        for e, mv in enumerate(moves[t] or ()):
            if mv is None:
                frac[:, e] = (0.57, 0.41)                                        # 0.2 of a cell along each axis: 11 mm in all
            else:
                cells[:, e] += mv
        S[0:2] = torch.from_numpy(((cells + frac) * RES).astype(np.float32)).cuda()
        env.depth_camera.tick(force=True)
        torch.cuda.synchronize()
        out.append((S.cpu().numpy().copy(), env.depth.cpu().numpy().copy(), env.buffers["obs_state"].cpu().numpy().copy()))
    cam = env.depth_camera.config
    camera = dict(width=width, height=height, fovy=cam.fovy_deg, near=cam.near, far=cam.far, mount_pos=tuple(cam.mount_pos), mount_quat=tuple(cam.mount_quat))
    env.close()
    return camera, out


class Rig:
    """what ElevationMap reads of an env - state, image, observation, done, the camera's config - as tensors the test fills, and the map on them"""

    def __init__(self, n, camera, obs_dim=171, method="pgtt", **settings):
        dev = torch.device("cuda:0")
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)
        self.camera = camera
        cc = depth_mod.config_struct(camera["width"], camera["height"], camera["fovy"], camera["near"], camera["far"], 0, camera["mount_pos"],
                                     camera["mount_quat"])
        self.env = types.SimpleNamespace(depth=z(n, camera["height"], camera["width"]), depth_camera=types.SimpleNamespace(config=cc),
                                         buffers={"state": z(abi.NSTATE, n), "obs_state": z(n, obs_dim), "done": z(n)}, device=dev, num_envs=n,
                                         observation_size={"state": obs_dim}, config=dict(scan_dist_x=0.1, scan_dist_y=0.1), method=method)
        self.map = elevation.ElevationMap(self.env, **settings)

    def put(self, state, image, obs=None):
        self.env.buffers["state"].copy_(torch.from_numpy(np.ascontiguousarray(state)))
        self.env.depth.copy_(torch.from_numpy(np.ascontiguousarray(image)))
        if obs is not None:
            self.env.buffers["obs_state"].copy_(torch.from_numpy(np.ascontiguousarray(obs)))

    def tick(self, **kw):
        self.map.tick(**kw)
        torch.cuda.synchronize()
        m = self.map
        return {k: getattr(m, k).cpu().numpy().copy() for k in ("map", "origin", "est", "known", "obs")}

    def close(self):
        self.map.close()


def ref_cfg(camera, settings):
    return dict(fovy=camera["fovy"], near=camera["near"], far=camera["far"], mount_pos=camera["mount_pos"], mount_quat=camera["mount_quat"], res=settings["res"],
                alpha=settings["alpha"], self_half=settings["self_half"])


class Tally:
    def __init__(self):
        self.touched = self.touched_out = self.scan = self.scan_out = 0
        self.worst_map = self.worst_est = 0.0
        self.est_ticks = self.est_strict = 0                     # env-ticks with known compared scan points; those of them held to the bar as they stand

    def shares(self):
        return self.touched_out / max(self.touched, 1), self.scan_out / max(self.scan, 1)


def compare(got, e, want, doubtful, tally, G):
    """one env of one tick against the reference's `want`; `doubtful`: the world cells in doubt so far (this tick's included)"""
    assert np.array_equal(got["origin"][e], want["origin"]), (got["origin"][e], want["origin"])
    wc = ref.world_cells(want["origin"], G)
    out = np.array([[tuple(wc[i, j]) in doubtful for j in range(G)] for i in range(G)])
    dev, w = got["map"][e].astype(float), want["map"]
    assert np.array_equal(np.isnan(dev)[~out], np.isnan(w)[~out]), "NaN pattern"
    cmp = ~out & ~np.isnan(w)
    if cmp.any():
        ratio = np.abs(dev[cmp] - w[cmp]) / (EPS * (1 + np.abs(w[cmp])))
        tally.worst_map = max(tally.worst_map, float(ratio.max()))
        assert ratio.max() <= 1, ("map", float(ratio.max()))
    tally.touched += int(want["touched"].sum()); tally.touched_out += int((want["touched"] & out).sum())
    # the scan: a point near a border or in a doubtful cell is left out
    sc = want["scan"]
    left = (sc["margin"] < EPS) | np.array([tuple(c) in doubtful for c in sc["cell"]])
    tally.scan += ref.NSCAN; tally.scan_out += int(left.sum())
    k = ~left
    assert np.array_equal(got["known"][e][k] != 0, want["known"][k]), "known"
    assert np.isfinite(got["est"][e]).all()
    kk = k & want["known"]
    assert (got["est"][e][k & ~want["known"]] == 0).all()
    if kk.any():
        # est = z - min z.  Up to a common offset always.  As it stands whenever the minimum is a compared point on BOTH sides (the reference's est
        # and the device's est are 0 at a compared point): the two minima are then values of compared cells, which agree.  Otherwise a left-out
        # point - a cell in doubt, which may hold another pixel's height or nothing on one side - is the minimum on one side, and every est
        # moves by the difference.
        i0 = np.flatnonzero(kk)[0]
        bar = EPS * (1 + np.abs(want["est"][kk]))
        rel = np.abs((got["est"][e][kk].astype(float) - got["est"][e][i0]) - (want["est"][kk] - want["est"][i0])) / bar
        assert rel.max() <= 1, ("est, offset-free", float(rel.max()))
        tally.est_ticks += 1
        if (want["est"][kk] == 0).any() and (got["est"][e][kk] == 0).any():
            tally.est_strict += 1
            ratio = np.abs(got["est"][e][kk] - want["est"][kk]) / bar
            tally.worst_est = max(tally.worst_est, float(ratio.max()))
            assert ratio.max() <= 1, ("est", float(ratio.max()))
    # obs_out
    o, src, r0 = _bits(got["obs"][e]), _bits(want["obs_in"]), 38
    assert np.array_equal(o[:r0], src[:r0]) and np.array_equal(o[r0 + 117:], src[r0 + 117:]) and np.array_equal(o[r0:r0 + 117], _bits(got["est"][e]))


def run_sequence(rig, ticks, cfg, G, tally, clear_first=True):
    states = [ref.new_state(G) for _ in range(3)]
    doubtful = [set() for _ in range(3)]
    for t, (S, img, obs) in enumerate(ticks):
        rig.put(S, img, obs)
        got = rig.tick(clear_all=clear_first and t == 0)
        for e in range(3):
            want = ref.tick(states[e], S[:7, e], img[e], cfg, clear=clear_first and t == 0)
            want["obs_in"] = obs[e]
            # a cell stays in doubt while it can still hold something of the doubtful tick: until it leaves the window, or, with alpha = 1, until a
            # tick replaces it (a tick that touches it with a doubtful pixel puts it in doubt again)
            wc = ref.world_cells(want["origin"], G)
            if cfg["alpha"] == 1.0:
                doubtful[e] -= {tuple(c) for c in wc[want["touched"]]}
            doubtful[e] &= {tuple(c) for c in wc.reshape(-1, 2)}
            doubtful[e] |= ref.doubtful_cells(want, cfg["res"], EPS)
            compare(got, e, want, doubtful[e], tally, G)
            states[e] = (want["map"], want["origin"])


# ---------------------------------------------------------------- 1. parity
# G = 8 and G = 24 are windows of 0.32 m and 0.96 m around the base, which a camera that looks ahead from the head hardly sees: those cases tell the map
# that the camera sits further back (the unprojection does not care how the image was made): by 0.8 m and 0.5 m for the 16 x 12 image, so that its
# near field lands in the window, and by 1.6 m and 2.0 m for the 64 x 48 image, so that its far field does - there a cell gets about one pixel, while
# the near field of 3072 pixels in 64 cells would put 4 x 2e-5 / 0.04 x 48 = 10 % of the cells in doubt by the count of pixels alone.  G < 24 runs without the self filter (the other path of the kernel), G = 24 with a small box, G = 64 with the default one;
# G = 9 is the odd size, where a map is not a whole number of 16-byte runs
CASES = [(w, h, g, a) for (w, h) in ((16, 12), (64, 48)) for g in (8, 24, 64) for a in (1.0, 0.5)] + [(16, 12, 9, 0.5)]


def case_setup(camera, G, alpha):
    settings = dict(grid=G, res=RES, alpha=alpha, self_half=(0.45, 0.25, 0.45))
    if G <= 24:
        back = (0.8 if G < 24 else 0.5) if camera["width"] < 64 else (1.6 if G < 24 else 2.0)
        camera = dict(camera, mount_pos=(camera["mount_pos"][0] - back, 0.0, camera["mount_pos"][2]))
        settings["self_half"] = (0.0, 0.0, 0.0) if G < 24 else (0.12, 0.1, 0.45)
    return camera, settings


@pytest.mark.parametrize("width,height,G,alpha", CASES)
def test_parity(width, height, G, alpha):
    """Left out on an MI355X, per case (three envs, three ticks pooled), the same for alpha = 1 unless two figures are given (alpha = 1 / alpha = 0.5):

        image   G    touched cells   left out, cells            left out, scan points (of 1053)
        16x12   8        193         1        0.52 %            6    0.57 %
        16x12   9        239         1        0.42 %            6    0.57 %   (alpha = 0.5 only)
        16x12  24        756         0        0.00 %            3    0.28 %
        16x12  64       1161         4 / 5    0.34 / 0.43 %     4    0.38 %
        64x48   8        211         0        0.00 %            8    0.76 %
        64x48  24       1115        11 / 15   0.99 / 1.35 %     5 / 6    0.47 / 0.57 %
        64x48  64       4093        76 / 102  1.86 / 2.49 %    11 / 12   1.04 / 1.14 %

    against the cap of 5 % each.  The worst error on the compared cells is 0.010 of the bar, on `est` 0.006 of it; `est` was held as it stands in
    7 of 7 or 9 of 9 env-ticks of every case but 64x48 G = 24 (8 of 9).  The reference alone, on the CPU, with the poses of the CPU oracle (which the
    env follows to 1e-5) and the images of depth_reference, before the poses were fixed: 0.00 - 2.97 % of the cells, 0.38 - 1.14 % of the scan points."""
    camera, ticks = recorded(width, height)
    camera, settings = case_setup(camera, G, alpha)
    rig = Rig(3, camera, **settings)
    tally = Tally()
    run_sequence(rig, ticks, ref_cfg(camera, settings), G, tally)
    rig.close()
    cells, scan = tally.shares()
    print(f"{width}x{height} G={G} alpha={alpha}: touched {tally.touched}, left out {tally.touched_out} ({100 * cells:.2f} %), scan left out {tally.scan_out} of {tally.scan} "
          f"({100 * scan:.2f} %), worst error / bar: map {tally.worst_map:.3f}, est {tally.worst_est:.3f}; est held as it stands in {tally.est_strict} of "
          f"{tally.est_ticks} env-ticks")
    assert tally.touched >= 20, "the case would be vacuous"
    assert tally.est_strict >= 1 and 2 * tally.est_strict >= tally.est_ticks, "the subtraction of the minimum was hardly checked"
    assert cells <= 0.05 and scan <= 0.05


# ---------------------------------------------------------------- 2. batch independence, determinism
def _two_ticks(n, camera, ticks, cols, **settings):
    """two ticks of a batch whose env i has the rows of recorded env cols[i] -> the outputs of the second tick"""
    rig = Rig(n, camera, **settings)
    for t in range(2):
        S, img, obs = ticks[t]
        rig.put(S[:, cols], img[cols], obs[cols])
        got = rig.tick(clear_all=t == 0)
    rig.close()
    return got


def test_batch_independence_and_determinism():
    camera, ticks = recorded(64, 48)
    settings = dict(grid=24, res=RES, alpha=0.5, self_half=(0.45, 0.25, 0.45))
    three = _two_ticks(3, camera, ticks, [0, 1, 2], **settings)
    again = _two_ticks(3, camera, ticks, [0, 1, 2], **settings)
    big = _two_ticks(65, camera, ticks, [0] + [1] * 63 + [2], **settings)
    for k in three:
        assert np.array_equal(_bits(three[k]), _bits(again[k])), k                     # determinism
    assert (~np.isnan(three["map"])).sum() > 50
    for e, pos in ((0, 0), (2, 64)):
        alone = _two_ticks(1, camera, ticks, [e], **settings)
        for k in three:
            assert np.array_equal(_bits(three[k][e]), _bits(alone[k][0])), (k, e)
            assert np.array_equal(_bits(three[k][e]), _bits(big[k][pos])), (k, e)


# ---------------------------------------------------------------- 3. clears
@pytest.mark.parametrize("name,kw,done,cleared", [("clear_all", dict(clear_all=True), (0, 0, 0), (1, 1, 1)),
                                                  ("mask", dict(clear_mask=(0, 1, 0)), (0, 0, 0), (0, 1, 0)),
                                                  ("use_done", dict(use_done=True), (0, 1, 0), (0, 1, 0)),
                                                  ("done_not_used", dict(use_done=False), (1, 1, 1), (0, 0, 0))])
def test_clears(name, kw, done, cleared):
    camera, ticks = recorded(16, 12)
    G = 24
    rig = Rig(3, camera, grid=G, res=RES, alpha=1.0, self_half=(0.45, 0.25, 0.45))
    S, img, obs = ticks[0]
    rig.put(S, img, obs)
    first = rig.tick(clear_all=True)                                              # the origin is the pose's from here on: nothing is stale
    rig.map.map.fill_(5.0)
    rig.env.buffers["done"].copy_(torch.tensor(done, dtype=torch.float32))
    if "clear_mask" in kw:
        kw = dict(kw, clear_mask=torch.tensor(kw["clear_mask"], dtype=torch.uint8))
    got = rig.tick(**kw)
    touched = ~np.isnan(first["map"])
    assert touched.sum() > 20
    for e in range(3):
        if cleared[e]:                                                            # cleared BEFORE integrating: this tick's cells and nothing else
            assert np.array_equal(_bits(got["map"][e]), _bits(first["map"][e])), (name, e)
        else:
            assert (got["map"][e][~touched[e]] == 5.0).all() and np.array_equal(_bits(got["map"][e][touched[e]]), _bits(first["map"][e][touched[e]])), (name, e)
    rig.close()


# ---------------------------------------------------------------- 4. degenerate images
def test_degenerate_images():
    camera, ticks = recorded(64, 48)
    G = 64
    settings = dict(grid=G, res=RES, alpha=1.0, self_half=(0.45, 0.25, 0.45))
    S, img, obs = ticks[0]
    img = img.copy()
    good = img[2].copy()
    img[0] = camera["far"]
    img[1] = 0.01                                                                # below near
    img[2].reshape(-1)[::5] = np.nan
    img[2].reshape(-1)[1::7] = np.inf
    img[2].reshape(-1)[2::11] = -np.inf
    rig = Rig(3, camera, **settings)
    rig.put(S, img, obs)
    got = rig.tick(clear_all=True)
    assert np.isnan(got["map"][0]).all() and np.isnan(got["map"][1]).all()
    assert (got["est"][:2] == 0).all() and (got["known"][:2] == 0).all() and np.isfinite(got["est"]).all()
    cfg = ref_cfg(camera, settings)
    tally = Tally()
    want = ref.tick(ref.new_state(G), S[:7, 2], img[2], cfg, clear=True)
    want["obs_in"] = obs[2]
    compare(got, 2, want, ref.doubtful_cells(want, RES, EPS), tally, G)
    # the bad pixels gave the map nothing: every finite cell is one the good pixels alone reach
    clean = ref.tick(ref.new_state(G), S[:7, 2], np.where(np.isfinite(img[2]), good, camera["far"]), cfg, clear=True)
    assert want["touched"].sum() > 20 and np.array_equal(want["touched"], clean["touched"])
    assert not np.isinf(got["map"]).any()
    rig.close()


# ---------------------------------------------------------------- 5. the env
def test_env_integration():
    a, b = make_env(4, 5, depth={}, elevation=True, autoreset=True), make_env(4, 5, depth={}, autoreset=True)
    assert b.elevation_map is None and b.elevation_obs is None and b.elevation_known is None
    assert a.elevation_obs.shape == (4, 171) and a.elevation_known.shape == (4, 117) and a.elevation_map.grid == 64
    rng = np.random.default_rng(6)
    for t in range(4):
        act = torch.from_numpy(np.tanh(rng.normal(size=(4, 12)) * 0.6).astype(np.float32)).cuda()
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        torch.cuda.synchronize()
        for x, y in ((oa["state"], ob["state"]), (oa["privileged_state"], ob["privileged_state"]), (ra, rb), (da, db), (a.buffers["state"], b.buffers["state"]),
                     (a.depth, b.depth)):
            assert np.array_equal(_bits(x), _bits(y)), t
        eo = _bits(a.elevation_obs)
        assert np.array_equal(eo[:, :38], _bits(oa["state"])[:, :38]) and np.array_equal(eo[:, 155:], _bits(oa["state"])[:, 155:])
        assert np.array_equal(eo[:, 38:155], _bits(a.elevation_map.est)) and np.isfinite(a.elevation_map.est.cpu().numpy()).all()
    assert a.elevation_known.sum() > 0 and (a.elevation_map.est > 0).any()
    # one acting step on the map's observation
    actor = FusedActor(a, T=2, seed=1, obs=a.elevation_obs)
    pi = load_policy("policy177", "cuda:0")
    actor.load([(m.weight, m.bias) for m in pi.layers], pi.mean, pi.std)
    actor.act()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(actor.storage["obs"][0]), _bits(a.elevation_obs)) and np.isfinite(actor.action.cpu().numpy()).all()
    # reset(mask) clears the masked envs' maps and leaves the others'
    a.elevation_map.map.fill_(9.0)
    a.reset(5, mask=torch.tensor([1, 0, 0, 1], dtype=torch.uint8))
    torch.cuda.synchronize()
    m = a.elevation_map.map.cpu().numpy()
    for e, masked in enumerate((1, 0, 0, 1)):
        assert (m[e] == 9.0).any() != bool(masked), e
        assert np.isnan(m[e]).any() == bool(masked), e
    a.elevation_map.map.fill_(9.0)
    a.reset(5)
    torch.cuda.synchronize()
    assert not (a.elevation_map.map == 9.0).any()
    # a new terrain table: every map forgets the old one's heights
    a.elevation_map.map.fill_(9.0)
    a.set_terrain(a.terrain)
    torch.cuda.synchronize()
    assert torch.isnan(a.elevation_map.map).all()
    a.close(); b.close()
    assert a.elevation_map is None


def test_elevation_and_student_together():
    from phase_guided_terrain_traversal_amd import perceive
    env = make_env(4, 3, depth={}, elevation=dict(grid=24), student=perceive.ScanEstimator())
    env.step(torch.zeros(4, 12, device="cuda:0"))
    torch.cuda.synchronize()
    assert env.student_obs.shape == env.elevation_obs.shape == (4, 171) and env.elevation_map.grid == 24
    env.close()


def test_refusals_on_the_device():
    camera, _ = recorded(16, 12)
    with pytest.raises(ValueError):
        elevation.ElevationMap(types.SimpleNamespace(depth_camera=None))
    rig = Rig(3, camera, grid=24)
    cc = depth_mod.config_struct(16, 12, 58.0, 0.1, 3.0, 0, (0, 0, 0), (1, 0, 0, 0), every=2)
    rig.env.depth_camera = types.SimpleNamespace(config=cc)
    with pytest.raises(ValueError, match="period 1"):
        elevation.ElevationMap(rig.env)
    cc.every, cc.mount_body = 1, 3
    with pytest.raises(ValueError, match="torso"):
        elevation.ElevationMap(rig.env)
    cc.mount_body = 0
    with pytest.raises(elevation.ElevationError):
        elevation.ElevationMap(rig.env, grid=97)
    rig.close()


# ---------------------------------------------------------------- 6. graph capture
def test_graph_capture():
    """one tick captured on a stream and replayed twice equals two eager ticks bit for bit; the tick is one kernel node, so the graph has no
    parallel branches"""
    camera, ticks = recorded(64, 48)
    settings = dict(grid=64, res=RES, alpha=0.5, self_half=(0.45, 0.25, 0.45))
    S, img, obs = ticks[0]
    a, b = Rig(3, camera, **settings), Rig(3, camera, **settings)
    for r in (a, b):
        r.put(S, img, obs)
        r.map.map.fill_(0.25)                                                     # alpha = 0.5 moves every touched cell at every tick
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.map.tick()
    torch.cuda.current_stream().wait_stream(s)
    b.map.tick()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.map.tick()
    torch.cuda.synchronize()
    for t in range(2):
        before = b.map.map.clone()
        g.replay(); b.map.tick()
        torch.cuda.synchronize()
        for k in ("map", "origin", "est", "known", "obs"):
            assert np.array_equal(_bits(getattr(a.map, k)), _bits(getattr(b.map, k))), (k, t)
        assert not torch.equal(torch.nan_to_num(before), torch.nan_to_num(b.map.map))
    a.close(); b.close()
