"""The elevation map's kernels at the exact edges of their contract (include/pgtt_elevation.h): the case families of tests/elevation_edge_cases.py
driven through elevation.ElevationMap on hand-filled tensors.  Every family, every output it names - map, origin, est, known, obs, var, est_var,
cleared, bound - and every cell of each: no doubt mask, no exclusion list, nothing skipped.  A field marked "bits" is compared as int32 (a NaN is a
NaN); a field marked "bar" at the project's bars, 2e-5 (1 + |ref|) on heights and 1e-4 relative on variances.

Cases that share settings run as the envs of one launch, at most 64; env 0 is a second copy of the batch's last case, so every case is also held
at a non-zero batch position.  What the cases are, and that they sit on their edges, is shown on the CPU by tests/test_elevation_edge_cases.py.

Measured on an MI355X (pytest -m gpu -s prints the line of each family).  All nine families pass; no family exposed a defect of a kernel, and
pgtt_elevation.hip is unchanged.  Worst error over the bar among the fields held to the bars:

    family  cases  of them with `bar` fields                               worst error / bar
    E          4   1   alpha = 0.3 on values that are not dyadic                0.0007
    F         13   2   the base quaternion multiplied by 3                      0.0000 (the same bits)
    G        194   194 the image source: pgtt_elevation, pgtt_elevation_var     0.0024
    H          9   1   sigma_rel > 0                                            0.0014
    A, B, C, D, J: every field bit for bit; so are the other cases of E, F and H.

That the cases can fail was tried with two libraries built from kernel sources with comparisons changed, twenty in all.  The first: x * (1 / res)
in the tick's cell rule, < for <= in the self box, the band and the gate, >= for > in `near < d` and in the verdict, < for <= in
r_k <= Lh - end_guard, 3 G for the cap 2 G, the key without its sign fold, alpha = 1 through h + alpha (m - h), min(n, max_count) dropped, the row
wrap of the variance tick's float4 image loop dropped, the sanity test of the stored origin dropped.  The second: the recentre without its y axis,
`var` left standing where the recentre or the clean-up forgets `map`, P / stride rays for ceil(P / stride), floor(x + 0.5) for rint, the hold
call's window one cell off for an even G, est at an unknown point not 0.  Every family failed on the cases named for the changed comparison, but
for one change: dropping the origin's sanity test changes nothing, because an origin that far away makes every slot stale by the recentre rule
itself.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_edge_cases as ec  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, depth as depth_mod, elevation  # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ("map", "origin", "est", "known", "obs", "var", "est_var", "cleared", "bound")
VARIANCES = ("var", "est_var")
F = np.float32


class Rig:
    """what ElevationMap reads of an env - state, image or points, observation, the sensors' configs and the sensor's counter - as tensors the test
    fills, and the map on them"""

    def __init__(self, n, S, points=None):
        dev = torch.device("cuda:0")
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)
        cam = S["camera"] or dict(width=1, height=1, fovy=90.0, near=0.1, far=1.0, mount_pos=(0.0, 0.0, 0.0), mount_quat=(1.0, 0.0, 0.0, 0.0))
        cc = depth_mod.config_struct(cam["width"], cam["height"], cam["fovy"], cam["near"], cam["far"], 0, cam["mount_pos"], cam["mount_quat"])
        self.env = types.SimpleNamespace(depth=z(n, cam["height"], cam["width"]), depth_camera=types.SimpleNamespace(config=cc),
                                         buffers={"state": z(abi.NSTATE, n), "obs_state": z(n, ec.OBS_DIM), "done": z(n)}, device=dev, num_envs=n,
                                         observation_size={"state": ec.OBS_DIM}, config=dict(scan_dist_x=S["sdx"], scan_dist_y=S["sdy"]),
                                         method={38: "pgtt", 30: "baseline"}[S["row0"]], dt=0.02, env_id_offset=0)
        kw = dict(grid=S["grid"], res=S["res"], alpha=S["alpha"], self_half=S["self_half"], follow_sensor=S["follow"])
        vis = S["visibility"]
        if points is not None:
            self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
            self.env.lidar_scanner = types.SimpleNamespace(points=z(n, points, 3), counter=self.counter, config=types.SimpleNamespace(
                every=2 if S["follow"] else 1, mount_body=0, mount_pos=tuple(vis["sensor_pos"]) if vis else (0.0, 0.0, 0.0)))
            kw["source"] = "lidar"
        if S["variance"]:
            kw["variance"] = dict(S["variance"])
        if vis:
            kw.update(visibility={k: vis[k] for k in ("margin", "end_guard", "stride", "sigmas")}, dense_bound=True)
        self.map = elevation.ElevationMap(self.env, **kw)
        assert self.map.config.scan_row0 == S["row0"]

    def put(self, qpos, obs, points=None, image=None):
        S = np.zeros((abi.NSTATE, len(qpos)), F)
        S[:7] = np.asarray(qpos, F).T
        self.env.buffers["state"].copy_(torch.from_numpy(S))
        self.env.buffers["obs_state"].copy_(torch.from_numpy(np.ascontiguousarray(obs, F)))
        if points is not None:
            self.env.lidar_scanner.points.copy_(torch.from_numpy(np.ascontiguousarray(points, F)))
        if image is not None:
            self.env.depth.copy_(torch.from_numpy(np.ascontiguousarray(image, F)))

    def out(self):
        torch.cuda.synchronize()
        return {k: getattr(self.map, k).cpu().numpy().copy() for k in OUTS if hasattr(self.map, k)}

    def close(self):
        self.map.close()


def hold_field(name, mark, want, got, where):
    """one field of one env -> its error over the bar (0 for a field held bit for bit)"""
    want, got = np.asarray(want), np.asarray(got)
    if want.dtype.kind in "iub" or got.dtype.kind in "iu":
        assert mark == "bits" and np.array_equal(want.astype(np.int64), got.astype(np.int64)), (where, name, want.tolist() if want.size < 8 else "")
        return 0.0
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(got)), (where, name, "NaN pattern", np.argwhere(nan != np.isnan(got))[:6].tolist())
    if mark == "bits":
        a, b = ec.bits(want.astype(F))[~nan], ec.bits(got)[~nan]
        bad = np.nonzero(a != b)[0]
        assert not len(bad), (where, name, "bits", len(bad), want[~nan][bad[:4]].tolist(), got[~nan][bad[:4]].tolist())
        return 0.0
    w, g = want[~nan].astype(float), got[~nan].astype(float)
    if not w.size:
        return 0.0
    fin = np.isfinite(w)
    assert np.array_equal(w[~fin], g[~fin]), (where, name, "infinities")
    bar = ec.VAR_BAR * np.abs(w[fin]) + 1e-30 if name in VARIANCES else ec.HEIGHT_BAR * (1 + np.abs(w[fin]))
    ratio = np.abs(g[fin] - w[fin]) / bar
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, (where, name, "over the bar", worst)
    return worst


def run_batch(cases):
    """one launch sequence for cases that share settings -> (fields compared, the worst error over the bar among the `bar` fields, what failed)"""
    envs = [cases[-1]] + list(cases)
    n, S = len(envs), cases[0]["S"]
    assert n <= 64
    want = [ec.expected(c) for c in cases]
    want = [want[-1]] + want
    t0 = cases[0]["ticks"][0]
    rig = Rig(n, S, points=None if S["camera"] else len(t0["points"]))
    worst, fields, problems = 0.0, 0, []
    try:
        for ti in range(len(cases[0]["ticks"])):
            ticks = [c["ticks"][ti] for c in envs]
            op = ticks[0]["op"]
            obs = np.stack([t["obs"] if t.get("obs") is not None else np.zeros(ec.OBS_DIM, F) for t in ticks])
            src = {}
            if ticks[0].get("points") is not None:
                src["points"] = np.stack([t["points"] for t in ticks])
            if ticks[0].get("image") is not None:
                src["image"] = np.stack([t["image"] for t in ticks])
            rig.put(np.stack([t["qpos"] for t in ticks]), obs, **src)
            if any(t.get("origin_in") is not None for t in ticks):
                o = rig.map.origin.cpu().numpy()
                for e, t in enumerate(ticks):
                    if t.get("origin_in") is not None:
                        o[e] = np.array(t["origin_in"], np.int64).astype(np.int32)
                rig.map.origin.copy_(torch.from_numpy(o))
            mask = torch.tensor([1 if t.get("clear", False) else 0 for t in ticks], dtype=torch.uint8)
            if S["follow"]:
                rig.counter.fill_(1 if op == "tick" else 2)                       # every = 2: the counter behind a sensor call that was fresh / was not
            if op == "clean":
                rig.map.clean(clear_mask=mask)
            else:
                rig.map.tick(clear_mask=mask)
            got = rig.out()
            for e, c in enumerate(envs):
                for name, (mark, w) in want[e][ti].items():
                    assert name in got, (c["name"], name, "the map has no such output")
                    try:                                                          # every field of every case is looked at; the family fails on the list
                        worst = max(worst, hold_field(name, mark, w, got[name][e], (c["name"], f"tick {ti}", f"env {e}")))
                    except AssertionError as err:
                        problems.append(str(err)[:400])
                    fields += 1
    finally:
        rig.close()
    return fields, worst, problems


@pytest.mark.parametrize("fam", list(ec.FAMILIES))
def test_family(fam):
    cases = ec.family(fam)
    worst, fields, launches, problems = 0.0, 0, 0, []
    for batch in ec.batches(cases):
        f, w, p = run_batch(batch)
        fields, worst, launches, problems = fields + f, max(worst, w), launches + 1, problems + p
    nbar = sum(1 for c in cases if c["mode"] == "ref" or c["marks"])
    print(f"family {fam}: {len(cases)} cases ({nbar} with fields at the bars) in {launches} batches, {fields} fields compared, "
          f"worst error / bar of the bar fields {worst:.4f}")
    assert fields > 0
    assert not problems, (len(problems), problems[:12])
