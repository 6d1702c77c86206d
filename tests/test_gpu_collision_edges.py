"""physics_kernel's collision stage against the brute-force oracle at its edges, exactly: no W, no mismatch allowance, no post-mortem.

Part A.  With ctrl_dt = sim_dt the contact records of one launch (dbg_contact, dbg_dist) depend on the input qpos and the terrain alone, so for every
env that the REFERENCE does not call doubtful (tests/collision_cases.py: fp32 and fp64 oracle agree, and the fp64 set survives base shifts of 2e-6 m x
max(1, |coordinate|)) the device's set {(foot, geom) : dist < 0} must EQUAL the fp64 oracle's, every distance in it must lie within the family's bar
(4 x the fp32 oracle's own error against fp64, at least 8 fp32 ulp of the family's largest foot coordinate), and every number written must be finite.
Families: A1 every box index and every foot (100 pillars; B = 37, T = 3 on the last variant), A2 feet on the lines of the terrain grid, from the
neighbouring cell, A3 feet off the map (the plane at 40 m, placeholders at 100 - 198 m, boxes that the grid's extent ignores) with the scan there,
A4 the narrow phase's branches on rotated boxes, A5 the selection, the many-box pass and the max_geom_pairs cut on the crafted terrains of the parity suite.

Part B.  One launch of a control step of 4 and of 8 substeps against as many one-substep launches of the same layout on the same batch, bit for bit:
bases at 2 - 30 m/s over the dense terrain and over 100 random boxes, with the four per-env classes counted from the one-substep records.  The
kernel decides per WAVE whether the proof is carried, so a third workload is laid out per wave (collision_cases.pit_terrain): waves whose every env
carries, waves whose every env establishes the proof and then sinks onto a beam whose pair the max_geom_pairs cut removes, and waves that fall
37 mm towards buried cubes so that only the displacement term of the proof tells that it no longer holds - the wave-substeps that carry and the
env-substeps at which a kept proof would change a bit are counted from the device's records per wave of the layout.

Measured on MI355X; hex, oct and quad gave the same figures.  Envs compared / left out as doubtful, set mismatches, the `dist` bar (the measured part
4 x |fp32 oracle - fp64 oracle|, the floor 8 ulp of the largest foot coordinate) and the largest device error / bar:
    A1  137 / 0   0 mismatches   bar 1.907e-06 (measured 2.344e-08, floor at 2.6 m)    error / bar 0.011
    A2  200 / 0   0 mismatches   bar 1.907e-06 (measured 7.799e-07, floor at 3.9 m)    error / bar 0.117
    A3   42 / 0   0 mismatches   bar 1.221e-04 (measured 3.011e-06, floor at 198.7 m)  error / bar 0.006; scan: 4910 points compared, 4 left out, largest error 4.5e-08
    A4  128 / 0   0 mismatches   bar 4.768e-07 (measured 3.596e-07, floor at 1.0 m)    error / bar 0.145
    A5  189 / 0   0 mismatches   bar 9.537e-07 (measured 4.076e-07, floor at 1.2 m)    error / bar 0.087; 96 envs took the many-box pass, 139 lost a penetrating pair to the cut
    B   bit-identical on 96 envs x 3 workloads x {4, 8} substeps; classes a / b / c / d over "dense" and "random": 177 / 181 / 16 / 138 (4 substeps),
        613 / 372 / 49 / 320 (8).  "waves", per wave of the layout, 4 / 8 substeps: wave-substeps that carry hex 32 / 64, oct 16 / 32, quad 8 / 16 (minimum 4);
        env-substeps at which a proof that was never dropped would change a bit 64 (minimum 16), at which one dropped on thr alone would 32 (minimum 16)
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import collision_cases as CC
import parity_explain as X
import test_gpu_parity as G

PEN_OVERFLOW = 0x10000          # PGTT_DBG_PEN_OVERFLOW


@pytest.fixture(params=["hex", "oct", "quad"])
def layout(request):
    return request.param


def launch(bt, layout, scan=False):
    """one physics launch of one mjx.step from the batch's poses (zero velocity, zero warm start, zero action) -> numpy records"""
    from phase_guided_terrain_traversal_amd.env import Joystick
    n = bt["n"]
    env = Joystick("stairs", CC.config(), num_envs=n, terrain=bt["terrain"], device="cuda:0", variant=torch.from_numpy(bt["variant"]), layout=layout,
                   debug_contacts=True)
    env.reset(3)
    torch.cuda.synchronize()
    S = env.buffers["state"].cpu().numpy()
    S[:19] = bt["qpos"].T
    S[19:55] = 0.0
    env.buffers["state"].copy_(torch.from_numpy(S))
    out = {}
    if scan:
        out["scan"] = env.scan().cpu().numpy().copy()
    env.physics(torch.zeros((n, 12), dtype=torch.float32, device="cuda:0"))
    torch.cuda.synchronize()
    out.update(con=env.buffers["dbg_contact"].cpu().numpy().reshape(n, 8, 2), dist=env.buffers["dbg_dist"].cpu().numpy(),
               niter=env.buffers["dbg_niter"].cpu().numpy(), state=env.buffers["state"].cpu().numpy(), scan_z=env.buffers["scan_z"].cpu().numpy())
    env.close()
    return out


def hold_family(name, layout, scan=False):
    """the three assertions of part A on every batch of a family -> the device records per batch"""
    fam, ref = CC.family(name), CC.reference(name)
    compared = left_out = 0
    worst, mism, recs = 0.0, [], []
    for bt, r in zip(fam, ref["batches"]):
        g = launch(bt, layout, scan=scan)
        recs.append(g)
        assert np.isfinite(g["state"]).all() and np.isfinite(g["dist"]).all() and np.isfinite(g["scan_z"]).all(), (name, bt["label"])
        sets = G.active_sets(g["con"], g["dist"])
        for e in range(bt["n"]):
            if r["doubtful"][e]:
                left_out += 1
                continue
            compared += 1
            if sets[e] != r["sets"][e]:
                feet = {f for f, _ in set(sets[e]) ^ set(r["sets"][e])}
                mism.append(dict(family=name, batch=bt["label"], env=e, device=sets[e], oracle=r["sets"][e],
                                 feet={f: r["feet64"][e, f].tolist() for f in feet}))
                continue
            for (f, b), d in zip(g["con"][e], g["dist"][e]):
                if d < 0 and b != -2:
                    worst = max(worst, abs(float(d) - r["dist"][e][(int(f), int(b))]))
    print(f"\n[{name} {layout}] envs compared {compared}, left out {left_out}; set mismatches {len(mism)}; dist bar {ref['bar']:.3e} "
          f"(measured part {ref['bar_measured']:.3e}, floor {ref['bar_floor']:.3e}), device error / bar {worst / ref['bar']:.3f}")
    assert not mism, mism[:4]
    assert worst <= ref["bar"], (name, worst, ref["bar"])
    return recs


def test_a1_every_box_index_and_every_foot(layout):
    hold_family("A1", layout)


def test_a2_feet_on_the_grid_lines(layout):
    hold_family("A2", layout)


def test_a3_off_the_map_with_the_scan(layout):
    recs = hold_family("A3", layout, scan=True)
    for g, (Z, M), bt in zip(recs, CC.scan_reference(), CC.family("A3")):
        err = np.abs(g["scan"] - Z)
        assert np.isfinite(g["scan"]).all()
        print(f"[A3 scan {layout}, {bt['label']}] points compared {int((~M).sum())}, left out {int(M.sum())}; largest error {err[~M].max():.2e} (bar {CC.SCAN_BAR})")
        assert M.mean() <= CC.SCAN_LEFT_OUT_CAP
        bad = np.argwhere((err > CC.SCAN_BAR) & ~M)
        assert len(bad) == 0, (bt["label"], bad[:5].tolist(), err[~M].max())


def test_a4_narrow_phase_branches_on_rotated_boxes(layout):
    hold_family("A4", layout)


def test_a5_selection_the_many_box_pass_and_the_cut(layout):
    recs = hold_family("A5", layout)
    many = sum(int(((g["niter"] & PEN_OVERFLOW) != 0).sum()) for g in recs)
    cut = CC.coverage("A5")["envs with a penetrating pair removed by the cut"]
    print(f"[A5 {layout}] envs that took the many-box pass {many} (minimum {CC.MANY_BOX_MIN}); envs with a penetrating pair removed by the cut {cut} (minimum {CC.CUT_MIN})")
    assert many >= CC.MANY_BOX_MIN and cut >= CC.CUT_MIN
    assert all(((g["niter"] & 0xFFFF) <= 5).all() for g in recs)


@pytest.mark.parametrize("nsub", CC.CARRY_SUBSTEPS)
def test_b_one_launch_equals_its_one_substep_launches(layout, nsub):
    """the proof carried over the substeps of a launch changes no bit: qpos, qvel, qacc, dbg_contact, dbg_dist and dbg_niter of ONE launch of nsub
    substeps equal those of nsub one-substep launches (which remember nothing).  "dense" and "random" are the fast scattered workloads with their per-env
    classes; "waves" is laid out per wave, because the kernel carries per wave: whole waves that carry with a penetrating pair present, and whole
    waves in which every env established the proof and then meets a substep whose cut removes a penetrating pair - a kernel that kept the proof there
    would keep the pair and differ in dbg_contact"""
    from phase_guided_terrain_traversal_amd.env import Joystick
    total = dict(a=0, b=0, c=0, d=0)
    for name in ("dense", "random", "waves"):
        w = CC.carry_workload(name)
        n = CC.CARRY_N
        cfg = CC.config()
        cfg["ctrl_dt"] = cfg["sim_dt"] * nsub
        env = Joystick("stairs", cfg, num_envs=n, terrain=w["terrain"], device="cuda:0", variant=torch.from_numpy(w["variant"]), layout=layout, debug_contacts=True)
        env.reset(3)
        torch.cuda.synchronize()
        S0 = env.buffers["state"].cpu().numpy()
        S0[:19] = w["qpos"].T; S0[19:37] = w["qvel"].T; S0[37:55] = 0.0
        env.buffers["state"].copy_(torch.from_numpy(S0))
        act = np.zeros((n, 12), np.float32)
        env.physics(torch.from_numpy(act).cuda())
        torch.cuda.synchronize()
        one = dict(state=env.buffers["state"][:55].cpu().numpy(), con=env.buffers["dbg_contact"].cpu().numpy(), dist=env.buffers["dbg_dist"].cpu().numpy(),
                   niter=env.buffers["dbg_niter"].cpu().numpy())
        dev = X.DeviceSubsteps("stairs", env.config, env.model, w["terrain"], layout, n, {"variant": w["variant"]}, lifted=False)
        S, qpos_in, ni_max, flags = S0, [], np.zeros(n, np.int64), np.zeros(n, np.int64)
        for k in range(nsub):
            qpos_in.append(S[:19].T.copy())
            dev(np.arange(n), S, act, None, 1)
            S = dev.env.buffers["state"].cpu().numpy()
            ni = dev.env.buffers["dbg_niter"].cpu().numpy().astype(np.int64)
            ni_max, flags = np.maximum(ni_max, ni & 0xFFFF), flags | (ni & ~0xFFFF)
        many = dict(state=S[:55], con=dev.env.buffers["dbg_contact"].cpu().numpy(), dist=dev.env.buffers["dbg_dist"].cpu().numpy(), niter=(ni_max | flags).astype(np.int32))
        dev.close(); env.close()
        assert np.isfinite(one["state"]).all()
        for key in ("state", "con", "dist", "niter"):
            diff = np.nonzero((one[key] != many[key]).reshape(-1, n).any(0) if key == "state" else (one[key] != many[key]).reshape(n, -1).any(1))[0]
            assert len(diff) == 0, (name, layout, nsub, key, "envs", diff[:8].tolist())
        cnt = CC.carry_classes(name, np.asarray(qpos_in))
        moved = np.linalg.norm(S[:2] - S0[:2], axis=0)
        print(f"\n[carry {layout}, {name}, {nsub} substeps] bit-identical on {n} envs; classes {cnt}; bases moved {moved.min():.2f} - {moved.max():.2f} m")
        if name == "waves":
            # the kernel decides per WAVE: whole waves that carry, and whole waves that hold a proof when the cut starts to remove a pair
            wv = CC.carry_waves(name, np.asarray(qpos_in), CC.WAVE_ENVS[layout])
            print(f"[carry {layout}, waves of {CC.WAVE_ENVS[layout]} envs, {nsub} substeps] {wv}, minima {CC.WAVE_MIN}")
            for k, lo in CC.WAVE_MIN.items():
                assert wv[k] >= lo, (layout, k, wv)
            assert wv["unsound"] == 0
            continue
        for k in total:
            total[k] += cnt[k]
    print(f"[carry {layout}, {nsub} substeps] both workloads {total}, minima {CC.CARRY_MIN}")
    for k, m in CC.CARRY_MIN.items():
        assert total[k] >= m, (k, total)
