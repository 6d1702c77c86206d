"""The inputs of tests/test_gpu_collision_edges.py are fair: from the CPU oracle alone (no GPU), every family of tests/collision_cases.py keeps its
share of doubtful envs under its cap, reaches what it is aimed at (the coverage minima), and expects what it was built to expect; the carried-proof
workloads visit all four classes on the fp32 oracle's own one-substep trajectories."""
import numpy as np
import pytest

import collision_cases as CC


@pytest.mark.parametrize("name", CC.FAMILIES)
def test_doubtful_share_is_under_the_cap(name):
    ref = CC.reference(name)
    print(f"\n[{name}] envs {ref['envs']}, doubtful share {ref['doubtful_share']:.4f} (cap {CC.CAPS[name]}), dist bar {ref['bar']:.3e} "
          f"(4 x fp32-vs-fp64 = {ref['bar_measured']:.3e}, floor 8 ulp of {ref['max_coord']:.1f} m = {ref['bar_floor']:.3e})")
    assert ref["doubtful_share"] <= CC.CAPS[name]
    assert all(bt["n"] <= 128 for bt in CC.family(name))


def test_a1_expects_one_box_contact_per_env_and_walks_every_box_and_foot():
    for bt, r in zip(CC.family("A1"), CC.reference("A1")["batches"]):
        for e in range(bt["n"]):
            assert CC.box_pairs(r["sets"][e]) == [(e % 4, e)], (bt["label"], e, r["sets"][e])
            assert abs(r["dist"][e][(e % 4, e)] + 0.005) < 1e-6
    cov = CC.coverage("A1")
    print("\n[A1]", cov)
    assert cov["box indices pressed"] == 100 and cov["feet used"] == 4
    assert [bt["n"] % 16 for bt in CC.family("A1")] == [4, 5]               # partial last waves


def test_a2_uses_every_grid_line_from_the_neighbouring_cell():
    fam, ref = CC.family("A2"), CC.reference("A2")
    for bt, r in zip(fam[:2], ref["batches"][:2]):
        for e in range(bt["n"]):
            pair = (int(bt["foot"][e]), int(bt["box"][e]))
            assert CC.box_pairs(r["sets"][e]) == [pair], (bt["label"], e, r["sets"][e])
            assert abs(r["dist"][e][pair] + 0.0075) < 1e-5                  # the side face, 7.5 mm in
    bt, r = fam[2], ref["batches"][2]
    for e in range(bt["n"]):
        want = [(int(bt["foot"][e]), int(bt["box"][e]))] if bt["box"][e] >= 0 else []
        assert [p for p in CC.box_pairs(r["sets"][e]) if p[0] == bt["foot"][e]] == want, (e, r["sets"][e])
    cov = CC.coverage("A2")
    print("\n[A2]", cov)
    assert cov["x lines used"] == 15 and cov["y lines used"] == 15
    assert cov["foot cell differs from the box centre's"] >= 40


def test_a3_expectations_and_the_scan_points_left_out():
    fam, ref = CC.family("A3"), CC.reference("A3")
    E = [float(CC.grid_of(bt["terrain"])[0]) for bt in fam]
    assert abs(E[0] - 1.6176) < 1e-3 and E[1] == 1.0
    seen = set()
    for bt, r in zip(fam, ref["batches"]):
        for e in range(bt["n"]):
            w, boxes = str(bt["what"][e]), CC.box_pairs(r["sets"][e])
            seen.add(w)
            if w == "i":
                assert boxes == [] and len(r["sets"][e]) == 4, (e, r["sets"][e])            # plane contacts only
            else:
                assert len(boxes) >= 1, (bt["label"], w, e, r["sets"][e])
            if w == "iii":
                assert {b for _, b in boxes} == {2}
            if w == "iv":
                assert {b for _, b in boxes} <= {3, 4}
    assert seen == {"i", "ii", "iii", "iv", "v", "map"}
    assert ref["max_coord"] > 160.0
    for (Z, M), bt in zip(CC.scan_reference(), fam):
        print(f"\n[A3 scan, {bt['label']}] points {M.size}, left out {int(M.sum())} ({M.mean():.4f}, cap {CC.SCAN_LEFT_OUT_CAP}); highest hit {Z.max():.1f} m")
        assert M.mean() <= CC.SCAN_LEFT_OUT_CAP
        assert Z.max() > 100.0 and Z.min() == 0.0


def test_a4_reaches_every_narrow_phase_class():
    cov = CC.coverage("A4")
    print("\n[A4]", cov)
    for c in ("face", "edge", "corner", "inside", "inside margin >= 1 mm", "deeper than the radius"):
        assert cov[c] >= 8, (c, cov)
    bt, r = CC.family("A4")[0], CC.reference("A4")["batches"][0]
    for e in range(bt["n"]):
        if not r["doubtful"][e]:
            assert (int(bt["foot"][e]), int(bt["box"][e])) in r["sets"][e], e


def test_a5_reaches_the_many_box_pass_and_the_cut():
    cov = CC.coverage("A5")
    print("\n[A5]", cov)
    assert cov["envs with more than four penetrating boxes under a foot"] >= CC.MANY_BOX_MIN
    assert cov["envs with a penetrating pair removed by the cut"] >= CC.CUT_MIN


@pytest.mark.parametrize("nsub", CC.CARRY_SUBSTEPS)
def test_carry_workloads_visit_all_four_classes_on_the_fp32_oracle(nsub):
    total = dict(a=0, b=0, c=0, d=0)
    for name in ("dense", "random"):
        w = CC.carry_workload(name)
        speed = np.linalg.norm(w["qvel"][:, :2], axis=1)
        assert speed.min() >= (4 if name == "dense" else 2) and speed.max() <= (30 if name == "dense" else 15)
        cnt = CC.carry_classes(name, CC.oracle_one_substep_chain(name)[:nsub])
        print(f"\n[carry, {name}, {nsub} substeps] classes {cnt}")
        for k in total:
            total[k] += cnt[k]
    print(f"[carry, {nsub} substeps] both workloads {total}, minima {CC.CARRY_MIN}")
    for k, m in CC.CARRY_MIN.items():
        assert total[k] >= m, (k, total)


@pytest.mark.parametrize("nsub", CC.CARRY_SUBSTEPS)
def test_whole_waves_establish_drop_and_carry_the_proof_on_the_fp32_oracle(nsub):
    """physics_kernel carries the proof per WAVE, so the per-env classes above say nothing about what a wave does: the "waves" workload lays whole waves
    out to carry, and whole waves out to meet - with a proof established earlier in the launch by every env of the wave - a substep in which the cut
    removes a penetrating pair; counted with the model of collide()'s rule, for the wave sizes of all three lane layouts"""
    chain = CC.oracle_one_substep_chain("waves")[:nsub]
    for layout, m in CC.WAVE_ENVS.items():
        cnt = CC.carry_waves("waves", chain, m)
        print(f"\n[carry waves, {layout} ({m} envs per wave), {nsub} substeps] {cnt}, minima {CC.WAVE_MIN}")
        for k, lo in CC.WAVE_MIN.items():
            assert cnt[k] >= lo, (layout, k, cnt)
        assert cnt["unsound"] == 0
    for name in ("dense", "random"):
        assert all(CC.carry_waves(name, CC.oracle_one_substep_chain(name)[:nsub], m)["unsound"] == 0 for m in CC.WAVE_ENVS.values())
