"""The elevation map's edge cases are what they claim (tests/elevation_edge_cases.py), shown with the fp32 twin and the fp64 references alone: no GPU.

  on the edge      every edge input sits on its edge: replaced by its neighbouring float, the twin decides otherwise
  agreement        with the edge inputs moved 1e-3 m off their edges, to either side, the twin and the fp64 references (elevation_points_reference,
                   elevation_reference, elevation_variance_reference, elevation_visibility_reference) decide alike - cells, known, origin, the update's
                   branches, the cleaned cells - and their values agree within the project's bars
  vacuity guards   the two cell rules do separate border points of family A at res = 0.04 and 0.12; all four update branches occur in H; every move
                   size occurs on both axes in D
  nothing left out no case carries a doubt mask or an exclusion list

J at res = 0.04: with the sensor at fl32(1.3) (the case "rules-apart") 4 of a ray's 11 samples are floats that the division rule would place in
another cell than the reciprocal rule does; the other cases' samples lie a quarter of a cell from every border and separate nothing.  The count is
printed and asserted to be at least 1; at res = 2^-5 both rules are exact and it is 0.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_edge_cases as ec  # noqa: E402
import elevation_visibility_reference as visref  # noqa: E402

F = np.float32
TWIN_FAMILIES = ("A", "B", "C", "D", "E", "F", "H", "J")


def _within(got, want, bar_of):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern"
    ok = ~np.isnan(want) & np.isfinite(want)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - want[ok]) / bar_of(want[ok])).max())


def height_bar(ref):
    return ec.HEIGHT_BAR * (1 + np.abs(ref))


def var_bar(ref):
    return ec.VAR_BAR * np.abs(ref) + 1e-30


def agree(case):
    """the twin against the fp64 references on one case (tick and hold ops: run_reference; clean ops: the visibility reference on the twin's state)
    -> the worst error over the bar"""
    twin = ec.run_twin(case)
    worst = 0.0
    S = case["S"]
    if all(t["op"] != "clean" for t in case["ticks"]):
        for t, a, b in zip(case["ticks"], twin, ec.run_reference(case)):
            assert np.array_equal(a["origin"], b["origin"]), (case["name"], "origin")
            assert np.array_equal(a["known"].astype(bool), np.asarray(b["known"], bool)), (case["name"], "known")
            worst = max(worst, _within(a["map"], b["map"], height_bar), _within(a["est"], b["est"], height_bar))
            if "obs_out" in b:
                worst = max(worst, _within(a["obs"], b["obs_out"], height_bar))
            if S["variance"] and t["op"] == "tick":
                assert np.array_equal(a["decisions"]["branch"], b["branch"]), (case["name"], "branch")
                assert np.array_equal(a["decisions"]["n"], np.where(b["touched"], b["n"], 0)), (case["name"], "n")
                worst = max(worst, _within(a["var"], b["var"], var_bar), _within(a["est_var"], b["est_var"], var_bar))
        return worst
    st = ec.new_state(S)
    for t, a in zip(case["ticks"], twin):
        if t["op"] == "clean":
            vis = S["visibility"]
            w = visref.visibility((st["map"], st["origin"]), np.array(t["qpos"], F).astype(float), ec.ref_cfg(S), vis, points=np.asarray(t["points"], F),
                                  var=st["var"] if S["variance"] else None, skip=t.get("clear", False))
            dec, vd = w["bound_decided"], w["verdict_decided"]
            if case.get("border_samples"):
                # samples that are floats next to a border are in doubt for the fp64 reference whatever the ray's end is moved by: there the twin's
                # bound lies between the reference's two, and the rest is compared as everywhere
                und = ~dec & ~np.isnan(a["bound"])
                assert 0 < (~dec).sum() <= 12 and (a["bound"][und] >= w["bound_any"][und] - height_bar(w["bound_any"][und])).all(), case["name"]
            else:
                assert dec.all() and vd.all(), (case["name"], "the reference is in doubt")
            gone = np.isnan(a["map"]) & ~np.isnan(st["map"])
            assert np.array_equal(gone[vd], w["clear_sure"][vd]) and (not vd.all() or int(a["cleared"]) == w["cleared"]), (case["name"], "verdicts")
            worst = max(worst, _within(np.where(dec, a["bound"], np.nan), np.where(dec, w["bound_sure"], np.nan), height_bar))
        st = dict(map=a["map"], origin=a["origin"], var=a.get("var"))
    return worst


def moved(case, sign):
    """the case with every edge input moved 1e-3 m: sign = +1 across its edge, -1 away from it"""
    c = case
    for e in case["edges"]:
        # J: a ray end moved by 1e-3 m moves its bounds by up to 7e-4 m, so the heights on the verdict's edge move 5e-3 m
        c = ec.with_edge_moved(c, e, by=sign * (5e-3 if case["family"] == "J" and e[0] == 0 else 1e-3))
    return c


@pytest.mark.parametrize("fam", TWIN_FAMILIES)
def test_on_the_edge(fam):
    n_edges = 0
    for case in ec.family(fam):
        base = ec.decisions(case)
        for e in case["edges"]:
            assert not ec.same_decisions(base, ec.decisions(ec.with_edge_moved(case, e))), (case["name"], e, "the neighbouring float decides alike")
            n_edges += 1
    print(f"family {fam}: {len(ec.family(fam))} cases, {n_edges} edge inputs")
    if fam in ("A", "C", "F", "H", "J"):
        assert n_edges > 0


@pytest.mark.parametrize("fam", TWIN_FAMILIES)
def test_agreement_with_the_fp64_references(fam):
    worst = 0.0
    for case in ec.family(fam):
        if fam == "D" and case["S"]["grid"] == 96:
            continue                                                              # the same code path as G = 24, and minutes of fp64 reference
        variants = [moved(case, +1), moved(case, -1)] if case["edges"] else [case]
        for c in variants:
            worst = max(worst, agree(c))
    print(f"family {fam}: twin against the fp64 references, worst error / bar {worst:.3g}")
    assert worst <= 1.0


def test_the_bar_cases_are_off_every_edge_and_family_g_is_lit():
    """the cases held to the bars take their expected values from the fp64 references; family G's pixels are at least 1e-3 m from every cell border"""
    lit = 0
    for case in ec.family("G"):
        (o,) = ec.run_reference(case)
        v = o["valid"]
        if v.any():
            assert o["margin"][v].min() >= 1e-3, (case["name"], float(o["margin"][v].min()))
        n = int((~np.isnan(o["map"])).sum())
        assert n == int(v.sum()) <= 1, case["name"]
        lit += n
        if "lit" in case:
            assert bool(n) == case["lit"], case["name"]
    print(f"family G: {len(ec.family('G'))} cases, {lit} with their one pixel in a cell")
    assert lit >= 2 * (sum(w * h for w, h in ec.G_SHAPES) + 2)


def test_vacuity_guards():
    # A: border points that the reciprocal rule would put into another cell
    for res in (0.04, 0.12, 2.0 ** -5):
        n = tot = 0
        for case in ec.family("A"):
            if case["S"]["res"] == res:
                p = case["ticks"][0]["points"]
                for ax in (0, 1):
                    n += int((ec.cell(p[:, ax], res) != ec.cell_recip(p[:, ax], res)).sum())
                    tot += len(p)
        print(f"family A, res = {res:g}: {n} of {tot} border coordinates fall into another cell under x * (1 / res)")
        assert n >= 1 or res == 2.0 ** -5
    # J: samples that the division rule would place elsewhere
    for res in (0.04, 2.0 ** -5):
        n = tot = 0
        for case in ec.family("J"):
            if case["S"]["res"] == res:
                for o in ec.run_twin(case):
                    for x, y in o.get("samples", []):
                        tot += 1
                        n += int(ec.cell(x, res) != ec.cell_recip(x, res) or ec.cell(y, res) != ec.cell_recip(y, res))
        print(f"family J, res = {res:g}: {n} of {tot} samples fall into another cell under floor(x / res)")
        assert tot > 50 and (n >= 1 or res != 0.04)
    # H: all four branches of the update; D: every move size on both axes
    seen = set()
    for case in ec.family("H"):
        if case["mode"] == "bits":
            for o in ec.run_twin(case):
                seen |= set(np.unique(o["decisions"]["branch"]).tolist())
    assert {1, 2, 3, 4} <= seen, seen
    for G in (8, 9, 24):
        moves = {c["move"] for c in ec.family("D") if c["S"]["grid"] == G and "move" in c}
        for mv in ec.D_MOVES(G):
            assert {(mv, "x"), (mv, "y"), (mv, "xy")} <= moves, (G, mv)


def test_family_d_keeps_the_intersection_of_the_windows():
    """the surviving cells are exactly the intersection of the two windows, with their bits, in their slots"""
    for case in ec.family("D"):
        if "move" not in case:
            continue
        G = case["S"]["grid"]
        o = ec.run_twin(case)
        wc0, wc1 = (ec.eref.world_cells(x["origin"], G) for x in o[:2])
        same = (wc0 == wc1).all(-1)
        assert np.array_equal(~np.isnan(o[1]["map"]), same) and np.array_equal(ec.bits(o[1]["map"])[same], ec.bits(o[0]["map"])[same]), case["name"]
        mv = abs(case["move"][0])
        assert int(same.sum()) == (max(G - mv, 0) ** 2 if case["move"][1] == "xy" else G * max(G - mv, 0)), case["name"]


def test_nothing_left_out():
    """no doubt mask, no exclusion list: every expected field is a full array, and the share of compared cells left out is 0"""
    total = 0
    for fam in ec.FAMILIES:
        for case in ec.family(fam):
            assert not {"doubt", "doubtful", "exclude", "excluded", "mask", "skip", "xfail"} & set(case), case["name"]
            assert case["mode"] in ("bits", "ref") and set(case["marks"].values()) <= {"bar"}
            total += 1
    G = ec.family("E")[0]["S"]["grid"]
    for e in ec.expected(ec.family("E")[0]):
        assert e["map"][1].shape == (G, G) and e["est"][1].shape == (ec.NSCAN,) and e["known"][1].shape == (ec.NSCAN,)
    print(f"{total} cases in {len(ec.FAMILIES)} families, none with an exclusion")
