"""The bracketing rounds of physics_kernel's line search keep their trial steps in role order and take the first butterfly step of their row sums crossed
(QSolver::ls_points' paired form, pair_sum2: slot 0 plus the pair partner's slot 1).  The two addends of every sum are the ones
the replicated form added (tests/test_crossed_butterfly_model.py has the argument), so every build reproduces, bit for bit, what the commit before
computed (tests/golden/linesearch_crossed_parent.npz, recorded by tools/gen_golden_linesearch_crossed.py on that commit) where
tests/test_gpu_linesearch_roles.py does not look:
 - crowded: feet on three or four box contacts - the (slot 2, slot 3) row pair of hex (the crowded wave's own copy of the round loop), quad's `k >= 2`
   slot loop, oct's `units() > 2`.  That the case is what it says is asserted on the build under test: the same number of env-steps with a foot on
   >= 3 box slots as in the record, and more than none;
 - dr: level13 with full domain randomisation - the HAS_DR kernels, oct's per-lane-cap kernels among them;
 - ls2: level4 with ls_iterations = 2 - the round loop leaves by its cap, after the second round.
Hex / oct / quad, N = 13 (ragged last wave in every layout), 6 control steps; zero differing words per case and layout."""
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_golden_linesearch_crossed", os.path.join(ROOT, "tools", "gen_golden_linesearch_crossed.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    z = np.load(gen.GOLDEN)
    return {k: z[k] for k in z.files}


def test_the_fixture_is_whole(golden):
    info = json.loads(str(golden["build_info"]))
    assert info["flavor"] == "product" and len(info["src"]) == 64, info
    for c, l in gen.cases():
        st, ni = golden[f"{c}/{l}/state"], golden[f"{c}/{l}/niter"]
        assert st.shape == (gen.NROWS, gen.N) and st.dtype == np.float32 and ni.shape == (gen.STEPS, gen.N) and ni.dtype == np.int32
        assert np.isfinite(st).all(), (c, l)
    for l in gen.LAYOUTS:
        assert int(golden[f"crowded/{l}/crowded_steps"]) > 0, l
    assert os.path.getsize(gen.GOLDEN) < 300_000


@pytest.mark.parametrize("layout", gen.LAYOUTS)
@pytest.mark.parametrize("case", gen.CASES)
def test_bits_of_the_replicated_row_sums(golden, case, layout):
    state, niter, crowded = gen.rollout(case, layout)
    gs, gn, gc = golden[f"{case}/{layout}/state"], golden[f"{case}/{layout}/niter"], int(golden[f"{case}/{layout}/crowded_steps"])
    bad_n = int((niter != gn).sum())
    bad_w = int((state.view(np.uint32) != gs.view(np.uint32)).sum())
    print(f"\n[{case} {layout}] differing words of qpos / qvel / warm start: {bad_w} of {gs.size}; dbg_niter entries that differ: {bad_n} of {gn.size}; "
          f"env-steps with a foot on >= 3 box slots: {crowded} (recorded: {gc}) of {gen.STEPS * gen.N}")
    if case == "crowded":
        assert crowded > 0 and crowded == gc, (layout, crowded, gc)
    assert bad_n == 0, (case, layout, bad_n)
    assert bad_w == 0, (case, layout, bad_w)
