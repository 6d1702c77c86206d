"""The line search of physics_kernel carries its two bracket ends in lane pairs (QSolver::linesearch: role = lane & 1, `lo` in the even lane, `hi` in the
odd one, traded by quad_perm [1,0,3,2]).  It is the arithmetic of the replicated form on the same operands, so
 - every build reproduces, bit for bit, what the commit before the split computed (tests/golden/linesearch_roles_parent.npz, recorded by
   tools/gen_golden_linesearch.py on that commit): level4 and flat, hex / oct / quad, N = 61 (ragged last wave in every layout), the product's caps,
   ls_iterations = 1 and iterations = 1.  ls_iterations = 0 cannot be recorded: pgtt_create takes 1 .. 64 (asserted below), so the search that ends
   without a round - its ends handed back from the roles they never left - is met where every env of a wave starts within tolerance;
 - an env's bits do not depend on who shares its wave: eight different envs in one launch against each env run as four copies of itself - a wrong exchange
   partner (a lane of another env) shows here first."""
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from phase_guided_terrain_traversal_amd import configs
from phase_guided_terrain_traversal_amd.env import Joystick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_golden_linesearch", os.path.join(ROOT, "tools", "gen_golden_linesearch.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    z = np.load(gen.GOLDEN)
    return {k: z[k] for k in z.files}


def test_the_fixture_is_whole(golden):
    info = json.loads(str(golden["build_info"]))
    assert info["flavor"] == "product" and len(info["src"]) == 64, info
    for w, l, s in gen.cases():
        st, ni = golden[f"{w}/{l}/{s}/state"], golden[f"{w}/{l}/{s}/niter"]
        assert st.shape == (gen.NROWS, gen.N) and st.dtype == np.float32 and ni.shape == (gen.STEPS, gen.N) and ni.dtype == np.int32
        assert np.isfinite(st).all(), (w, l, s)
    # the settings do what they are there for: the caps bind
    cap = lambda s: max(int((golden[f"{w}/{l}/{s}/niter"] & 0xFFFF).max()) for w in gen.WORKLOADS for l in gen.LAYOUTS)
    assert cap("it1") == 1 and cap("caps") > 1
    assert os.path.getsize(gen.GOLDEN) < 600_000


@pytest.mark.parametrize("layout", gen.LAYOUTS)
@pytest.mark.parametrize("workload", gen.WORKLOADS)
def test_bits_of_the_replicated_line_search(golden, workload, layout):
    for setting in gen.SETTINGS:
        state, niter = gen.rollout(workload, layout, setting)
        gs, gn = golden[f"{workload}/{layout}/{setting}/state"], golden[f"{workload}/{layout}/{setting}/niter"]
        bad_n = int((niter != gn).sum())
        bad_s = int((state.view(np.uint32) != gs.view(np.uint32)).any(0).sum())
        print(f"\n[{workload} {layout} {setting}] envs whose qpos / qvel / warm start differ: {bad_s} of {gen.N}; dbg_niter entries that differ: {bad_n} of {gn.size}")
        assert bad_n == 0, (workload, layout, setting, bad_n)
        assert bad_s == 0, (workload, layout, setting, bad_s)


def test_a_line_search_without_rounds_is_refused():
    from phase_guided_terrain_traversal_amd import mjcf, native
    with pytest.raises(native.PgttError, match="iteration counts out of range"):
        Joystick("flat_terrain", configs.training_config(), num_envs=4, device="cuda:0", model=dict(mjcf.load_model("flat_terrain"), ls_iterations=0))


@pytest.mark.parametrize("layout", ["hex", "quad"])
def test_an_env_among_strangers_and_among_copies_of_itself(layout):
    terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
    n, copies, steps = 8, 4, 12
    variant = np.random.default_rng(2).integers(0, terrain.shape[0], n).astype(np.int32)
    rep = np.repeat(np.arange(n), copies)            # e, e, e, e: a hex wave is four copies of one env, a quad wave four envs four times
    ri = torch.from_numpy(rep).cuda()
    for task, ter in (("stairs", terrain), ("flat_terrain", None)):
        mk = lambda idx: Joystick(task, configs.training_config(), num_envs=len(idx), terrain=ter, device="cuda:0", layout=layout,
                                  **({"variant": torch.from_numpy(variant[idx])} if ter is not None else {}))
        A, B = mk(np.arange(n)), mk(rep)
        A.reset(3)
        rng = np.random.default_rng(0)
        diff = 0
        for k in range(steps):
            a = torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda()
            for key in ("state", "istate"):
                B.buffers[key].copy_(A.buffers[key][..., ri])
            B.buffers["scan_z"].copy_(A.buffers["scan_z"][ri])
            A.step(a); B.step(a[ri].contiguous())
            torch.cuda.synchronize()
            diff += int((A.buffers["state"][:55, ri].view(torch.int32) != B.buffers["state"][:55].view(torch.int32)).any(0).sum())
        print(f"\n[{task} {layout}] {diff} of {steps * len(rep)} env-steps differ between an env among seven others and among copies of itself")
        assert torch.isfinite(B.buffers["state"][:55]).all()
        assert diff == 0, (task, layout, diff)
        A.close(); B.close()
