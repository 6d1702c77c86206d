"""Records tests/golden/linesearch_crossed_parent.npz: what physics_kernel computed BEFORE the bracketing rounds' row sums took their first butterfly step
crossed (QSolver::ls_points' paired form, pair_sum2) - tests/test_gpu_linesearch_crossed.py holds every later build to these bits.
   usage (on a GPU, with the library of the commit before the change - a checkout of it, or PGTT_LIB=<its libpgtt.so>):
       python tools/gen_golden_linesearch_crossed.py [out.npz]
It records what tests/golden/linesearch_roles_parent.npz (tools/gen_golden_linesearch.py) does not reach - the code the crossed sums share with the rare
row pair, the DR kernels, and a round loop that leaves by its cap after the second round:
  crowded   three or four slabs with the same top face overlap over the whole spawn area (the overlap terrain of tests/test_gpu_parity.py, a fourth slab
            in two of the four variants): a standing foot holds three or four box contacts, so hex runs the (slot 2, slot 3) row pair, quad the
            `k >= 2` slot loop and oct `units() > 2`.  The record counts, from the debug contact record, the env-steps in which some foot holds >= 3 box
            slots (`crowded/<layout>/crowded_steps`); a recording without any is refused, and the test asserts the same count on its build;
  dr        level13 with full domain randomisation (params, box friction, variants): the HAS_DR kernels, oct's per-lane-cap kernels among them;
  ls2       level4 with ls_iterations = 2.
All: hex / oct / quad, N = 13 envs (a ragged last wave in every layout), 6 control steps from reset(seed=0) under tanh(N(0, 0.6)) actions of a fixed seed.
Kept per case: state[:55] (qpos, qvel, warm start) after the last step - every earlier step's bits are in it - and dbg_niter after every step.
The file says what recorded it (`build_info`: native.build_info() of the loaded library).  rollout() is what the test runs, too."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "linesearch_crossed_parent.npz")
N, STEPS = 13, 6
CASES = ("crowded", "dr", "ls2")
LAYOUTS = ("hex", "oct", "quad")
NROWS = 55          # state rows of qpos (19), qvel (18) and the solver's warm start (18)
TERRAINS = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains")


def crowded_terrain():
    """[4 variants][100 boxes][10]: slabs 3 x 3 m, tops at 4 cm, centres apart so that the broad-phase order is well defined; the rest parked far away"""
    T = []
    for v in range(4):
        rows = [[0.3 + 0.1 * v, 0.2, 0.02, 1, 0, 0, 0, 3.0, 3.0, 0.02],
                [-0.4, -0.3 + 0.1 * v, 0.02, 1, 0, 0, 0, 3.0, 3.0, 0.02],
                [0.1 * v, 0.5, 0.02, 0, 0, 0, 1, 3.0, 3.0, 0.02]]
        if v >= 2:
            rows.append([-0.2, 0.1 * v - 0.6, 0.02, 1, 0, 0, 0, 3.0, 3.0, 0.02])
        rows += [[100.0 + k, 100.0 + k, 100.0 + k, 1, 0, 0, 0, 0.5, 0.5, 0.5] for k in range(100 - len(rows))]
        T.append(rows)
    return np.asarray(T, dtype=np.float32)


def crowded_feet(dbg_contact):
    """envs in which some foot holds three or four box slots, from the debug contact record [N][8][2] (foot; geom: -1 plane, box index, -2 none)"""
    con = dbg_contact.reshape(-1, 8, 2)[:, 4:]
    per_foot = np.stack([((con[..., 0] == f) & (con[..., 1] >= 0)).sum(1) for f in range(4)], 1)
    return int((per_foot.max(1) >= 3).sum())


def rollout(case, layout):
    """-> (state[:55] after the last step [55, N] float32, dbg_niter after every step [STEPS, N] int32, env-steps with a foot on >= 3 box slots)"""
    import torch
    from phase_guided_terrain_traversal_amd import configs, mjcf
    from phase_guided_terrain_traversal_amd.env import Joystick
    from phase_guided_terrain_traversal_amd.randomize import domain_randomize
    model = mjcf.load_model("stairs")
    if case == "crowded":
        terrain = crowded_terrain()
        kw = {"variant": torch.from_numpy(np.random.default_rng(0).integers(0, terrain.shape[0], N).astype(np.int32))}
    elif case == "dr":
        terrain = np.load(os.path.join(TERRAINS, "level13.npy"))
        dr = domain_randomize(model, N, seed=3, terrain=terrain)
        kw = {"variant": torch.from_numpy(dr["variant"]), "params": torch.from_numpy(dr["params"]), "box_friction": torch.from_numpy(dr["box_friction"])}
    else:
        terrain = np.load(os.path.join(TERRAINS, "level4.npy"))
        kw = {"variant": torch.from_numpy(np.random.default_rng(0).integers(0, terrain.shape[0], N).astype(np.int32))}
        model = dict(model, ls_iterations=2)
    env = Joystick("stairs", configs.training_config(), num_envs=N, terrain=terrain, device="cuda:0", layout=layout, debug_contacts=True, model=model, **kw)
    env.reset(seed=0)
    rng = np.random.default_rng(11)
    niter = np.zeros((STEPS, N), np.int32)
    crowded = 0
    for k in range(STEPS):
        env.step(torch.from_numpy(np.tanh(rng.normal(size=(N, 12)) * 0.6).astype(np.float32)).cuda())
        torch.cuda.synchronize()
        niter[k] = env.buffers["dbg_niter"].cpu().numpy()
        crowded += crowded_feet(env.buffers["dbg_contact"].cpu().numpy())
    state = env.buffers["state"][:NROWS].cpu().numpy().copy()
    env.close()
    return state, niter, crowded


def cases():
    return [(c, l) for c in CASES for l in LAYOUTS]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from phase_guided_terrain_traversal_amd import native
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    res = {"build_info": np.array(json.dumps(native.build_info())), "library": np.array(os.path.basename(native.LIB_PATH))}
    for c, l in cases():
        st, ni, cr = rollout(c, l)
        res[f"{c}/{l}/state"], res[f"{c}/{l}/niter"], res[f"{c}/{l}/crowded_steps"] = st, ni, np.array(cr, np.int32)
        print(f"{c:8s} {l:4s} finite {bool(np.isfinite(st).all())}  env-steps with a foot on >= 3 box slots {cr} of {STEPS * N}  "
              f"niter (low 16 bits) histogram {np.bincount(ni.ravel() & 0xFFFF).tolist()}")
        if c == "crowded" and cr == 0:
            sys.exit(f"refused: no env-step of the crowded case ({l}) has a foot on three or four box slots - the record would not reach the rare row pair")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes;", res["build_info"])
