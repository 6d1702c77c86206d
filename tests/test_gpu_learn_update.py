"""learn.NativeLearner.update as a whole against the fp64 statement of the update in tests/ppo_reference.py, with the protocol and the bars of
tests/test_gpu_ppo_update.py (tests/learn_cases.py); the data-parallel path on a one-rank group; ppo.train(learner="native") end to end."""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import learn_cases as cases  # noqa: E402
import ppo_reference as ref  # noqa: E402


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in cases.ENV_KEYS + ("PGTT_PPO_FORCE_DP",):          # learn_cases.set_env writes os.environ: monkeypatch restores it afterwards
        monkeypatch.setenv(k, "x"); monkeypatch.delenv(k)


@pytest.mark.parametrize("mb,clip_active", [(5120, True), (1280, False)])
def test_native_update_matches_fp64_reference(mb, clip_active):
    """Loss (2e-5 relative), the clipped gradient of each of the 16 tensors and the Adam step of six updates against fp64.  The gradient bar is
    the one of test_gpu_ppo_update.py: the same errors are measured for the PyTorch-op trainer on the same GPU in this test, and the native
    learner must stay within 4x of it per tensor (worst of the six calls; relative L2 and max-norm).  The product path (_Learner) runs alongside
    for the three-row table of DESIGN.md 17."""
    from phase_guided_terrain_traversal_amd import ppo
    op, _ = cases.run_six(mb, clip_active, "op")
    pr, _ = cases.run_six(mb, clip_active, "product")
    na, learner = cases.run_six(mb, clip_active, "native")
    assert learner.graph is not None and len(learner.graph) == 1 and learner.calls == 6
    names = [n for n, _ in ppo.ActorCritic().named_parameters()]
    bad = []
    print(f"mb={mb} clip {'active' if clip_active else 'inactive'}: gradient error against fp64, worst of six calls (relative L2 | max-norm)")
    for i, name in enumerate(names):
        e = {k: [max(r[i][j] for r in rows) for j in (0, 1)] for k, rows in (("op", op), ("product", pr), ("native", na))}
        print(f"  {name:18s} op form {e['op'][0]:.2e} | {e['op'][1]:.2e}   product {e['product'][0]:.2e} | {e['product'][1]:.2e}   "
              f"native {e['native'][0]:.2e} | {e['native'][1]:.2e}   native / op {e['native'][0] / max(e['op'][0], 1e-300):.2f} | {e['native'][1] / max(e['op'][1], 1e-300):.2f}")
        if e["native"][0] > 4 * e["op"][0] or e["native"][1] > 4 * e["op"][1]:
            bad.append((name, e["op"], e["native"]))
    for k in range(6):
        print(f"  call {k + 1}: worst relative L2  op form {max(e[0] for e in op[k]):.2e}  product {max(e[0] for e in pr[k]):.2e}  native {max(e[0] for e in na[k]):.2e}")
    assert not bad, bad


DP_WORKER = r'''
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch, torch.distributed as dist
import learn_cases as cases, ppo_reference as ref
from phase_guided_terrain_traversal_amd import ppo
from phase_guided_terrain_traversal_amd.distributed import init_from_env
rank, local, world = init_from_env(sys.argv[2], force=True)
assert dist.is_initialized() and world == 1
mb, out = 1280, {}
for mode in ("0", "1"):
    os.environ["PGTT_PPO_FORCE_DP"] = mode
    assert ppo._dp() == (mode == "1")
    cases.set_env("native")
    model, norm_s, norm_p, B, cfg, learner, g = cases.setup(mb, True, "native")
    assert learner.dp == (mode == "1")
    perm = torch.randperm(4 * mb, device="cuda", generator=g)
    for k in range(5):
        learner.update(perm[(k % 4) * mb:(k % 4 + 1) * mb])
    torch.cuda.synchronize()
    assert learner.graph is not None and len(learner.graph) == (2 if mode == "1" else 1)
    out[mode] = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).double().cpu(), float(learner.loss)
a, b = out["0"][0], out["1"][0]
tol = 5 * (2.0 ** -23 * a.abs() + 1e-5 * 3e-4)
print(json.dumps({"worst": float(((a - b).abs() / tol).max()), "equal_bits": bool(torch.equal(a, b)), "finite": bool(torch.isfinite(b).all()),
                  "loss": [out["0"][1], out["1"][1]]}))
dist.destroy_process_group()
'''


def test_data_parallel_path_on_a_one_rank_group(tmp_path):
    """PGTT_PPO_FORCE_DP=1 on a one-rank RCCL group: two graphs round an all-reduce of the flat gradient (an identity here) and grad_scale = 1 / 1
    give the parameters of the single-process path after five updates, within the Adam bar 5 (2^-23 |p| + 1e-5 lr).  Measured: equal bits."""
    script = tmp_path / "dp_worker.py"
    script.write_text(DP_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29647", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(script), ROOT, "nccl"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(res)
    assert res["finite"] and res["worst"] <= 1.0, res


def test_train_native_end_to_end(tmp_path):
    """ppo.train(learner="native") on a 256-env flat Joystick, two iterations of 256 x 20 rows (four minibatches of 1280, four passes): everything
    finite, every parameter moved, and checkpoint -> export_policy_npz -> policy.PolicyMLP gives the live model's head on 8 observations to 1e-5"""
    from phase_guided_terrain_traversal_amd import configs, learn, policy, ppo
    from phase_guided_terrain_traversal_amd.env import Joystick
    n = 256
    env = Joystick("flat_terrain", configs.training_config(), num_envs=n, device="cuda:0", autoreset=True)
    cfg = ppo.PPOConfig(num_timesteps=2 * 20 * n, num_evals=3, batch_size=64, num_minibatches=4, seed=11, learner="native")
    torch.manual_seed(cfg.seed)
    initial = [p.detach().clone() for p in ppo.ActorCritic(env.observation_size["state"], env.observation_size["privileged_state"]).parameters()]
    ckpts = []
    model, (ns, npv), hist = ppo.train(env, cfg, policy_params_fn=lambda s, c: ckpts.append((s, c)))
    torch.cuda.synchronize()
    assert [s for s, _ in hist] == [20 * n, 40 * n] and len(ckpts) == 2
    params = list(model.parameters())
    lo = min(p.data_ptr() for p in params)
    assert sum(p.numel() for p in params) * 4 == max(p.data_ptr() + 4 * p.numel() for p in params) - lo        # still views of one flat buffer
    for p, p0 in zip(params, initial):
        assert bool(torch.isfinite(p).all()) and float((p.detach().cpu() - p0).abs().max()) > 0
    for _, m in hist:
        assert all(v == v and abs(v) != float("inf") for v in m.values()), m
    assert bool(torch.isfinite(ns.mean).all() and torch.isfinite(ns.std).all() and torch.isfinite(npv.mean).all())
    path = str(tmp_path / "policy.npz")
    ppo.export_policy_npz(ckpts[-1][1], path)
    net = policy.PolicyMLP(path).cuda()
    obs = env._obs()["state"][:8].clone()
    with torch.no_grad():
        live = model.policy(ns(obs))
    assert float((net.head(obs) - live).abs().max()) <= 1e-5
    print(f"native end to end: loss {hist[-1][1]['loss']:.4f}, {hist[-1][1]['env_steps_per_s_total'] / 1e6:.2f} M env-steps/s in total")
    env.close()
