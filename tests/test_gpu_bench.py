"""The driver's own command, `python bench.py --gpus 1 --steps 20 --warmup 5`, on the GPU: ONE JSON line with the contract's fields and the metric of
BASELINE.json on its configuration, nothing beyond the headline window, and the outputs of its last timed step with --dump-outputs.  With --full the same
line also carries `cpu_baseline` and the side rows this repository adds (other single-GPU configs, the roll-out row, one-HIP-graph row, the seven
curriculum levels of configs[4], the 1-ulp-division side build).  A guard for the measurement, not a benchmark: thresholds are far below the measured values."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


DRIVER = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
OUTPUTS = {"obs_state": (4096, None), "obs_privileged_state": (4096, None), "reward": (4096,), "done": (4096,), "info_metrics": (None, 4096),
           "info_episode_metrics": (None, 4096)}


def _bench(extra, timeout):
    """-> (JSON line, wall seconds of the whole process)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "PGTT_LIB")}
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + DRIVER + extra, env=env, capture_output=True, text=True, timeout=timeout)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), wall


def _load_outputs(d):
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert set(got) == set(OUTPUTS), sorted(got)
    for k, shape in OUTPUTS.items():
        a = got[k]
        assert a.dtype == np.float32 and a.ndim == len(shape) and all(s is None or s == t for s, t in zip(shape, a.shape)), (k, a.shape)
        assert np.isfinite(a).all(), k
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6
    return got


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plain") / "outputs")
    d, wall = _bench(["--dump-outputs", out], 600)
    return d, wall, out


def test_plain_run_is_lean_and_dumps_the_last_step(plain_run):
    """the plain command times the headline workload and nothing else: no cpu_baseline, no other_configs, at most 30 s of the process outside
    its warm-up and timed steps; --dump-outputs leaves what the last timed step returned to its caller"""
    d, wall, out = plain_run
    assert d["steps"] == 20 and d["warmup"] == 5 and "cpu_baseline" not in d and "other_configs" not in d and "error" not in d
    assert d["env_steps_allreduced"] == d["env_steps_expected"] == 4096 * 20
    assert abs(d["value"] - d["env_steps_allreduced"] / (d["ms_per_step"] * 1e-3 * 20)) < 1e-6 * d["value"]
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert wall - (20 + 5) * d["ms_per_step"] * 1e-3 < 30, wall
    got = _load_outputs(out)
    assert set(np.unique(got["done"])) <= {0.0, 1.0}


def test_driver_command_line_contract(plain_run, tmp_path):
    d, _ = _bench(["--full", "--cpu-sample-steps", "25", "--dump-outputs", str(tmp_path / "full")], 1500)
    # --full changes nothing about the headline window: the same inputs, the same outputs, bit for bit
    ref = _load_outputs(plain_run[2])
    for k, a in _load_outputs(str(tmp_path / "full")).items():
        assert np.array_equal(a, ref[k]), k
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "env-steps/s" and d["n_gpus"] == 1 and d["steps"] == 20
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert d["env_steps_allreduced"] == d["env_steps_expected"] == 4096 * 20 and "error" not in d and d["cold"] is False
    assert abs(d["value"] - d["env_steps_allreduced"] / (d["ms_per_step"] * 1e-3 * 20)) < 1e-6 * d["value"]
    assert d["value"] > 15e6                                     # target of the north star: 1 M; measured 22 - 23 M
    c = d["config"]
    assert "level4" in c["workload"] and c["envs_per_gpu"] == 4096 and c["prime_steps"] >= 100
    # top-level "warmup" echoes the command line (the driver compares the two); every untimed step before the clock (40 code-path priming steps +
    # prime_steps + those 5) is `untimed_steps`
    assert d["warmup"] == 5 and d["untimed_steps"] == c["untimed_steps_before_clock"] == 40 + c["prime_steps"] + 5
    assert "domain_randomize" in c["terrain_variants"] and "fp32_div_sqrt" not in c          # the product rounds `/` and sqrt correctly: no footnote
    assert len(d["ranks_dt"]) == 1 and 0 < d["ranks_dt"][0] <= d["ms_per_step"] * 1e-3 * 20 * 1.0001
    r = d["roofline"]
    assert r["kernel"] == "physics_kernel" and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0.1 < r["frac"] < 1.0
    # counters are quoted only when profiles/hbm_traffic.json was measured on the sources of the library being timed
    from phase_guided_terrain_traversal_amd import native
    measured_on = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json"))).get("_source", {}).get("csrc_sha256")
    info = native.build_info()
    assert info["flavor"] == "product" and info["src"] == native.source_sha256()            # the loaded library is the product build of this tree
    assert r["profile_stale"] is (measured_on != info["src"])
    if r["profile_stale"]:
        assert r["traffic"] is None and r["valu_busy"] is None and r["mfma_ops"] is None
    else:
        assert 3e6 < r["traffic"] < 2e7 and 0.3 < r["valu_busy"] < 1.0
    # round 6: the fraction against the UNPACKED fp32 ceiling (78.65 TFLOP/s) beside the stated one, and the static share of packed vector instructions
    assert abs(r["frac_unpacked_ceiling"] - r["achieved"] / 78.65) < 1e-9 and abs(r["frac_unpacked_ceiling"] - 2 * r["frac"]) < 1e-3
    isa = json.load(open(os.path.join(ROOT, "profiles", "isa_static.json")))
    assert (r["valu_packed_share"] == isa["valu_packed_share"]) if isa["csrc_sha256"] == info["src"] else (r["valu_packed_share"] is None)
    k = d["kernels_ms"]
    assert k["launches"] >= 3 and 0.05 < k["physics_kernel"] < 0.3 and 0.005 < k["observe_kernel"] < 0.05
    assert k["physics_kernel"] + k["observe_kernel"] < d["ms_per_step"] * 1.05          # the kernels fit inside the step they are part of
    b = d["cpu_baseline"]
    assert b["kind"] == "port" and b["cores"] >= 1 and b["value"] > 0 and abs(b["per_core"] - b["value"] / b["cores"]) < 1e-6 * b["value"] and "25 control steps" in b["sample"]
    rows = {(r_["workload"], r_["envs"], r_.get("fp32_div_sqrt"), r_.get("stage")): r_ for r_ in d["other_configs"]}
    assert rows[("flat", 4096, None, None)]["value"] > 20e6 and rows[("wfc_dr", 8192, None, None)]["value"] > 20e6 and rows[("level4", 32768, None, None)]["value"] > 20e6
    # BASELINE configs[4]: every level file of the curriculum has a driver-timed figure at the per-rank batch
    for stage, lvl in enumerate([1, 2, 3, 4, 7, 10, 13]):
        cr = rows[("curriculum", 4096, None, stage)]
        assert cr["level"] == f"level{lvl}" and cr["value"] > 10e6 and cr["steps"] >= 100
    gr = rows[("graph", 4096, None, None)]
    assert "skipped" not in gr and gr["env_steps_counted"] == gr["env_steps_expected"] and gr["steps_per_graph"] == 20
    assert gr["value"] > 0.9 * d["value"]                    # the same kernels without launch gaps / event records
    roll = rows[("rollout", 4096, None, None)]
    assert "skipped" not in roll and roll["value"] > 8e6 and roll["launches_per_step"] == 4              # measured 18 - 19 M
    fast = rows[("level4", 4096, "1ulp", None)]
    assert "skipped" not in fast and 0.9 * d["value"] < fast["value"] < 1.25 * d["value"]
