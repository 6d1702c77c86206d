"""GPU parity: libpgtt.so (HIP, through the C ABI) vs the CPU oracle on identical seeded inputs.

Bar (BASELINE.json north_star): float32 state within 1e-4 after one control step (4 physics substeps)
from an identical state, contact flags and the ACTIVE (foot, geom) contact set bit-exact.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle
from phase_guided_terrain_traversal_amd import abi, configs, mjcf

import parity_explain as X

ASSETS = os.path.join(os.path.dirname(mjcf.__file__), "assets")


# execution options of the envs this module builds (PgttConfig.lane_layout / observe_form), set by the fixtures below
EXEC = {"layout": None, "observe_form": None}


def make_pair(task, n, terrain=None, noise=1.0, autoreset=False, dr=False, method="pgtt", ctrl_dt=None, product_variants=False, cfg_over=None, no_variant_buffer=False,
              model=None):
    from phase_guided_terrain_traversal_amd.env import Joystick
    cfg = configs.with_overrides(configs.training_config(method), **{"noise_config.level": noise}, **(cfg_over or {}))
    if ctrl_dt is not None:
        cfg["ctrl_dt"] = ctrl_dt          # ctrl_dt = sim_dt: one control step = ONE mjx.step (per-substep parity)
    model = mjcf.load_model(task) if model is None else model
    kw = {"model": model}
    variant = params = bf = None
    if terrain is not None and not no_variant_buffer:
        variant = np.random.default_rng(2).integers(0, terrain.shape[0], n).astype(np.int32)
    from phase_guided_terrain_traversal_amd.randomize import domain_randomize
    if terrain is not None and product_variants and not dr:      # the labelling train.py / evaluate.py / bench.py get (grouped per 4096 global ids), DR off
        variant = domain_randomize(model, n, seed=2, terrain=terrain, enable=False)["variant"]
    if dr:
        out = domain_randomize(model, n, seed=11, terrain=terrain)
        params, bf = out["params"], out.get("box_friction")
        kw["params"] = torch.from_numpy(params)
        if bf is not None:
            kw["box_friction"] = torch.from_numpy(bf)
        if terrain is not None:
            variant = out["variant"]
    if variant is not None:
        kw["variant"] = torch.from_numpy(variant)
    env = Joystick(task, cfg, num_envs=n, terrain=terrain, device="cuda:0", autoreset=autoreset, debug_contacts=True, **EXEC, **kw)
    cfg2 = dict(cfg); cfg2["autoreset"] = int(autoreset)
    cs, ms = abi.config_struct(cfg2), abi.model_struct(model)
    hb = oracle.HostBuffers(n, with_params=dr, with_variant=variant is not None, with_box_friction=bf is not None, method=method)
    if variant is not None:
        hb["variant"][:] = variant
    if dr:
        hb["params"][:] = params
        if bf is not None:
            hb["box_friction"][:] = bf
    return env, hb, cs, ms


def motor_targets(env, act):
    """the 12 motor-target rows of a control step, in the float32 arithmetic of both sides (go2/joystick_pgtt.py:143): default pose + action x scale.
    (After an AutoReset the state rows hold the first state's zeros instead.)"""
    key = np.asarray(env.model["key_qpos"], np.float32)[7:]
    return (key[:, None] + act.T.astype(np.float32) * np.float32(env.config["action_scale"])).astype(np.float32)


def sync_to_host(env, *hbs):
    for hb in hbs:
        for k in ("state", "istate", "scan_z", "done", "first_state", "first_obs", "ep_metrics"):
            hb[k][...] = env.buffers[k].cpu().numpy()


def active_sets(con, dist):
    con = con.reshape(-1, 8, 2)
    return [sorted((int(f), int(b)) for (f, b), d in zip(con[e], dist[e]) if d < 0 and b != -2) for e in range(con.shape[0])]


def per_env_errors(g, hb):
    """max-abs error per env for every compared quantity (g: dict of numpy arrays from the GPU)."""
    S, H = g["state"], hb["state"]
    rel = lambda a, b, ax: (np.abs(a - b) / (1 + np.abs(b))).max(axis=ax)
    return dict(qpos=np.abs(S[:19] - H[:19]).max(0), qvel=np.abs(S[19:37] - H[19:37]).max(0),
                warm=rel(S[37:55], H[37:55], 0),
                info=np.abs(np.delete(S[55:], np.s_[abi.S_QERR_HIST - 55:abi.S_QVEL_HIST + 24 - 55], 0)
                            - np.delete(H[55:], np.s_[abi.S_QERR_HIST - 55:abi.S_QVEL_HIST + 24 - 55], 0)).max(0),
                hist=np.abs(S[abi.S_QERR_HIST:abi.S_QVEL_HIST + 24] - H[abi.S_QERR_HIST:abi.S_QVEL_HIST + 24]).max(0),
                frame=rel(g["frame"], hb["frame"], 0),
                scan=np.abs(g["scan_z"] - hb["scan_z"]).max(1), obs=rel(g["obs_state"], hb["obs_state"], 1),
                priv=rel(g["obs_priv"], hb["obs_priv"], 1), reward=np.abs(g["reward"] - hb["reward"]),
                metrics=rel(g["metrics"], hb["metrics"], 0))


# Measured on MI355X (tools/gpu_parity_stats.py, 30 k env-steps per workload and lane layout):
#   W = env-steps whose every Newton solve reaches its minimiser in the fp64 oracle (scaled gradient < 1e-6 at the exit: the
#       5-iteration cut of go2_mjx_feetonly.xml:17 did not bite) AND whose fp32 oracle result agrees with the fp64 one
#       (qpos 1e-5, qvel 1e-3): the env-steps on which the reference's answer does not depend on rounding.
#   control step (4 x mjx.step):  W = 77-79 % of env-steps; HIP vs oracle on W: qpos > 1e-4 on 0.08-0.17 %, qvel > 5e-3 on 0.10-0.22 %,
#       qacc_warmstart > 1e-2 (relative) on 0.2-0.4 %, contact flags differ on <= 0.01 %
#   one mjx.step (ctrl_dt = sim_dt): W = 86-87 %; qpos > 1e-4 on 0.05 %, qvel > 2e-2 on 0.05 %
# The residue are solves that converge exactly AT the cap in the oracle (gradient 0.6 -> 4e-7 in the fifth iteration) and one
# line-search round later on the GPU; the bars below are the measured rates x 2 (binomial noise of a 10-15 k sample).
W_FLOOR = {4: 0.72, 1: 0.81}                 # measured - 5 points
VIOL_CAP = {4: dict(qpos=0.003, qvel=0.004, warm=0.008, info=0.003, hist=0.006, scan=0.002, obs=0.004, priv=0.005, frame=0.005, reward=0.003, metrics=0.006),
            1: dict(qpos=0.0015, qvel=0.0015, warm=0.004, info=0.0015, hist=0.004, scan=0.002, obs=0.003, priv=0.004, frame=0.004, reward=0.0015, metrics=0.004)}
# Round 3 (profiles/archive/r03_parity_p90.txt): percentiles of the GPU-vs-oracle error next to the oracle's own fp32-vs-fp64 error.
#   on W:        GPU p90 / oracle p90 = 1.26-1.47 (qpos 3 ulp vs 2 ulp of a unit coordinate), p99 1.2-1.45; observation / sensor-frame rows (relative):
#                p99.9 = 1.8e-3 .. 4.4e-3  ->  tolerances below = 2 x that (they were 2e-2);
#   all steps:   p90 ratio 1.8-2.0 - with the correctly rounded division / sqrt build (make PRECISE_DIV=1) just the same (1.8-2.2), and the ORACLE's two fp32
#                builds against each other (portable vs -O3 -march=native, tools/cpu_fp32_pair_stats.py, no GPU involved) 1.7-2.1: on the env-steps whose
#                solve is cut short two fp32 evaluations differ from each other by more than either differs from fp64.  Bounded at 2.6.
P90_W_RATIO, P90_ALL_RATIO = 1.75, 2.6
P90_FLOOR = dict(qpos=1.2e-7, qvel=5e-6, obs=2e-6, frame=3e-6)        # one rounding of the quantity's typical size


def run_parity(task, n, terrain, steps, dr=False, autoreset=False, noise=1.0, method="pgtt", ctrl_dt=None, w_floor=None, cap_scale=1.0, med_tol=2e-6,
               product_variants=False, cfg_over=None, no_variant_buffer=False, model=None):
    """One control step (4 x mjx.step; ONE mjx.step with ctrl_dt = sim_dt) from an IDENTICAL state, repeated `steps` times along
    a GPU rollout (the oracle is re-synchronised from the GPU state before every step).

    The reference truncates Newton at 5 iterations with a 5-round line search (go2_mjx_feetonly.xml:17).  A solve that is CUT
    before it reaches the minimiser returns a point that depends on the rounding of every intermediate: the fp32 and fp64
    builds of the ORACLE ITSELF then disagree by up to 0.1 on qpos.  A solve that reaches the minimiser is unique.  So:
      * on W (see above; the set is defined by the two ORACLE builds alone, the GPU has no say in it): north-star bar -
        qpos within 1e-4, qvel within 1e-4 / ctrl_dt, qacc_warmstart, observations, rewards, contact flags and the ACTIVE
        (foot, geom) set bit-exact - with the violation caps above;
      * on all env-steps: integers bit-exact, everything finite, errors bounded, and the GPU-vs-oracle error distribution
        no worse than the oracle's own fp32-vs-fp64 distribution.
    """
    nsub = 4 if ctrl_dt is None else int(round(ctrl_dt / 0.005))
    env, hb, cs, ms = make_pair(task, n, terrain, noise=noise, dr=dr, autoreset=autoreset, method=method, ctrl_dt=ctrl_dt, product_variants=product_variants,
                                cfg_over=cfg_over, no_variant_buffer=no_variant_buffer, model=model)
    h64 = oracle.HostBuffers(n, with_params=dr, with_variant="variant" in hb.arrays, with_box_friction="box_friction" in hb.arrays, method=method)
    for k in ("params", "variant", "box_friction"):
        if k in hb.arrays:
            h64[k][...] = hb[k]
    seed = 3
    env.reset(seed)
    oracle.reset(cs, ms, terrain, hb, seed=seed, nthreads=8)
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in env.buffers.items()}
    assert np.abs(g["state"][:37] - hb["state"][:37]).max() < 1e-5
    conv0 = ((g["dbg_niter"] & 0xFFFF) < 5) & (hb["dbg_niter"] < 5)
    assert conv0.mean() > 0.5
    # per-env maxima; at the full-size batches a handful of the reset's solves converge AT the cap on one side only (same residue as in the
    # step loop below): at most 0.1 % of the envs may miss a bar that every env of the small cases meets
    # Round 5 (correctly rounded division / sqrt in the product): 1 env of 128 on level13 + DR sits at 3.1e-2 on its warm start with 2 Newton iterations
    # on both sides and identical contacts (|qacc| ~ 270 in that reset, tools/gpu_reset_warm_diag.py): the tail of a rounding error, so ONE env may miss the
    # bar in a small batch as 0.1 % may in a big one - but none by more than 5 x
    # Round 6: no blanket allowance.  An env that misses one of these bars goes through the judge of the step loop - both sides of the reset's
    # forward pass against the minimiser of its problem: a side off it must have stopped at the cap or on the fp32 resolution of its cost (every case met so
    # far: the latter, on both sides; round 5's case, |qacc| ~ 270 with 2 iterations and equal contacts, is one) - or must be one whose two forward passes move
    # by at least half as much in the fp32 oracle itself under <= 2 roundings of the pose (parity_explain.reset_ensemble).
    # Second line: never more than max(1, 0.3 %) of the envs (measured 3 of 2048 on level13 + DR), none by more than 5 x.
    key_z = float(np.asarray(env.model["key_qpos"])[2])
    reset_spread = {}
    ms_long = X.model_copy(ms, iterations=X.LONG_ITER, ls_iterations=X.LONG_LS)

    def reset_explained(e, observed, scale=1.0):
        """the reset's second forward pass of env e, both sides against the minimiser of its problem (same judge as a substep of the step loop: a side off
        the minimiser must have stopped at the cap or on the fp32 resolution of its cost); failing that, the oracle's own qacc spread under <= 2 roundings"""
        if e not in reset_spread:
            ed = X.env_data(hb, terrain, e)
            inp = (hb["state"][:19, e].astype(np.float64), hb["state"][19:37, e].astype(np.float64), np.zeros(18))
            ctrl = np.asarray(hb["state"][7:19, e], np.float64)
            why = []
            for side, src in (("device", g), ("fp32 oracle", hb)):
                sub = dict(qacc=src["state"][37:55, e], niter=int(src["dbg_niter"][e]) & 0xFFFF, con=src["dbg_contact"][e], dist=src["dbg_dist"][e])
                why += [a for a in X.judge_substep(ms, ms_long, ed, inp, ctrl, sub, side)]
            reset_spread[e] = (why, X.reset_ensemble(ms, ed, hb["state"][:19, e], hb["state"][19:37, e], key_z, seed=e))
        why, spread = reset_spread[e]
        return (why and all(a["cause"] != "unexplained" for a in why)) or spread * scale >= 0.5 * observed
    ci = np.nonzero(conv0)[0]
    # second line: measured 3 of 2048 envs over the warm-start bar on level13 + DR (tools/gpu_explain_big.py), none by more than 1.5 x
    few = lambda per_env, tol: (per_env > tol).sum() <= max(1, 3e-3 * n) and not (per_env > 5 * tol).any()
    warm0 = (np.abs(g["state"][37:55] - hb["state"][37:55]) / (1 + np.abs(hb["state"][37:55])))[:, conv0].max(0)
    assert few(warm0, 2e-2), (int((warm0 > 2e-2).sum()), float(warm0.max()), n)
    for j in np.nonzero(warm0 > 2e-2)[0]:
        assert reset_explained(int(ci[j]), warm0[j]), (int(ci[j]), float(warm0[j]), reset_spread[int(ci[j])])
    assert np.abs(g["state"][55:] - hb["state"][55:]).max() < 1e-5
    # the privileged observation holds the accelerometer and actuator forces of the reset's forward pass: compared where that solve converged on
    # both sides (same reason as in the step loop below); an accelerometer row moves by about (1 + |qacc|) x the relative change of qacc
    qs = 1.0 + np.abs(hb["state"][37:55]).max(0)
    priverr = np.abs(g["obs_priv"] - hb["obs_priv"])[conv0].max(1)
    assert few(priverr, 5e-3), (int((priverr > 5e-3).sum()), float(priverr.max()), n)
    for j in np.nonzero(priverr > 5e-3)[0]:
        assert reset_explained(int(ci[j]), priverr[j], qs[ci[j]]), (int(ci[j]), float(priverr[j]), reset_spread[int(ci[j])], float(qs[ci[j]]))
    assert np.abs(g["obs_state"] - hb["obs_state"]).max() < 5e-3
    assert np.array_equal(g["istate"], hb["istate"])
    assert np.array_equal(g["frame"][abi.F_CONTACT:abi.F_CONTACT + 4], hb["frame"][abi.F_CONTACT:abi.F_CONTACT + 4])
    foerr = np.abs(g["first_obs"] - hb["first_obs"])[conv0].max(1)            # [N][171 + 215]: the same two rows once more
    assert few(foerr, 5e-3) and set(ci[foerr > 5e-3]) <= set(ci[priverr > 5e-3])
    if reset_spread:
        print("reset: envs over a bar, their causes and the fp32 oracle's own qacc spread under <= 2 roundings of the pose:",
              {e: ([a["cause"] + " (" + a["side"] + ")" for a in w], f"{v:.3g}") for e, (w, v) in reset_spread.items()})
    rng = np.random.default_rng(1)
    EG, EF, flag_mismatch, set_mismatch, nactive, nbox_active = [], [], 0, 0, 0, 0
    nviol = {}
    well_total, well_flag_mismatch, well_set_mismatch, well_done_mismatch = 0, 0, 0, 0
    dt_ctrl = 0.005 * nsub
    tols = (("qpos", 1e-4), ("qvel", 1e-4 / dt_ctrl), ("warm", 1e-2), ("info", 2e-4), ("hist", 2e-2), ("scan", 1e-5), ("obs", 6e-3), ("priv", 1e-2),
            ("frame", 1e-2), ("reward", 2e-4), ("metrics", 2e-3))
    WELL = []
    # round 6: every env-step of W that misses a bar is replayed substep by substep and must show its cause (parity_explain.py): the 5-iteration cut
    # (`cap`), a solve that stopped on the fp32 resolution of its cost (`floor`), a contact distance within rounding of 0 (`sign`) - or the test fails
    ledger = X.Ledger()
    layout_used = EXEC["layout"] or ("hex" if n <= 4096 else ("oct" if n <= 8192 else "quad"))
    substeps = X.DeviceSubsteps(task, env.config, env.model, terrain, layout_used, n, {kk: hb[kk] for kk in ("params", "variant", "box_friction") if kk in hb.arrays})
    ALLQ = {"qpos_1e4": 0, "qvel_1e4": 0, "qvel_5e3": 0}
    for k in range(steps):
        sync_to_host(env, hb, h64)
        S0 = hb["state"].copy()
        act = np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)
        env.step(torch.from_numpy(act).cuda())
        r64 = np.zeros(n)
        oracle.step(cs, ms, terrain, hb, act, seed=seed, nthreads=8)
        oracle.step(cs, ms, terrain, h64, act, seed=seed, nthreads=8, fp64=True, resid=r64)
        torch.cuda.synchronize()
        g = {kk: v.cpu().numpy() for kk, v in env.buffers.items()}
        eg = per_env_errors(g, hb)
        ef = per_env_errors(hb.arrays, h64)
        EG.append(eg); EF.append(ef)
        # W: every solve of the step reached its minimiser in fp64, and the oracle's fp32 build lands on the same point
        well = (r64 < 1e-6) & (ef["qpos"] < 1e-5) & (ef["qvel"] < 1e-3)
        well_total += int(well.sum()); WELL.append(well)
        # integers never depend on the solver path; nothing may blow up anywhere
        assert np.array_equal(g["istate"], hb["istate"]), k
        assert all(np.isfinite(g[kk]).all() for kk in ("state", "frame", "obs_state", "obs_priv", "reward", "metrics", "scan_z")), k
        assert eg["qpos"].max() < 0.5, (k, eg["qpos"].max())      # all env-steps: bounded (measured max 0.13); the scan is a step function of the pose
        fl_g, fl_h = g["frame"][abi.F_CONTACT:abi.F_CONTACT + 4], hb["frame"][abi.F_CONTACT:abi.F_CONTACT + 4]
        fm = (fl_g != fl_h).any(0)
        ga, ha = active_sets(g["dbg_contact"], g["dbg_dist"]), active_sets(hb["dbg_contact"], hb["dbg_dist"])
        sm = np.array([a != b for a, b in zip(ga, ha)])
        flag_mismatch += int(fm.sum()); set_mismatch += int(sm.sum())
        well_flag_mismatch += int((fm & well).sum()); well_set_mismatch += int((sm & well).sum())
        nactive += sum(len(a) for a in ha); nbox_active += sum(1 for a in ha for (_, b) in a if b >= 0)
        well_done_mismatch += int(((g["done"] != hb["done"]) & well).sum())
        vkeys = {}
        for key, tol in tols:
            bad = well & (eg[key] > tol)
            nviol[key] = nviol.get(key, 0) + int(bad.sum())
            for e in np.nonzero(bad)[0]:
                vkeys.setdefault(int(e), []).append(key)
        for key, bad in (("flags", fm & well), ("sets", sm & well), ("done", (g["done"] != hb["done"]) & well)):
            for e in np.nonzero(bad)[0]:
                vkeys.setdefault(int(e), []).append(key)
        ALLQ["qpos_1e4"] += int((eg["qpos"] < 1e-4).sum()); ALLQ["qvel_1e4"] += int((eg["qvel"] < 1e-4).sum()); ALLQ["qvel_5e3"] += int((eg["qvel"] < 1e-4 / dt_ctrl).sum())
        if vkeys:
            ve = np.array(sorted(vkeys), dtype=np.int64)
            # an env the AutoReset wrapper has just put back on its first state no longer shows the physics output the replay ends with
            was_reset = (g["done"] != 0) | (hb["done"] != 0) if autoreset else np.zeros(n, bool)
            fin = g["state"][:55].copy()
            nrec = len(ledger.records)
            X.explain_step(ledger, k, ve, vkeys, ms, hb, terrain, S0, act, hb["state"][abi.S_MOTOR_TARGETS:abi.S_MOTOR_TARGETS + 12] if not autoreset else motor_targets(env, act),
                           fin, substeps, nsub, skip_final_check=was_reset, observed=eg, scan_ctx=dict(cs=cs, dev_scan=g["scan_z"], orc_scan=hb["scan_z"]))
            bad_now = [r for r in ledger.records[nrec:] if r["cause"] == "unexplained"]
            if bad_now:           # keep the whole batch of that step: tools/gpu_explain_case.py replays it (other layouts, other builds) on the GPU box
                out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "unexplained")
                os.makedirs(out, exist_ok=True)
                name = os.environ.get("PYTEST_CURRENT_TEST", "case").split("::")[-1].split(" ")[0].replace("[", "_").replace("]", "").replace("/", "_")
                np.savez_compressed(os.path.join(out, f"{name}_step{k}.npz"), S0=S0, act=act, fin=fin, envs=np.array([r["env"] for r in bad_now]), layout=layout_used, task=task, n=n, nsub=nsub,
                                    dr=dr, method=method, oracle_state=hb["state"], model_pickle=np.frombuffer(__import__("pickle").dumps(env.model), np.uint8),
                                    cfg_pickle=np.frombuffer(__import__("pickle").dumps(dict(env.config)), np.uint8), **{kk: hb[kk] for kk in ("params", "variant", "box_friction") if kk in hb.arrays},
                                    **({"terrain": terrain} if terrain is not None else {}))
    cat = lambda L, key: np.concatenate([d[key] for d in L])
    egq, efq = cat(EG, "qpos"), cat(EF, "qpos")
    stats = dict(frac_gpu_1e4=float((egq < 1e-4).mean()), frac_fp_1e4=float((efq < 1e-4).mean()),
                 med_gpu=float(np.median(egq)), p99_gpu=float(np.percentile(egq, 99)), p99_fp=float(np.percentile(efq, 99)),
                 max_gpu=float(egq.max()), max_fp=float(efq.max()), well_frac=well_total / (steps * n),
                 flag_mismatch=flag_mismatch, set_mismatch=set_mismatch, well_flag_mismatch=well_flag_mismatch,
                 well_set_mismatch=well_set_mismatch, active_contacts=nactive, box_contacts=nbox_active)
    print(f"\n[{task} n={n} steps={steps} substeps={nsub} dr={dr} autoreset={autoreset}]", {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in stats.items()})
    stats["well_violations"] = dict(nviol)
    stats["all_env_steps"] = {kk: v / (steps * n) for kk, v in ALLQ.items()}
    stats["explained"] = ledger.summary()
    print("env-steps in W:", well_total, "of", steps * n, " violations of the bar:", nviol)
    print("ALL env-steps (W or not): qpos < 1e-4 on {qpos_1e4:.2%}, qvel < 1e-4 on {qvel_1e4:.2%}, qvel < 1e-4 / ctrl_dt on {qvel_5e3:.2%}".format(**stats["all_env_steps"]))
    print("post-mortem of the", len(ledger.records), "env-steps of W that miss a bar:", stats["explained"])
    print("   how each `cap` was proven:", stats["explained"]["cap_proof"], f"({substeps.launches} launches of the lifted handle)")
    for r in ledger.unexplained()[:10]:
        print("   UNEXPLAINED step", r["step"], "env", r["env"], r["keys"], "-", r["detail"])
    assert not ledger.unexplained(), (len(ledger.unexplained()), ledger.unexplained()[0]["detail"])
    caps = VIOL_CAP[1 if nsub == 1 else 4]                  # other substep counts (2, 8: test_other_substep_counts_parity) are held to the control step's rates, scaled by the caller
    assert stats["well_frac"] > (W_FLOOR[1 if nsub == 1 else 4] if w_floor is None else w_floor), stats["well_frac"]
    for key, cnt in nviol.items():
        lim = cap_scale * caps[key] * well_total              # the caps are 2 x the measured rates; + 2 sigma of a binomial for the small samples
        assert cnt <= max(2, lim + 2.0 * np.sqrt(lim)), (key, cnt, well_total)
    assert well_done_mismatch <= 1
    # bit-exact contact indices on W: a foot whose distance changes sign within rounding of 0 may differ - measured 0-2 env-steps in 24 k per workload and
    # layout (tools/gpu_parity_stats.py, profiles/r05_parity_stats.txt: 5 in 142 k over six workloads = 3.5e-5).  The caps are RATES, 1e-4 / 2e-4 of W
    # (2e-4 / 5e-4 in round 4, 5e-4 / 1.5e-3 until round 3); a count is held to the 99.9 % quantile of a Poisson variable with that mean.  Until round 4
    # it was held to max(1, mean), which a 2 300-env-step test misses once in 60 runs at the measured rate: round 5's change of rounding moved two of
    # ~40 such tests over it.  (W = 2 300: 3 / 3; W = 25 000: 8 / 13.)
    from scipy.stats import poisson
    flag_cap, set_cap = int(poisson.ppf(0.999, 0.0001 * cap_scale * well_total)), int(poisson.ppf(0.999, 0.0002 * cap_scale * well_total))
    assert well_flag_mismatch <= flag_cap and well_set_mismatch <= set_cap, (well_flag_mismatch, well_set_mismatch, well_total, flag_cap, set_cap)
    assert stats["med_gpu"] < med_tol
    # all env-steps: no worse than the oracle's own fp32 noise floor (a distribution statement: needs a sample, 3 sigma of a binomial)
    pf = stats["frac_fp_1e4"]
    slack = 0.03 + 3.0 * np.sqrt(max(pf * (1.0 - pf), 0.06 * 0.94) / (steps * n))
    assert stats["frac_gpu_1e4"] >= stats["frac_fp_1e4"] - slack
    if steps * n >= 2000:
        assert stats["p99_gpu"] <= 2.5 * stats["p99_fp"] + 1e-4
        # 90th percentile on W within 1.75 x the oracle's own fp32 noise (measured 1.26-1.47).  Outside W (solves cut short) the MEDIAN error within
        # 2.6 x the oracle's fp32-vs-fp64 median (two fp32 evaluations against each other, see the table above) - the p90 over all env-steps of that
        # table lies inside this population for a control step (W = 78 %), but ON its edge for a single mjx.step (W = 86 %), hence the median here
        Wm = np.concatenate(WELL)
        for key in ("qpos", "qvel", "obs", "frame"):
            gq, fq = cat(EG, key), cat(EF, key)
            pw_g, pw_f = np.percentile(gq[Wm], 90), np.percentile(fq[Wm], 90)
            stats[f"p90_{key}"] = (float(pw_g), float(pw_f))
            assert pw_g <= P90_W_RATIO * pw_f + P90_FLOOR[key], (key, "W", pw_g, pw_f)
            if nsub == 4 and (~Wm).sum() >= 2000:                 # measured for the control step (profiles/archive/r03_parity_p90.txt)
                mo_g, mo_f = np.median(gq[~Wm]), np.median(fq[~Wm])
                stats[f"p90_{key}"] += (float(mo_g), float(mo_f))
                assert mo_g <= P90_ALL_RATIO * mo_f + 20 * P90_FLOOR[key], (key, "outside W", mo_g, mo_f)
        print("p90 on W (GPU, oracle fp32-vs-fp64) and median outside W (GPU, oracle):", {k: tuple(f"{x:.2e}" for x in v) for k, v in stats.items() if k.startswith("p90_")})
    env.close(); substeps.close()
    return stats


def test_one_substep_launches_reproduce_the_control_step(layout):
    """what the post-mortem of run_parity stands on: a handle with ctrl_dt = sim_dt, launched n_substeps times on the physics kernel alone, ends on the
    bits of ONE launch of the control step's kernel (same lane layout; state round-trips through HBM instead of registers) - with DR and without"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    for task, ter, dr in (("stairs", terrain, False), ("stairs", terrain, True), ("flat_terrain", None, False)):
        n = 200
        env, hb, cs, ms = make_pair(task, n, ter, dr=dr)
        env.reset(3)
        rng = np.random.default_rng(4)
        for _ in range(6):
            env.step(torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda())
        torch.cuda.synchronize()
        S0 = env.buffers["state"].cpu().numpy()
        act = np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)
        env.step(torch.from_numpy(act).cuda())
        torch.cuda.synchronize()
        fin = env.buffers["state"][:55].cpu().numpy()
        for kk in ("params", "variant", "box_friction"):
            if kk in env.buffers:
                hb[kk][...] = env.buffers[kk].cpu().numpy()
        dev = X.DeviceSubsteps(task, env.config, env.model, ter, layout, n, {kk: hb[kk] for kk in ("params", "variant", "box_friction") if kk in env.buffers})
        subs = dev(np.arange(n), S0, act, None, 4)
        dev.close()
        rep = np.stack([np.concatenate([s[-1]["qpos"], s[-1]["qvel"], s[-1]["qacc"]]) for s in subs], 1)
        assert np.array_equal(rep, fin), (task, dr, np.abs(rep - fin).max())
        assert max(s[k]["niter"] for s in subs for k in range(4)) == 5
        env.close()


def audit_rollout(task, ter, dr, n, steps, layout, method="pgtt", min_minimiser=0.7, min_cut=50, model=None):
    """the device's every substep along a rollout through parity_explain.audit_control_step -> tally of verdicts (asserts: none unexplained, the replay
    reproduces the control step's bits, and the quality bar on the solves both sides cut).  `model`: another PgttModel dict than the task's (make_pair and
    DeviceSubsteps take it from there); the lifted-caps variant for the solver-parameter models is tests/test_gpu_solver_params.py::run_case"""
    env, hb, cs, ms = make_pair(task, n, ter, dr=dr, method=method, model=model)
    env.reset(3)
    rng = np.random.default_rng(4)
    for _ in range(12):                                                      # the landing
        env.step(torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda())
    dev = X.DeviceSubsteps(task, env.config, env.model, ter, layout, n, {kk: hb[kk] for kk in ("params", "variant", "box_friction") if kk in hb.arrays})
    tally, proofs, cols, gaps, sens_worst, scan_stat = {}, {}, np.arange(n), [], [0.0], [0, 0]
    for k in range(steps):
        torch.cuda.synchronize()
        S0 = env.buffers["state"].cpu().numpy()
        act = np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)
        env.step(torch.from_numpy(act).cuda())
        torch.cuda.synchronize()
        fin = env.buffers["state"].cpu().numpy()
        subs = dev(cols, S0, act, None, 4)
        rep = np.stack([np.concatenate([s_[-1]["qpos"], s_[-1]["qvel"], s_[-1]["qacc"]]) for s_ in subs], 1)
        assert np.array_equal(rep, fin[:55]), k
        # ... and the sensor frame the step hands to the task layer is the fp64 oracle's on the input of the device's LAST substep - every row that does not
        # hang on the solve (the accelerometer is affine in qacc and goes with it): gyro, the three trunk velocities, up vector, gravity, feet positions /
        # velocities / site heights, actuator forces, and the contact flags (a flag may differ only where a distance is within 1e-6 of 0)
        Fr, scan_dev = env.buffers["frame"].cpu().numpy(), env.buffers["scan_z"].cpu().numpy()
        for e in cols:
            sub = subs[e]
            inp = (S0[:19, e], S0[19:37, e], S0[37:55, e]) if len(sub) == 1 else (sub[-2]["qpos"], sub[-2]["qvel"], sub[-2]["qacc"])
            ed = X.env_data(hb, ter, int(e))
            D = oracle.forward(ms, *[np.asarray(v, np.float64) for v in inp[:2]], fin[abi.S_MOTOR_TARGETS:abi.S_MOTOR_TARGETS + 12, e].astype(np.float64),
                               np.asarray(inp[2], np.float64), boxes=ed.boxes, box_friction=ed.box_friction, params=ed.params, fp64=True)
            sd = D["sensordata"]
            want = {abi.F_GYRO: sd[0:3], abi.F_GLOBAL_LINVEL: sd[13:16], abi.F_GLOBAL_ANGVEL: sd[16:19], abi.F_LOCAL_LINVEL: sd[19:22], abi.F_UPVECTOR: sd[22:25],
                    abi.F_GRAVITY: -D["site_imu_mat"].reshape(-1)[6:9], abi.F_FEET_POS: sd[25:37], abi.F_FEET_VEL: sd[37:49], abi.F_ACT_FORCE: D["actuator_force"],
                    abi.F_FOOT_SITE_Z: D["site_foot"][[1, 0, 3, 2], 2]}
            for row, v in want.items():
                err = np.abs(Fr[row:row + len(v), e] - v) / (1 + np.abs(v))
                sens_worst[0] = max(sens_worst[0], float(err.max()))
                assert err.max() < 2e-5, (k, int(e), row, float(err.max()))
            for f, leg in enumerate((1, 0, 3, 2)):
                ds = [float(d) for ft, b, d in zip(D["con_foot"], D["con_box"], D["con_dist"]) if ft == leg and b != -2]
                flag = any(d < 0 for d in ds)
                assert bool(Fr[abi.F_CONTACT + f, e]) == flag or min(abs(d) for d in ds) < 1e-6, (k, int(e), f, ds)
            # ... and the 117 scan heights are the fp64 oracle's at the pose the step ended on (go2/heightmap.py:10-67), ray by ray; a ray that differs must be one
            # the fp32 oracle's own scan moves on by at least half as much when the pose moves by <= 2 roundings (a box edge, a near-vertical face)
            if ter is not None:
                qf = fin[:7, e].astype(np.float64)
                want = oracle.scan(cs, ed.boxes, qf[:3], oracle.quat_to_yaw(qf[3:7], fp64=True), fp64=True)[:, :, 2].reshape(-1)
                diff = np.abs(scan_dev[e] - want)
                rays = np.nonzero(diff > 1e-5)[0]
                scan_stat[0] += 117; scan_stat[1] += len(rays)
                if len(rays):
                    spread = X.scan_ensemble(cs, ed, fin[:19, e], fin[:19, e], seed=1000 * k + int(e))
                    assert all(spread[r] >= 0.5 * diff[r] for r in rays), (k, int(e), rays.tolist(), diff[rays].tolist(), spread[rays].tolist())
        for r in X.audit_control_step(ms, hb, ter, S0, fin[abi.S_MOTOR_TARGETS:abi.S_MOTOR_TARGETS + 12], subs, cols, seed=1000 * k):
            tally[r["cause"]] = tally.get(r["cause"], 0) + 1
            if r["cause"] == "cap":
                proofs[r["proof"]] = proofs.get(r["proof"], 0) + 1
            assert r["cause"] != "unexplained", (task, k, r)
            sens_worst.append(r["euler"])
            assert r["euler"] < 5e-7, (task, k, r)        # the integrator (measured 8e-8: one rounding): qvel' and qpos' are the semi-implicit Euler step of the device's own acceleration
            if "gap_dev" in r and r["niter"] >= int(ms.iterations) and r["niter_o32"] >= int(ms.iterations):
                gaps.append((max(r["gap_dev"], 1e-3), max(r["gap_o32"], 1e-3)))
    print(f"\n[{task} dr={dr} {layout} {method}] every substep of {n * steps} env-steps:", tally, f"; sensor frame against the fp64 oracle on the last substep's input: worst relative {sens_worst[0]:.2e}; Euler step of the device's own acceleration: worst {max(sens_worst[1:]):.2e}; scan rays off the fp64 oracle's by > 1e-5: {scan_stat[1]} of {scan_stat[0]} (each on an edge)")
    # the solves BOTH sides cut at the iteration cap from the same input: the device stops NO FURTHER from the minimum than the fp32 oracle does.  (The gap
    # above the minimum, in fp32 roundings of the cost's terms, spans five decades.  Measured: the device's median is 0.2 - 0.35 decades BELOW the oracle's, it
    # is better by more than a decade on 10 - 12 % of these solves and worse on 2 % - presumably because the arrowhead factorisation does a fifth of the dense
    # one's arithmetic, so its Newton directions carry less rounding error; not investigated further.  One-sided bar: a device that converged more slowly
    # than the reference would show here.)
    print(f"   how each `cap` was proven: {proofs} ({dev.launches} launches of the lifted handle)")
    assert sum(proofs.values()) == tally.get("cap", 0) and set(proofs) <= set(X.PROOFS) - {"reference"}, proofs
    lg = np.log10(np.array(gaps))
    worse, better = float(np.mean(lg[:, 0] > lg[:, 1] + 1)), float(np.mean(lg[:, 1] > lg[:, 0] + 1))
    print(f"   cut on both sides: {len(gaps)} solves, median log10 gap above the minimum: device {np.median(lg[:, 0]):.2f}, fp32 oracle {np.median(lg[:, 1]):.2f}; "
          f"device worse by more than a decade on {worse:.1%}, better on {better:.1%}")
    assert len(gaps) > min_cut and np.median(lg[:, 0]) < np.median(lg[:, 1]) + 0.25 and worse < better + 0.05
    assert tally["minimiser"] > min_minimiser * 4 * n * steps and tally.get("cap", 0) + tally.get("edge of W", 0) > 0
    dev.close(); env.close()
    tally["cap_proof"] = proofs
    return tally


def test_every_device_substep_is_the_minimiser_or_says_why(layout):
    """A statement that needs no W and no oracle trajectory: EVERY mjx.step the kernels take along a rollout - no selection by convergence, none by
    violation - returns the minimiser of that substep's convex problem (fp64 oracle from the device's own input, caps lifted) to a tenth of the bars with
    the fp64 oracle's ACTIVE contact set, or shows why not: it stopped at the iteration cap (`cap`; the fp64 oracle at the reference's caps is cut there
    too: `edge of W`), on the fp32 resolution of its cost (`floor`), a contact distance or a sphere centre sits within 1e-6 of a surface (`sign` / `tie`),
    or the fp32 oracle's own answer moves as far under two roundings of the input (`unstable`).  Nothing may be left unexplained.  level4 and the flat
    task with DR; tests/test_parity_explain.py makes the same statement about a second fp32 build of the oracle, on the CPU."""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    audit_rollout("stairs", terrain, False, 256, 10, layout)
    audit_rollout("flat_terrain", None, True, 128, 8, layout)


def test_device_solver_with_lifted_caps_reaches_the_minimiser(layout):
    """The solver's correctness on EVERY input of a rollout, W or not, with no cut to hide behind: each substep of 64 envs x 6 control steps (after a
    12-step landing; level4, and the flat task with DR) is taken once more by a handle whose model carries iterations = 64, ls_iterations = 60 - what
    pgtt_create accepts, read by the kernels at run time - from the capped run's input, whole batch, and judged against a* (fp64 oracle, 100 x 60) at
    OFF_DV / OFF_REL with the fp64 oracle's contact set.  Every solve ends `minimiser`, `floor`, `sign`, `tie` or `unstable`; none runs 64 iterations
    and stays off a*; and the capped sequence still ends on the control step's bits with the lifted handle at work beside it."""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    n, steps = 64, 6
    for task, ter, dr in (("stairs", terrain, False), ("flat_terrain", None, True)):
        env, hb, cs, ms = make_pair(task, n, ter, dr=dr)
        env.reset(3)
        rng = np.random.default_rng(4)
        for _ in range(12):                                                      # the landing
            env.step(torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda())
        dev = X.DeviceSubsteps(task, env.config, env.model, ter, layout, n, {kk: hb[kk] for kk in ("params", "variant", "box_friction") if kk in hb.arrays}, lift_all=True)
        tally, cols, worst_iter = {}, np.arange(n), 0
        for k in range(steps):
            torch.cuda.synchronize()
            S0 = env.buffers["state"].cpu().numpy()
            act = np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)
            env.step(torch.from_numpy(act).cuda())
            torch.cuda.synchronize()
            fin = env.buffers["state"].cpu().numpy()
            subs = dev(cols, S0, act, None, 4)
            rep = np.stack([np.concatenate([s_[-1]["qpos"], s_[-1]["qvel"], s_[-1]["qacc"]]) for s_ in subs], 1)
            assert np.array_equal(rep, fin[:55]), (task, k)
            for r in X.audit_lifted(ms, hb, ter, S0, fin[abi.S_MOTOR_TARGETS:abi.S_MOTOR_TARGETS + 12], subs, cols, seed=1000 * k):
                tally[r["cause"]] = tally.get(r["cause"], 0) + 1
                worst_iter = max(worst_iter, r["niter"])
                assert r["cause"] in ("minimiser", "floor", "sign", "tie", "unstable"), (task, k, r)
                assert r["niter"] < X.LIFT_ITER or r["cause"] in ("minimiser", "floor"), (task, k, r)
        share = (tally.get("minimiser", 0) + tally.get("floor", 0)) / (4 * n * steps)
        print(f"\n[{task} dr={dr} {layout}] lifted replay of every substep of {n * steps} env-steps:", tally, f"; minimiser + floor: {share:.4f}; most iterations: {worst_iter}; "
              f"{dev.launches} launches of the lifted handle")
        assert dev.launches == 4 * steps
        # the CPU stand-in (the oracle's -O3 -march=native build with the same lifted caps, tests/test_parity_explain.py::
        # test_second_fp32_build_with_lifted_caps_reaches_the_minimiser, same workloads) reaches minimiser + floor on 1536 of 1536 substeps of either workload:
        # share 1.0000.  The device is held to that minus two points: the binomial noise of about 1500 solves
        assert share >= 1.0000 - 0.02, (task, share, tally)
        dev.close(); env.close()


def test_an_envs_bits_do_not_depend_on_its_wave_mates(layout):
    """The premise of DeviceSubsteps' whole-batch replay, by the protocol of tools/gpu_wave_company.py: 48 envs step as one batch, and every third of them
    as a batch of 16 from the same states - other wave mates, 12 control steps.  The physics rows state[:55] are bit-equal in the quad layout on both tasks
    (an env's arithmetic does not see its wave there, by construction) and in every layout on the flat task; on level4 the oct layout splits a wave's
    contact work by the box slots in use ANYWHERE in the wave and hex switches on four box contacts of one foot (profiles/r06_wave_company.txt: 148 and 0 of
    20480): those two counts are printed, not asserted - they are why the replay takes the whole batch."""
    from phase_guided_terrain_traversal_amd.env import Joystick
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    n, steps = 48, 12
    variant = np.random.default_rng(2).integers(0, terrain.shape[0], n).astype(np.int32)
    third = np.arange(0, n, 3)
    ti = torch.from_numpy(third).cuda()
    for task, ter in (("stairs", terrain), ("flat_terrain", None)):
        mk = lambda idx: Joystick(task, configs.training_config(), num_envs=len(idx), terrain=ter, device="cuda:0", layout=layout,
                                  **({"variant": torch.from_numpy(variant[idx])} if ter is not None else {}))
        A, B = mk(np.arange(n)), mk(third)
        A.reset(3)
        rng = np.random.default_rng(0)
        diff = 0
        for k in range(steps):
            a = torch.from_numpy(np.tanh(rng.normal(size=(n, 12)) * 0.6).astype(np.float32)).cuda()
            for key in ("state", "istate"):
                B.buffers[key].copy_(A.buffers[key][..., ti])
            B.buffers["scan_z"].copy_(A.buffers["scan_z"][ti])
            A.step(a); B.step(a[ti].contiguous())
            torch.cuda.synchronize()
            diff += int((A.buffers["state"][:55, ti] != B.buffers["state"][:55]).any(0).sum())
        print(f"\n[{task} {layout}] {diff} of {steps * len(third)} env-steps differ in qpos / qvel / warm start between the whole batch and the every-third-env batch")
        assert torch.isfinite(B.buffers["state"][:55]).all()
        if layout == "quad" or ter is None:
            assert diff == 0, (task, layout, diff)
        A.close(); B.close()


@pytest.mark.parametrize("which", ["level13_dr", "random_boxes", "ramps", "overlap", "baseline"])
def test_every_device_substep_on_the_harder_terrains(which):
    """the same audit where the contact geometry is least kind: level13 with the full domain randomisation (per-env masses, gains, frictions), 100 boxes
    thrown at random (any orientation, any overlap), pitched and rolled ramps, three overlapping slabs (up to 12 simultaneous contacts of equal depth),
    and the baseline task's kernels"""
    lay = "hex"
    if which == "level13_dr":
        audit_rollout("stairs", np.load(os.path.join(ASSETS, "terrains", "level13.npy")), True, 192, 8, lay)
    elif which == "random_boxes":
        audit_rollout("stairs", random_box_terrain(5, 100), False, 160, 8, lay, min_minimiser=0.5)
    elif which == "ramps":
        audit_rollout("stairs", ramp_terrain(), False, 160, 8, lay, min_minimiser=0.5)
    elif which == "overlap":
        audit_rollout("stairs", overlap_terrain(), False, 128, 8, lay, min_minimiser=0.4, min_cut=30)
    else:
        audit_rollout("stairs", np.load(os.path.join(ASSETS, "terrains", "level4.npy")), False, 128, 6, lay, method="baseline")


def test_flat_parity(layout):
    st = run_parity("flat_terrain", 256, None, steps=40)
    assert st["active_contacts"] > 1000


def test_flat_dr_parity(layout):
    """the flat task WITH domain randomisation (go2/randomize_simple.py:24-138: floor friction U(0.4, 1), masses, armature, damping, gains, qpos0 per env;
    no boxes): the DR-without-terrain kernels of every layout, step and reset's forward pass, AutoReset on"""
    st = run_parity("flat_terrain", 192, None, steps=30, dr=True, autoreset=True, w_floor=0.65)          # measured W = 72.7 %: robots with randomised gains land harder
    assert st["active_contacts"] > 3000 and st["box_contacts"] == 0


@pytest.fixture(params=["quad", "oct", "hex"])
def layout(request):
    """the three lane layouts of physics_kernel (pgtt_physics_quad.hip.h): 16, 8 or 4 envs per wave"""
    EXEC["layout"] = request.param
    yield request.param
    EXEC["layout"] = None


def test_level4_parity(layout):
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    st = run_parity("stairs", 256, terrain, steps=60)


def test_single_mjx_step_parity(layout):
    """north star, literally: ONE mjx.step from identical (qpos, qvel, ctrl, terrain) - ctrl_dt = sim_dt, so a control step is a
    single physics substep and errors are not compounded over four of them; W = 86-87 % of env-steps here"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    run_parity("stairs", 256, terrain, steps=60, ctrl_dt=0.005)
    run_parity("flat_terrain", 256, None, steps=40, ctrl_dt=0.005)


def test_level13_dr_autoreset_parity(layout):
    terrain = np.load(os.path.join(ASSETS, "terrains", "level13.npy"))
    run_parity("stairs", 128, terrain, steps=40, dr=True, autoreset=True)


def test_wfc_terrain_full_dr_parity(layout):
    """BASELINE configs[3] through the parity bar: terrain GENERATED on the host by the wave-function-collapse pipeline
    (terrain_gen.create_random_matrix = terrain/generator.py:368-391 + getIndexes.py:28-79 + wfc) and the full randomize.py DR
    (go2/randomize.py:23-171), with the AutoReset wrapper on, all lane layouts (8192 envs run the oct layout)"""
    from phase_guided_terrain_traversal_amd.terrain_gen import create_random_matrix
    terrain = create_random_matrix(100, 100, 5, 0.05, 0.13, seed=3)
    assert terrain.shape == (100, 100, 10) and terrain.dtype == np.float32
    st = run_parity("stairs", 192, terrain, steps=30, dr=True, autoreset=True)
    assert st["box_contacts"] > 1000


@pytest.mark.parametrize("level", ["1", "2", "3", "7", "10", "05", "09"])
def test_curriculum_levels_parity(level):
    """the remaining level files of the reference's training curriculum (BASELINE configs[4]; level4 and level13 are covered
    above; level2 / level3 hold 50 variants instead of 100) and two of its fixed-step-height evaluation series level01..09
    (training/evaluate_multiple.py:11-12) through the same parity bar, default lane layout"""
    terrain = np.load(os.path.join(ASSETS, "terrains", f"level{level}.npy"))
    run_parity("stairs", 128, terrain, steps=24)


def test_ragged_env_counts_parity(layout):
    """env counts that are not multiples of the 16 envs of a wave (partial last wave, grid not a multiple of the 8
    XCDs, a single partial wave) go through the same parity bar"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    run_parity("stairs", 203, terrain, steps=16)
    run_parity("flat_terrain", 37, None, steps=16)
    run_parity("flat_terrain", 5, None, steps=8, w_floor=0.5)        # 40 env-steps: the share of W is 28-33 of them, not a statistic
    run_parity("flat_terrain", 1, None, steps=12, w_floor=0.0)       # ONE env: a single wave with one live quad / row / leg group
    run_parity("stairs", 1, terrain, steps=12, w_floor=0.0)


def test_level4_parity_full_size():
    """BASELINE configs[2] AT ITS SIZE against the oracle: 4096 envs on level4, the lane layout, XCD block mapping and env labelling the bench
    times (layout auto = hex at 4096; variants as randomize.domain_randomize hands them out), 8 control steps = 32 768 env-steps through the
    same bar as the small cases (the oracle needs a few seconds for them on the host cores)"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    st = run_parity("stairs", 4096, terrain, steps=8, product_variants=True)
    assert st["active_contacts"] > 20000


def test_level4_parity_16384_envs_quad_by_auto():
    """beyond 8192 envs the automatic layout is quad (16 envs per wave, one workgroup per SIMD since its box data are read from the resident table
    instead of an LDS copy): 16384 envs on level4 = one round of 1024 waves, 3 control steps against the oracle, product variant labelling"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    st = run_parity("stairs", 16384, terrain, steps=3, product_variants=True, w_floor=0.6)
    assert st["active_contacts"] > 20000


def test_flat_parity_full_size():
    """BASELINE configs[1] at its size: 4096 envs on the plane, no DR, layout auto (hex), 8 control steps against the oracle"""
    st = run_parity("flat_terrain", 4096, None, steps=8)
    assert st["active_contacts"] > 20000


def test_wfc_dr_parity_full_size():
    """BASELINE configs[3] at its size: 8192 envs (layout auto = oct), WFC-generated terrain, full randomize.py DR, AutoReset on, 6 control steps"""
    from phase_guided_terrain_traversal_amd.terrain_gen import create_random_matrix
    terrain = create_random_matrix(100, 100, 5, 0.05, 0.13, seed=3)
    st = run_parity("stairs", 8192, terrain, steps=6, dr=True, autoreset=True)
    assert st["box_contacts"] > 4000


def test_baseline_method_parity():
    """the comparison task go2/joystick.py (162 / 206 observations, world-frame clearance, H_max = quadrant max)"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    st = run_parity("stairs", 128, terrain, steps=30, autoreset=True, method="baseline")
    env, _, _, _ = make_pair("stairs", 16, terrain, method="baseline")
    assert env.observation_size == {"state": 162, "privileged_state": 206}
    obs = env.reset(seed=1)
    assert obs["state"].shape == (16, 162) and obs["privileged_state"].shape == (16, 206)
    env.close()


def test_split_observe_parity():
    """observe as two kernels (scan + observation rows per wave, rewards / bookkeeping / AutoReset per lane), the path
    taken from 16 k envs: same parity bar, AutoReset included"""
    EXEC["observe_form"] = "split"
    try:
        terrain = np.load(os.path.join(ASSETS, "terrains", "level13.npy"))
        run_parity("stairs", 128, terrain, steps=40, dr=True, autoreset=True)
        run_parity("flat_terrain", 100, None, steps=20, autoreset=True, method="baseline")
    finally:
        EXEC["observe_form"] = None


def test_library_refuses_without_bind():
    import ctypes as C
    from phase_guided_terrain_traversal_amd import native
    L = native.lib()
    cs = abi.config_struct(configs.default_config()); ms = abi.model_struct(mjcf.load_model("flat_terrain"))
    h = C.c_void_p()
    native.check(L.pgtt_create(C.byref(cs), C.byref(ms), 0, 64, C.byref(h)))
    assert L.pgtt_step(h, None, None) == -2            # PGTT_E_STATE
    assert b"pgtt_bind" in L.pgtt_last_error()
    L.pgtt_destroy(h)


_SIDE_BUILD_PROBE = """
import os, sys
import numpy as np, torch
from phase_guided_terrain_traversal_amd import configs, native
from phase_guided_terrain_traversal_amd.env import Joystick
assert native.build_info()["flavor"] == "fastdiv", native.build_info()
terrain = np.load(os.path.join(os.path.dirname(native.__file__), "assets", "terrains", "level4.npy"))
msg = "does not contain the physics_kernel variant the call needs"
for lay in ("quad", "oct"):                               # libpgtt_fastdiv.so holds the hex step / forward kernels on box terrain without DR only
    env = Joystick("stairs", configs.training_config(), num_envs=64, terrain=terrain, device="cuda:0", layout=lay)
    before = {k: v.clone() for k, v in env.buffers.items() if torch.is_tensor(v)}
    for call in (lambda: env.reset(1), lambda: env.step(torch.zeros(64, 12, device="cuda:0"))):
        try:
            call()
        except native.PgttError as err:
            assert "libpgtt error -2" in str(err) and msg in str(err), str(err)     # PGTT_E_STATE
        else:
            raise AssertionError("a launch of a variant that was not built must fail: " + lay)
    torch.cuda.synchronize()
    assert all(torch.equal(v, env.buffers[k]) for k, v in before.items()), lay          # nothing was written
    env.close()
env = Joystick("stairs", configs.training_config(), num_envs=64, terrain=terrain, device="cuda:0", layout="hex")
env.reset(1); env.step(torch.zeros(64, 12, device="cuda:0")); torch.cuda.synchronize()
assert torch.isfinite(env.buffers["state"]).all()
env.close()
print("side build probe ok")
"""


def test_variant_missing_from_a_side_build_is_an_error_that_writes_nothing():
    """libpgtt_fastdiv.so (csrc/Makefile `fastdiv`) compiles two of the 36 physics_kernel variants: a call that needs another one returns PGTT_E_STATE
    before anything is launched; the variants it holds run.  In a child process: PGTT_LIB is read when the library is first loaded."""
    import subprocess, sys
    from phase_guided_terrain_traversal_amd import native
    lib = os.path.join(os.path.dirname(native.__file__), "libpgtt_fastdiv.so")
    assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() makes it (make -C csrc fastdiv)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(native.__file__)))
    r = subprocess.run([sys.executable, "-c", _SIDE_BUILD_PROBE], cwd=root, env=dict(os.environ, PGTT_LIB=lib), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "side build probe ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def nearest_boxes(terrain, B):
    """the B boxes of every variant whose centres lie nearest to the spawn area: a terrain table with FEWER than 100 boxes per variant"""
    out = np.zeros((terrain.shape[0], B, 10), np.float32)
    for v in range(terrain.shape[0]):
        order = np.argsort(np.hypot(terrain[v, :, 0], terrain[v, :, 1]), kind="stable")[:B]
        out[v] = terrain[v, np.sort(order)]
    return out


@pytest.mark.parametrize("B", [37, 6, 1])
def test_fewer_than_100_boxes_parity(layout, B):
    """pgtt_set_terrain accepts any B <= 100 (the reference's scene always carries 100 placeholders, terrain_scene_mjx.xml:20-21): B = 37 leaves every
    sub-lane split of the 100-box loops ragged and ends the table of the LAST variant exactly at its last record (the quad layout's rank pass used to
    prefetch one record further: ADVICE r04); B = 6 is the largest count for which MJX's broad phase does not cut (4 x 6 = 24 <= max_geom_pairs = 25: every
    pair goes to the narrow phase); B = 1 is a single slab"""
    lvl = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    terrain = nearest_boxes(lvl, B)
    if B == 1:
        terrain[:, 0] = [0.0, 0.0, 0.03, 1, 0, 0, 0, 2.0, 2.0, 0.03]
        terrain[1::2, 0, 7] = 0.6                      # every other variant: a narrower slab, so feet also meet its edges and the plane
    assert terrain.shape[1] == B
    st = run_parity("stairs", 128, terrain, steps=20, w_floor=0.6)
    assert st["box_contacts"] > (300 if B > 1 else 1500)
    # the same with domain randomisation (per-box friction rows are [100][N] whatever B is) and AutoReset
    if B == 37:
        run_parity("stairs", 96, terrain, steps=16, dr=True, autoreset=True, w_floor=0.6)


def test_single_variant_terrain_without_a_variant_buffer():
    """PgttBuffers.variant = NULL means variant 0 for every env (include/pgtt.h): a one-variant table, no label buffer bound on either side"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))[7:8]
    st = run_parity("stairs", 128, terrain, steps=20, no_variant_buffer=True)
    assert st["box_contacts"] > 300


@pytest.mark.parametrize("nsub", [2, 8])
def test_other_substep_counts_parity(nsub):
    """n_substeps = round(ctrl_dt / sim_dt) is a config value (go2/configs.py:8-9; pgtt_create accepts 1 .. 64): two and eight mjx.step per control step
    through the same bar - the longer the step, the fewer env-steps keep all their solves converged (measured W: 86 / 83 / 76 / 72 % for 1 / 2 / 4 / 8 substeps)"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    run_parity("stairs", 128, terrain, steps=24, ctrl_dt=0.005 * nsub, w_floor=0.80 if nsub == 2 else 0.55, cap_scale=1.0 if nsub == 2 else 2.0)


def test_short_episodes_autoreset_parity(layout):
    """Episode(7) + AutoReset against the oracle: within 24 control steps every env is truncated three times and restored from its first state
    (joystick wrappers of training/train.py:255,262), full DR, level13"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level13.npy"))
    st = run_parity("stairs", 128, terrain, steps=24, dr=True, autoreset=True, cfg_over={"episode_length": 7})
    assert st["active_contacts"] > 1000


@pytest.mark.parametrize("method", ["pgtt", "baseline"])
def test_config_values_are_read_not_assumed(method):
    """every scalar of go2/configs.py:6-79 that the step consumes is a run-time value of PgttConfig: with ALL of them moved off the reference's defaults
    (all 21 reward scales non-zero - several are 0.0 in the shipped config, so their terms would otherwise never show -, the tracking / phase sigmas, swing
    height and foot distance, command ranges and probabilities, gait-frequency range, the scan pitch and ray height, every noise scale, action scale, soft
    limit factor, history period, episode length) the kernels still agree with the oracle, which reads the same struct"""
    rng = np.random.default_rng(5)
    over = {"reward_config.scales." + k: float(np.sign(v if v != 0 else rng.choice([-1.0, 1.0])) * rng.uniform(0.2, 1.5) * (abs(v) if v != 0 else 0.3))
            for k, v in configs.default_config()["reward_config"]["scales"].items()}
    over.update({"reward_config.tracking_sigma": 0.31, "reward_config.swing_height": -0.17, "reward_config.base_feet_distance": -0.27, "reward_config.phase_sigma": 0.08,
                 "command_config.u_max": [0.9, 0.5, 0.8], "command_config.u_min": [-0.4, -0.6, -1.1], "command_config.b": [0.7, 0.4, 0.6], "gait_freq": [1.5, 2.5],
                 "scan_dist_x": 0.08, "scan_dist_y": 0.12, "scan_z_offset": 0.45, "action_scale": 0.35, "soft_joint_pos_limit_factor": 0.9, "history_update_steps": 3,
                 "episode_length": 11})
    over.update({"noise_config.scales." + k: v for k, v in dict(joint_pos=0.05, joint_vel=1.0, gyro=0.3, gravity=0.08, linvel=0.2, heightscan=0.02).items()})
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    st = run_parity("stairs", 128, terrain, steps=30, autoreset=True, method=method, cfg_over=over)
    assert st["box_contacts"] > 500


def perturbed_model(task, axes=False, seed=9):
    """PgttModel with the numeric fields moved off the Go2's values (what a different MJCF of the same topology would compile to): link offsets, inertial
    frames, masses, inertias, joint ranges (narrow: limit rows become active), joint and geom solver parameters, armature, damping, actuator gains / bias /
    ranges (tight force range: clipping becomes active), foot geometry, imu and foot sites, frictions, margins, a tilted gravity, impratio, solver tolerances
    and iteration counts, the collision cuts (max_geom_pairs 17, max_contact_points 3), another keyframe.
    LEFT AT THEIR DEFAULTS: the midpoint and power of all four solimp vectors (0.5, 2.0: kbi()'s power == 2 branch), and every solref stays in the standard
    form above 2 dt with solmix weights well above mjMINVAL - the general power, the direct forms, the `min` rule, the mjMINVAL weights and the clamps are
    tests/solver_param_cases.py and tests/test_gpu_solver_params.py"""
    m = {k: (np.array(v, dtype=np.float64, copy=True) if isinstance(v, (list, np.ndarray)) else v) for k, v in mjcf.load_model(task).items()}
    r = np.random.default_rng(seed)
    sc = lambda a, rel: np.asarray(a, np.float64) * (1 + r.uniform(-rel, rel, np.shape(a)))
    m["body_pos"] = m["body_pos"] + r.uniform(-0.01, 0.01, (13, 3)); m["body_ipos"] = m["body_ipos"] + r.uniform(-0.005, 0.005, (13, 3))
    q = m["body_iquat"] + r.normal(size=(13, 4)) * 0.05; m["body_iquat"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    m["body_mass"] = sc(m["body_mass"], 0.15); m["body_inertia"] = sc(m["body_inertia"], 0.15); m["body_invweight0"] = sc(m["body_invweight0"], 0.1)
    m["dof_invweight0"] = sc(m["dof_invweight0"], 0.1); m["meaninertia"] = float(m["meaninertia"]) * 1.1
    jr = np.asarray(m["jnt_range"], np.float64); mid, half = jr.mean(1), 0.5 * (jr[:, 1] - jr[:, 0])
    m["jnt_range"] = np.stack([mid - 0.8 * half, mid + 0.8 * half], 1)
    m["jnt_solref"] = np.array([0.03, 0.9]); m["jnt_solimp"] = np.array([0.85, 0.97, 0.002, 0.5, 2.0])
    m["dof_armature"] = np.asarray(m["dof_armature"], np.float64) + np.r_[np.zeros(6), r.uniform(0.0, 0.02, 12)]
    m["dof_damping"] = np.asarray(m["dof_damping"], np.float64) * np.r_[np.ones(6), r.uniform(0.6, 1.6, 12)]
    g = r.uniform(25.0, 45.0, 12); m["act_gain"] = g
    b = np.asarray(m["act_bias"], np.float64).copy(); b[:, 1] = -g; b[:, 2] = -r.uniform(0.2, 1.0, 12); m["act_bias"] = b
    m["act_forcerange"] = np.stack([-r.uniform(8, 14, 12), r.uniform(8, 14, 12)], 1)
    cr = np.asarray(m["act_ctrlrange"], np.float64); m["act_ctrlrange"] = np.stack([cr[:, 0] + 0.1, cr[:, 1] - 0.1], 1)
    m["foot_geom_pos"] = m["foot_geom_pos"] + r.uniform(-0.004, 0.004, (4, 3)); m["foot_radius"] = np.array([0.02, 0.019, 0.021, 0.0205])
    m["foot_site_pos"] = m["foot_site_pos"] + r.uniform(-0.004, 0.004, (4, 3)); m["imu_pos"] = m["imu_pos"] + r.uniform(-0.01, 0.01, 3)
    m["foot_friction"] = np.array([0.7, 0.005, 0.0001]); m["floor_friction"] = np.array([0.8, 0.005, 0.0001]); m["box_friction"] = np.array([0.55, 0.005, 0.0001])
    for k in ("foot", "floor", "box"):
        m[k + "_solref"] = np.array([0.02 + 0.004 * r.uniform(), 0.9 + 0.2 * r.uniform()]); m[k + "_solimp"] = np.array([0.7 + 0.2 * r.uniform(), 0.96, 0.002 + 0.02 * r.uniform(), 0.5, 2.0])
        m[k + "_solmix"] = 0.5 + r.uniform()
    # the plane contact takes any margin (here + 1 mm: rows of feet that hover become active); foot-box pairs need a mixed margin <= 0 (pgtt_create refuses more)
    m["foot_margin"] = -0.0005; m["box_margin"] = -0.001; m["floor_margin"] = 0.0015; m["floor_gap"] = 0.0005
    m["gravity"] = np.array([0.4, -0.3, -9.6]); m["impratio"] = 60.0; m["tolerance"] = 1e-7; m["ls_tolerance"] = 0.02
    m["iterations"] = 6; m["ls_iterations"] = 7; m["max_geom_pairs"] = 17; m["max_contact_points"] = 3; m["box_rbound"] = 1.5
    kq = np.asarray(m["key_qpos"], np.float64).copy(); kq[2] = 0.30; kq[7:] += np.tile([0.05, -0.1, 0.15], 4); m["key_qpos"] = kq
    if axes:
        ax = np.asarray(m["jnt_axis"], np.float64) + r.normal(size=(12, 3)) * 0.08; m["jnt_axis"] = ax / np.linalg.norm(ax, axis=1, keepdims=True)
    return m


@pytest.mark.parametrize("task", ["stairs", "flat_terrain"])
def test_model_values_are_read_not_assumed(layout, task):
    """the kernels take the robot from PgttModel, not from constants: a model of the same topology with its numeric fields changed (perturbed_model; all but
    solimp's midpoint and power, which keep 0.5 and 2.0, and with every solver parameter inside its standard range - those branches are held by
    tests/test_gpu_solver_params.py) goes through the parity bar, oracle and kernels reading the same struct - narrow joint ranges and tight force ranges make limit rows and actuator clipping
    active, 6 Newton / 7 line-search iterations, max_geom_pairs = 17 and max_contact_points = 3 move every cut of the solver and the collision stage"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy")) if task == "stairs" else None
    st = run_parity(task, 128, terrain, steps=24, model=perturbed_model(task, axes=True), w_floor=0.55, cap_scale=2.0, med_tol=4e-6)        # hinge axes tilted by ~5 degrees too
    assert st["active_contacts"] > 1500


def random_box_terrain(seed, nplaced):
    """boxes with ANY orientation (uniform random quaternions), half-sizes 2 - 35 cm, centres scattered over the spawn area at heights that leave their highest
    corners 0 - 30 cm above the floor, overlapping at random: corners, edges and steep faces under the feet, scan rays through tilted boxes"""
    r = np.random.default_rng(seed)
    T = []
    for v in range(6):
        rows = []
        for _ in range(nplaced):
            q = r.normal(size=4); q /= np.linalg.norm(q)
            size = r.uniform(0.02, 0.35, 3)
            reach = float(np.abs(size).sum())                # upper bound of the box's vertical half extent in any orientation
            rows.append([r.uniform(-1.3, 1.3), r.uniform(-1.3, 1.3), r.uniform(0.0, 0.3) - 0.6 * reach, *q, *size])
        rows += [[100.0 + n, 100.0 + n, 100.0 + n, 1, 0, 0, 0, 0.5, 0.5, 0.5] for n in range(100 - nplaced)]
        T.append(rows)
    return np.asarray(T, dtype=np.float32)


@pytest.mark.parametrize("nplaced", [25, 100])
def test_random_box_terrain_parity(layout, nplaced):
    """collision, contact frames, top-k selection and the scan on boxes nobody arranged: 25 or all 100 boxes per variant thrown at random (any orientation, any
    overlap) - sphere-box contacts on faces, edges and corners of rotated boxes, feet inside several boxes at once (the exact many-box pass where needed),
    rays through tilted boxes; the full bar against the oracle"""
    terrain = random_box_terrain(17 + nplaced, nplaced)
    st = run_parity("stairs", 160, terrain, steps=24, w_floor=0.45, cap_scale=3.0, med_tol=6e-6)
    assert st["box_contacts"] > 800


def test_extreme_states_parity(layout):
    """ONE control step from states no roll-out of this suite visits: any base orientation (robots on their backs: termination), bases 5 - 60 cm above the
    floor or the stairs (feet deep inside boxes or in the air), joints up to 20 % beyond their ranges (limit rows at work), joint speeds up to 12 rad/s,
    base spins up to 6 rad/s, a stale warm start - the oracle from the identical state, the bar on W; everything finite everywhere"""
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    n = 512
    env, hb, cs, ms = make_pair("stairs", n, terrain)
    h64 = oracle.HostBuffers(n, with_variant=True); h64["variant"][...] = hb["variant"]
    env.reset(3)
    torch.cuda.synchronize()
    r = np.random.default_rng(21)
    model = mjcf.load_model("stairs")
    jr = np.asarray(model["jnt_range"], np.float64); mid, half = jr.mean(1), 0.5 * (jr[:, 1] - jr[:, 0])
    S = env.buffers["state"].cpu().numpy()
    q = r.normal(size=(4, n)); q /= np.linalg.norm(q, axis=0, keepdims=True)
    upright = r.uniform(size=n) < 0.5                          # half of them keep a near-upright base (otherwise nearly every env would be terminal)
    yaw = r.uniform(-3.14, 3.14, n); tilt = r.normal(size=(2, n)) * 0.15
    qu = np.stack([np.cos(yaw / 2), tilt[0], tilt[1], np.sin(yaw / 2)]); qu /= np.linalg.norm(qu, axis=0, keepdims=True)
    S[3:7] = np.where(upright[None], qu, q)
    S[0:2] = r.uniform(-1.0, 1.0, (2, n)); S[2] = r.uniform(0.05, 0.6, n)
    S[7:19] = (mid[:, None] + half[:, None] * r.uniform(-1.2, 1.2, (12, n)))
    S[19:22] = r.uniform(-1.5, 1.5, (3, n)); S[22:25] = r.uniform(-6.0, 6.0, (3, n)); S[25:37] = r.uniform(-12.0, 12.0, (12, n))
    S[37:55] = r.normal(size=(18, n)) * 30.0
    env.buffers["state"].copy_(torch.from_numpy(S))
    sync_to_host(env, hb, h64)
    act = np.tanh(r.normal(size=(n, 12))).astype(np.float32)
    env.step(torch.from_numpy(act).cuda())
    r64 = np.zeros(n)
    oracle.step(cs, ms, terrain, hb, act, seed=3, nthreads=8)
    oracle.step(cs, ms, terrain, h64, act, seed=3, nthreads=8, fp64=True, resid=r64)
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in env.buffers.items()}
    assert all(np.isfinite(g[k]).all() for k in ("state", "frame", "obs_state", "obs_priv", "reward", "metrics", "scan_z"))
    assert np.array_equal(g["istate"], hb["istate"])
    eg, ef = per_env_errors(g, hb), per_env_errors(hb.arrays, h64)
    well = (r64 < 1e-6) & (ef["qpos"] < 1e-5) & (ef["qvel"] < 1e-3)
    ga, ha = active_sets(g["dbg_contact"], g["dbg_dist"]), active_sets(hb["dbg_contact"], hb["dbg_dist"])
    sm = np.array([a != b for a, b in zip(ga, ha)])
    deep = sum(1 for e in range(n) for d in hb["dbg_dist"][e] if d < -0.0175)
    print(f"\n[extreme states, {layout}] W {well.mean():.2f}; done {int(hb['done'].sum())} of {n}; contacts deeper than the foot radius {deep}; on W: qpos > 1e-4 {(eg['qpos'][well] > 1e-4).sum()}, "
          f"qvel > 5e-3 {(eg['qvel'][well] > 5e-3).sum()}, ACTIVE-set mismatches {(sm & well).sum()}, done mismatches {((g['done'] != hb['done']) & well).sum()}")
    assert well.mean() > 0.3 and 0.2 * n < hb["done"].sum() < 0.8 * n and deep > 50
    assert (eg["qpos"][well] > 1e-4).sum() <= max(2, 0.01 * well.sum()) and (eg["qvel"][well] > 5e-3).sum() <= max(2, 0.01 * well.sum())
    assert (sm & well).sum() <= 1 and ((g["done"] != hb["done"]) & well).sum() == 0
    assert np.abs(g["scan_z"] - hb["scan_z"])[well].max() < 1e-4 or (np.abs(g["scan_z"] - hb["scan_z"])[well].max(1) > 1e-5).sum() <= 2
    env.close()


def test_terrain_table_beyond_32_bit_offsets_is_refused():
    """the quad / oct kernels address the terrain table and the cell grid through 32-bit byte offsets from their bases: a table that does not fit is a
    PGTT_E_ARG of pgtt_set_terrain (checked before the table is read), not a wrapped offset"""
    import ctypes as C
    from phase_guided_terrain_traversal_amd import native
    L = native.lib()
    cs = abi.config_struct(configs.default_config()); ms = abi.model_struct(mjcf.load_model("stairs"))
    h = C.c_void_p()
    native.check(L.pgtt_create(C.byref(cs), C.byref(ms), 0, 64, C.byref(h)))
    tiny = np.zeros((1, 100, 10), np.float32)
    assert L.pgtt_set_terrain(h, tiny.ctypes.data, 600000, 100) == -1 and b"too large" in L.pgtt_last_error()         # 600 000 x 100 x 80 B = 4.8 GB
    assert L.pgtt_set_terrain(h, tiny.ctypes.data, 1100000, 1) == -1 and b"too large" in L.pgtt_last_error()          # the grid: 1.1 M x 4096 B
    assert L.pgtt_set_terrain(h, tiny.ctypes.data, 1, 100) == 0
    L.pgtt_destroy(h)


def dense_terrain():
    """Terrain on which MJX's broad-phase top-k (max_geom_pairs = 25) REALLY truncates: 90 tiny 2 x 2 cm tiles
    (2 mm high, 4 cm pitch) cluster their centres around the spawn area, while ten long slabs (3 cm high) have their
    centres 0.9 m away.  A foot standing on a slab is then often NOT among the 25 nearest (foot, box) centre pairs,
    the contact is dropped exactly as in the reference, and the exact rank pass of the HIP kernel is exercised.
    At most two boxes overlap at any point (kMaxPenQ = 4 per foot is not exceeded)."""
    T = []
    for v in range(4):
        rows = []
        for i in range(10):
            for j in range(9):
                rows.append([(i - 4.5) * 0.04 + 0.01 * v, (j - 4.0) * 0.04, 0.001, 1, 0, 0, 0, 0.01, 0.01, 0.001])
        for k in range(5):
            y = (k - 2) * 0.25
            rows.append([0.9, y, 0.015, 1, 0, 0, 0, 0.85, 0.10, 0.015])
            rows.append([-0.9, y, 0.015 + 0.002 * v, 0, 0, 0, 1, 0.85, 0.10, 0.015 + 0.002 * v])     # yaw 180 deg
        T.append(rows)
    return np.asarray(T, dtype=np.float32)


def test_broadphase_truncation_parity(layout):
    terrain = dense_terrain()
    st = run_parity("stairs", 128, terrain, steps=25)
    assert st["box_contacts"] > 500


def overlap_terrain():
    """Equal penetration depths at the max_contact_points cut: three slabs with the SAME top height overlap over the
    whole spawn area, so every standing foot holds three contacts of identical depth (same top face, same sphere) and an env has up
    to 12 penetrating pairs for 4 slots.  MJX keeps, among equal depths, the pair with the lower broad-phase rank (lax.top_k is
    stable and the narrow phase runs in broad-phase order = by distance between the geom centres); the slab centres differ, so
    the order is well defined.  Variants shift the centres so that the nearest slab differs between feet and envs."""
    T = []
    for v in range(4):
        rows = [[0.3 + 0.1 * v, 0.2, 0.02, 1, 0, 0, 0, 3.0, 3.0, 0.02],
                [-0.4, -0.3 + 0.1 * v, 0.02, 1, 0, 0, 0, 3.0, 3.0, 0.02],
                [0.1 * v, 0.5, 0.02, 0, 0, 0, 1, 3.0, 3.0, 0.02]]
        rows += [[100.0 + k, 100.0 + k, 100.0 + k, 1, 0, 0, 0, 0.5, 0.5, 0.5] for k in range(97)]      # parked placeholders (terrain_scene_mjx.xml)
        T.append(rows)
    return np.asarray(T, dtype=np.float32)


def test_equal_depth_tie_break_parity(layout):
    """ties at the top-4 cut are broken like lax.top_k does (lower broad-phase rank first): same ACTIVE set as the oracle"""
    st = run_parity("stairs", 128, overlap_terrain(), steps=25, w_floor=0.48, cap_scale=4.0, med_tol=6e-6)      # up to 12 simultaneous contacts: W = 55 % here, stiffer solves
    assert st["box_contacts"] > 2000


def stacked_slabs_terrain():
    """MORE than four boxes penetrated by one foot (kMaxPenQ): ten slabs of graded height, tops 1.5 mm apart, overlap over the
    whole spawn area.  A standing foot is 5-15 mm inside the tallest one and so penetrates six to ten slabs at once, every env has 25-40
    penetrating pairs for 4 contact slots and MJX's max_geom_pairs = 25 cut (go2_mjx_feetonly.xml:14-15) bites as well.  MJX keeps the four
    DEEPEST pairs of the env among the 25 closest ones."""
    T = []
    for v in range(4):
        rows = [[0.05 * k - 0.2 + 0.03 * v, 0.04 * k - 0.15, 0.5 * (0.040 - 0.0015 * k), 1, 0, 0, 0, 3.0, 3.0, 0.5 * (0.040 - 0.0015 * k)] for k in range(10)]
        rows += [[100.0 + k, 100.0 + k, 100.0 + k, 1, 0, 0, 0, 0.5, 0.5, 0.5] for k in range(90)]
        T.append(rows)
    return np.asarray(T, dtype=np.float32)


def equal_top_slabs_terrain():
    """Seven slabs with the SAME top face overlap over the spawn area (equal depths at the cut, more than four per foot), their centres spread so
    that the max_geom_pairs = 25 cut removes, for some feet, pairs that are as deep as the kept ones: which four of the 28 penetrating pairs
    survive is decided by the broad-phase order alone.  Two more slabs are lower (never selected while a top slab survives the cut)."""
    T = []
    for v in range(4):
        rows = [[0.35 * np.cos(0.9 * k + 0.2 * v), 0.35 * np.sin(0.9 * k + 0.2 * v), 0.015, 1, 0, 0, 0, 3.0, 3.0, 0.015] for k in range(7)]
        rows += [[0.02 * v, 0.01, 0.010, 1, 0, 0, 0, 3.0, 3.0, 0.010], [-0.05, 0.03 * v, 0.012, 0, 0, 0, 1, 3.0, 3.0, 0.012]]
        rows += [[100.0 + k, 100.0 + k, 100.0 + k, 1, 0, 0, 0, 0.5, 0.5, 0.5] for k in range(91)]
        T.append(rows)
    return np.asarray(T, dtype=np.float32)


@pytest.mark.parametrize("which", ["graded", "equal_tops"])
def test_more_penetrating_boxes_than_tracked_per_foot(which):
    """A foot that penetrates MORE boxes than the per-foot candidate table of the kernels holds (kMaxPenQ = 4; never on the shipped / generated
    terrains, reachable through pgtt_set_terrain): the wave re-runs the narrow phase through the exact many-box pass (rank cut over all 4 * nbox
    pairs before a pair may enter the table, MJX's order when a full table drops an entry) and the ACTIVE set equals the oracle's on W like
    everywhere else - go2_mjx_feetonly.xml:14-15 (max_geom_pairs = 25, max_contact_points = 4) consumed by go2/base.py:153-171.  The
    PGTT_DBG_PEN_OVERFLOW bit of dbg_niter only says that the pass was taken."""
    terrain = stacked_slabs_terrain() if which == "graded" else equal_top_slabs_terrain()
    n = 128
    for lay in ("hex", "oct", "quad"):
        EXEC["layout"] = lay
        try:
            env, hb, cs, ms = make_pair("stairs", n, terrain)
            h64 = oracle.HostBuffers(n, with_variant=True); h64["variant"][...] = hb["variant"]
            env.reset(3); oracle.reset(cs, ms, terrain, hb, seed=3, nthreads=8)
            rng = np.random.default_rng(1)
            well_total = mism_flagged = mism_unflagged = flagged = total = deep_pairs = flag_mism = 0
            for k in range(12):
                sync_to_host(env, hb, h64)
                act = np.tanh(rng.normal(size=(n, 12)) * 0.3).astype(np.float32)
                env.step(torch.from_numpy(act).cuda())
                r64 = np.zeros(n)
                oracle.step(cs, ms, terrain, hb, act, seed=3, nthreads=8)
                oracle.step(cs, ms, terrain, h64, act, seed=3, nthreads=8, fp64=True, resid=r64)
                torch.cuda.synchronize()
                g = {kk: v.cpu().numpy() for kk, v in env.buffers.items()}
                assert all(np.isfinite(g[kk]).all() for kk in ("state", "frame", "obs_state", "obs_priv", "reward", "metrics"))
                assert np.array_equal(g["istate"], hb["istate"])
                assert np.abs(g["state"][:19] - hb["state"][:19]).max() < 0.5
                ef = per_env_errors(hb.arrays, h64)
                well = (r64 < 1e-6) & (ef["qpos"] < 1e-5) & (ef["qvel"] < 1e-3)
                ga, ha = active_sets(g["dbg_contact"], g["dbg_dist"]), active_sets(hb["dbg_contact"], hb["dbg_dist"])
                sm = np.array([a != b for a, b in zip(ga, ha)])
                fl = (g["dbg_niter"] & 0x10000) != 0
                assert ((g["dbg_niter"] & 0xFFFF) <= 5).all()
                mism_flagged += int((sm & well & fl).sum()); mism_unflagged += int((sm & well & ~fl).sum()); well_total += int(well.sum())
                fc_g, fc_h = g["frame"][abi.F_CONTACT:abi.F_CONTACT + 4], hb["frame"][abi.F_CONTACT:abi.F_CONTACT + 4]
                flag_mism += int(((fc_g != fc_h).any(0) & well).sum())
                flagged += int(fl.sum()); total += n
                deep_pairs += sum(1 for a in ha for (_, b) in a if b >= 0)
            print(which, lay, "env-steps", total, "took the many-box pass", flagged, "| in W", well_total, ": ACTIVE-set mismatches with the pass", mism_flagged,
                  ", without", mism_unflagged, "| contact-flag mismatches", flag_mism, "| oracle box contacts", deep_pairs)
            assert flagged > 0.5 * total, (lay, flagged, total)                     # the regime is reached (feet in the air do not overflow)
            assert deep_pairs > 3 * total                                            # the oracle keeps (nearly) four box contacts per env here
            assert well_total > 0.3 * total, (lay, well_total)
            assert mism_flagged + mism_unflagged <= 1 and flag_mism <= 1, (lay, mism_flagged, mism_unflagged, flag_mism, well_total)
            env.close()
        finally:
            EXEC["layout"] = None


def _quat_mul(a, b):
    w1, x1, y1, z1 = a; w2, x2, y2, z2 = b
    return [w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2]


def _tilt_quat(yaw_deg, tilt_deg, about_y):
    """yaw about z, then a pitch (about the box's y) or a roll (about its x): the free quaternion a terrain row may carry
    (go2/randomize.py:97-108 copies pos AND quat of every box; terrain_scene_mjx.xml:20-21)"""
    y, t = np.deg2rad(yaw_deg) / 2, np.deg2rad(tilt_deg) / 2
    qt = [np.cos(t), 0.0, np.sin(t), 0.0] if about_y else [np.cos(t), np.sin(t), 0.0, 0.0]
    return _quat_mul([np.cos(y), 0.0, 0.0, np.sin(y)], qt)


def ramp_terrain():
    """Boxes that are NOT yaw-only: a 4 x 3 field of ramp tiles, pitched or rolled by 5 .. 25 degrees, two thirds of them also yawed, each overlapping
    its neighbours by 5 - 10 cm, the low edge of every tile below the floor plane (so plane and box contacts coexist) and the high edge 5 - 20 cm above
    it.  The sphere-box narrow phase then works in a rotated box frame (face selection among tilted faces, edge contacts along the ridge lines where
    two tiles meet), the grid cull sees world AABBs that are larger than the boxes, and the scan hits tilted tops."""
    T = []
    for v in range(4):
        rows, k = [], 0
        for i in range(4):
            for j in range(3):
                tilt = 5.0 + 20.0 * ((k * 7 + 3 * v) % 12) / 11.0
                yaw = 0.0 if k % 3 == 0 else (35.0 * k + 10.0 * v) % 360.0
                q = _tilt_quat(yaw, tilt if (k + v) % 2 == 0 else -tilt, about_y=(k % 2 == 0))
                rows.append([(i - 1.5) * 0.70 + 0.03 * v, (j - 1.0) * 0.60, -0.02 + 0.01 * (k % 3), *q, 0.40, 0.35, 0.05])
                k += 1
        rows += [[100.0 + n, 100.0 + n, 100.0 + n, 1, 0, 0, 0, 0.5, 0.5, 0.5] for n in range(100 - len(rows))]
        T.append(rows)
    return np.asarray(T, dtype=np.float32)


def ramp_pile_terrain():
    """Nine slabs piled over the spawn area, every one yawed AND tilted (0.3 .. 1.5 degrees about alternating axes), their centres on a 0.15 m ring at
    the same height: half a metre out the nine top faces are 1 - 12 mm apart, so a standing foot (5 - 15 mm inside the highest one) is inside five to
    nine rotated boxes at once and the narrow phase runs through the exact many-box pass - on boxes whose frames are general rotations."""
    T = []
    for v in range(4):
        rows = []
        for k in range(9):
            r, phi = (0.0, 0.0) if k == 8 else (0.15, 2 * np.pi * k / 8 + 0.2 * v)
            q = _tilt_quat(40.0 * k + 15.0 * v, (0.3 + 0.15 * k) * (1 if k % 3 else -1), about_y=(k % 2 == 0))
            rows.append([r * np.cos(phi), r * np.sin(phi), 0.02, *q, 2.0, 1.8, 0.03])
        rows += [[100.0 + n, 100.0 + n, 100.0 + n, 1, 0, 0, 0, 0.5, 0.5, 0.5] for n in range(100 - len(rows))]
        T.append(rows)
    return np.asarray(T, dtype=np.float32)


def test_tilted_box_contact_parity(layout):
    """MJX collides a sphere with a box of ANY orientation, the terrain table carries a free quaternion per box (go2/randomize.py:97-108,
    go2/xmls/terrain_scene_mjx.xml:20-21) and pgtt_set_terrain accepts it - every other contact-parity terrain of this suite is yaw 0 / 90 / 180.
    Ramps through the full parity bar (state, ACTIVE contact set, flags, scan) in all three lane layouts."""
    terrain = ramp_terrain()
    mats = terrain[:, :12, 3:7]
    assert (np.abs(mats[..., 1]) + np.abs(mats[..., 2]) > 0.04).all()          # every placed box really is pitched or rolled
    st = run_parity("stairs", 192, terrain, steps=30, w_floor=0.55, cap_scale=2.0, med_tol=4e-6)
    assert st["box_contacts"] > 1500 and st["box_contacts"] > 0.25 * st["active_contacts"]
    assert st["well_set_mismatch"] <= 2 and st["well_flag_mismatch"] <= 1


def test_tilted_boxes_with_dr_autoreset_and_the_baseline_task():
    """the ramps once more with everything else switched on: full domain randomisation (per-box friction on tilted faces), AutoReset, and the baseline
    task's observation layout; then the two-kernel observe form on the same terrain"""
    terrain = ramp_terrain()
    run_parity("stairs", 128, terrain, steps=24, dr=True, autoreset=True, w_floor=0.55, cap_scale=2.0, med_tol=4e-6)
    run_parity("stairs", 96, terrain, steps=16, autoreset=True, method="baseline", w_floor=0.55, cap_scale=2.0, med_tol=4e-6)
    EXEC["observe_form"] = "split"
    try:
        run_parity("stairs", 96, terrain, steps=16, autoreset=True, w_floor=0.55, cap_scale=2.0, med_tol=4e-6)
    finally:
        EXEC["observe_form"] = None


def test_tilted_box_many_box_pass_parity(layout):
    """the exact many-box pass (more than four penetrating boxes per foot) on rotated boxes: ACTIVE set = the oracle's on W, in every layout"""
    terrain = ramp_pile_terrain()
    n = 128
    env, hb, cs, ms = make_pair("stairs", n, terrain)
    h64 = oracle.HostBuffers(n, with_variant=True); h64["variant"][...] = hb["variant"]
    env.reset(3); oracle.reset(cs, ms, terrain, hb, seed=3, nthreads=8)
    rng = np.random.default_rng(1)
    well_total = mism = flagged = total = deep_pairs = flag_mism = 0
    for k in range(12):
        sync_to_host(env, hb, h64)
        act = np.tanh(rng.normal(size=(n, 12)) * 0.3).astype(np.float32)
        env.step(torch.from_numpy(act).cuda())
        r64 = np.zeros(n)
        oracle.step(cs, ms, terrain, hb, act, seed=3, nthreads=8)
        oracle.step(cs, ms, terrain, h64, act, seed=3, nthreads=8, fp64=True, resid=r64)
        torch.cuda.synchronize()
        g = {kk: v.cpu().numpy() for kk, v in env.buffers.items()}
        assert all(np.isfinite(g[kk]).all() for kk in ("state", "frame", "obs_state", "obs_priv", "reward", "metrics", "scan_z"))
        assert np.array_equal(g["istate"], hb["istate"])
        ef = per_env_errors(hb.arrays, h64)
        eg = per_env_errors(g, hb)
        well = (r64 < 1e-6) & (ef["qpos"] < 1e-5) & (ef["qvel"] < 1e-3)
        ga, ha = active_sets(g["dbg_contact"], g["dbg_dist"]), active_sets(hb["dbg_contact"], hb["dbg_dist"])
        sm = np.array([a != b for a, b in zip(ga, ha)])
        fl = (g["dbg_niter"] & 0x10000) != 0
        mism += int((sm & well).sum()); well_total += int(well.sum()); flagged += int(fl.sum()); total += n
        fc_g, fc_h = g["frame"][abi.F_CONTACT:abi.F_CONTACT + 4], hb["frame"][abi.F_CONTACT:abi.F_CONTACT + 4]
        flag_mism += int(((fc_g != fc_h).any(0) & well).sum())
        deep_pairs += sum(1 for a in ha for (_, b) in a if b >= 0)
        assert (eg["qpos"][well] > 1e-4).sum() <= max(1, 0.01 * well.sum()), (k, eg["qpos"][well].max())
        assert (eg["scan"][well] > 1e-5).sum() <= 1          # a ray next to a slab's side face may land on the other side of it (a step of the scan, not an error)
    print(layout, "env-steps", total, "took the many-box pass", flagged, "| in W", well_total, ": ACTIVE-set mismatches", mism, "| flag mismatches", flag_mism, "| oracle box contacts", deep_pairs)
    assert flagged > 0.5 * total and deep_pairs > 2.5 * total and well_total > 0.25 * total          # measured: 73 % flagged, 3.35 box contacts per env-step, W = 49 %
    assert mism <= 1 and flag_mism <= 1
    env.close()


def test_variant_label_out_of_range_is_an_error_not_a_fault():
    """the boundary promises integer error codes, never a GPU fault: a terrain-variant label outside [0, T) makes pgtt_reset return PGTT_E_ARG before
    it writes anything, and a step taken with such a label anyway (labels edited after the reset) runs on the clamped variant - no out-of-bounds read"""
    from phase_guided_terrain_traversal_amd import native
    from phase_guided_terrain_traversal_amd.env import Joystick
    terrain = np.load(os.path.join(ASSETS, "terrains", "level4.npy"))
    n, T = 64, terrain.shape[0]
    for lay in ("hex", "oct", "quad"):
        good = np.random.default_rng(0).integers(0, T, n).astype(np.int32)
        env = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", variant=torch.from_numpy(good), layout=lay)
        env.reset(1)
        before = env.buffers["state"].clone()
        for bad_value in (T, -1, 2 ** 30):
            env.buffers["variant"][5] = bad_value
            with pytest.raises(native.PgttError, match="variant label"):
                env.reset(1)
            assert torch.equal(env.buffers["state"], before)                      # nothing was written
        # a MASKED reset is the form a caller may keep in its loop: after a check that passed it does not wait for the stream again (labels edited in
        # place since are clamped, like in the step) - until pgtt_bind / pgtt_set_terrain hand the library new labels, when the next reset of any kind checks
        env.buffers["variant"][5] = int(good[5]); env.reset(1)
        env.buffers["variant"][5] = T + 3
        m = torch.zeros(n, dtype=torch.uint8); m[7] = 1
        env.reset(1, mask=m)                                                      # no error: asynchronous, label clamped
        env._bind()
        with pytest.raises(native.PgttError, match="variant label"):
            env.reset(1, mask=m)
        env.buffers["variant"][5] = int(good[5]); env.reset(1, mask=m)
        # stepping with the bad labels in place: clamped to the last / first variant, bit-identical to an env that carries the clamped labels
        env.buffers["variant"][5] = 2 ** 30; env.buffers["variant"][6] = -7
        ref_lab = good.copy(); ref_lab[5] = T - 1; ref_lab[6] = 0
        ref = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", variant=torch.from_numpy(ref_lab), layout=lay)
        ref.reset(1)
        for k in ("state", "istate"):
            env.buffers[k].copy_(ref.buffers[k])
        act = torch.tanh(torch.randn(n, 12, generator=torch.Generator().manual_seed(3)) * 0.5).cuda()
        for _ in range(3):
            env.step(act); ref.step(act)
        torch.cuda.synchronize()
        assert torch.isfinite(env.buffers["state"]).all()
        assert torch.equal(env.buffers["state"][:55], ref.buffers["state"][:55]) and torch.equal(env.buffers["scan_z"], ref.buffers["scan_z"])
        env.close(); ref.close()
