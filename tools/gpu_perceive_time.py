"""Time of the student perception module next to what it replaces and to its neighbours on the step path, with the protocol of
DESIGN.md 14: 4096 envs, level4 with per-env variants from domain_randomize(seed=0), 64x48 images of the default camera, poses after 40 control
steps of small random actions; device events around 20 back-to-back calls after 5 warm-up calls, median [min, max] of 11 such windows.

    python tools/gpu_perceive_time.py [--out profiles/NAME.txt]

(i) pgtt_perceive (two launches); (ii) the torch fp32 ScanEstimator forward under no_grad plus the obs_out assembly as torch ops - what (i)
replaces, the yardstick; (iii) the camera tick; (iv) the env step (no camera, no student); (v) pgtt_perceive_recurrent, the default net with a GRU
memory of 128 values per env (a second StudentPerception on the same image and observation); (vi) the torch fp32
ScanEstimator.step + assembly that (v) replaces."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phase_guided_terrain_traversal_amd import configs, mjcf, perceive  # noqa: E402
from phase_guided_terrain_traversal_amd.env import Joystick  # noqa: E402
from phase_guided_terrain_traversal_amd.randomize import domain_randomize  # noqa: E402


def window_us(fn, calls=20, warm=5, windows=11):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        e.synchronize()
        out.append(1e3 * s.elapsed_time(e) / calls)
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    n = args.num_envs
    terrain = np.load(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "assets", "terrains", "level4.npy"))
    dr = domain_randomize(mjcf.load_model("stairs"), n, seed=0, terrain=terrain)
    kw = dict(params=torch.from_numpy(dr["params"]), variant=torch.from_numpy(dr["variant"]), box_friction=torch.from_numpy(dr["box_friction"]))
    torch.manual_seed(0)
    est = perceive.ScanEstimator().cuda()
    env = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", depth={}, student=est, **kw)
    plain = Joystick("stairs", configs.training_config(), num_envs=n, terrain=terrain, device="cuda:0", **kw)
    g = torch.Generator().manual_seed(1)
    for e in (env, plain):
        e.reset(0)
    for _ in range(40):
        act = (0.2 * torch.randn(n, 12, generator=g)).clamp(-1, 1).cuda()
        env.step(act); plain.step(act)
    torch.cuda.synchronize()
    sp, obs, depth = env.student, env.buffers["obs_state"], env.depth
    rest = perceive.ScanEstimator(perceive.config(memory=128)).cuda()
    rsp = perceive.StudentPerception(env, rest)

    @torch.no_grad()
    def torch_path():
        return est.assemble(obs, est(depth, obs))

    @torch.no_grad()
    def torch_step():
        e, m1 = rest.step(depth, obs, rsp.mem)
        return rest.assemble(obs, e), m1

    rows = [("(i)   pgtt_perceive, two launches", window_us(sp.tick)),
            ("(ii)  torch fp32 ScanEstimator forward + obs_out assembly", window_us(torch_path)),
            ("(iii) camera tick (force)", window_us(lambda: env.depth_camera.tick(force=True))),
            ("(iv)  env step, no camera, no student", window_us(lambda: plain.step(act))),
            ("(v)   pgtt_perceive_recurrent, memory 128, two launches", window_us(rsp.tick)),
            ("(vi)  torch fp32 ScanEstimator.step + obs_out assembly", window_us(torch_step))]
    with torch.no_grad():
        agree = float((torch_path() - sp.tick()).abs().max())
        want, m1 = torch_step()
        ragree = max(float((want - rsp.tick()).abs().max()), float((m1 - rsp.mem).abs().max()))
    lines = [f"{n} envs, level4, 64x48, default net ({sum(p.numel() for p in est.parameters())} parameters); us per call, median [min, max] of 11 windows of 20 calls",
             f"libpgtt_perceive build: {perceive.build_info()}"]
    lines += [f"{name:60s} {m:9.1f} [{lo:.1f}, {hi:.1f}]" for name, (m, lo, hi) in rows]
    lines.append(f"(ii) / (i) = {rows[1][1][0] / rows[0][1][0]:.2f};  max |torch - kernel| over obs_out = {agree:.2e}")
    lines.append(f"(v) / (i) = {rows[4][1][0] / rows[0][1][0]:.2f};  (vi) / (v) = {rows[5][1][0] / rows[4][1][0]:.2f};  "
                 f"max |torch - kernel| over obs_out and mem = {ragree:.2e}  ({sum(p.numel() for p in rest.parameters())} parameters)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    rsp.close(); env.close(); plain.close()


if __name__ == "__main__":
    main()
