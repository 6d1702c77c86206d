"""The depth camera without a GPU: the fp64 reference (tests/depth_reference.py) against closed forms, the ctypes mirrors against a compile
of include/pgtt_depth.h with the host compiler, and Joystick(depth=None) leaving libpgtt_depth.so alone."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_reference as ref  # noqa: E402

from phase_guided_terrain_traversal_amd import depth, mjcf, native  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _level_camera(h):
    return np.array([0.0, 0.0, h]), np.array([1.0, 0.0, 0.0]), np.array([0.0, -1.0, 0.0]), np.array([0.0, 0.0, 1.0])


def test_reference_level_camera_over_a_flat_floor():
    """a level camera at height h: the ray fwd + u right + v up meets z = 0 where its axis component is h / -v; rows with v >= 0 see nothing"""
    W, H, fovy, h, near, far = 20, 13, 70.0, 0.4, 0.1, 3.0
    img = ref.depth_image(_level_camera(h), fovy, W, H, near, far)
    v = (1 - 2 * (np.arange(H) + 0.5) / H) * np.tan(np.radians(fovy) / 2)
    with np.errstate(divide="ignore"):
        expect = np.where(v < 0, np.clip(h / np.where(v < 0, -v, 1.0), near, far), far)
    assert np.abs(img["depth"] - expect[:, None]).max() < 1e-12
    assert (img["id"][v >= 0] == ref.ID_MISS).all() and (img["id"][v < 0] == ref.ID_PLANE).all()
    # H is odd: the middle row looks exactly along the horizon, and only there does a shift of the ray change what is seen
    assert (expect < far).any() and (expect == far).any() and not img["ambiguous"][v != 0].any() and img["ambiguous"][v == 0].all()


def test_reference_single_box_straight_ahead():
    """an axis-aligned box centred on the optical axis: every ray through its front face reads the face's distance D - hx"""
    W, H, fovy, h, near, far = 32, 24, 60.0, 1.0, 0.1, 5.0
    D, half = 2.0, np.array([0.25, 0.4, 0.3])
    box = dict(c=np.array([D, 0.0, h]), A=np.eye(3), h=half)
    img = ref.depth_image(_level_camera(h), fovy, W, H, near, far, boxes=[box])
    th = np.tan(np.radians(fovy) / 2)
    u = ((2 * (np.arange(W) + 0.5) / W - 1) * th * W / H)[None, :]
    v = ((1 - 2 * (np.arange(H) + 0.5) / H) * th)[:, None]
    front = D - half[0]
    on_face = (np.abs(u * front) < half[1]) & (np.abs(v * front) < half[2])
    assert on_face.sum() > 20
    assert np.abs(img["depth"][on_face] - front).max() < 1e-12 and (img["id"][on_face] == ref.ID_BOX).all()
    # beside the box: the floor below the horizon (h / -v, beyond the box's far side only where it is not hidden), nothing above it
    clear = (np.abs(u * (D + half[0])) > half[1] + 1e-9) & (np.abs(u * front) > half[1] + 1e-9)
    floor = clear & (v < 0)
    assert np.abs(img["depth"][floor] - np.clip(h / -np.broadcast_to(v, (H, W))[floor], near, far)).max() < 1e-12
    assert (img["depth"][clear & (v > 0)] == far).all()
    # a camera inside the box does not see it
    inside = ref.depth_image((box["c"], *_level_camera(h)[1:]), fovy, W, H, near, far, boxes=[box])
    assert (inside["id"] != ref.ID_BOX).all()


def test_reference_sphere_capsule_and_pitch():
    o = np.zeros(3)
    d = np.array([[1.0, 0.0, 0.0]])
    assert abs(ref.hit_sphere(o, d, np.array([2.0, 0.0, 0.0]), 0.5)[0] - 1.5) < 1e-12
    assert abs(ref.hit_capsule(o, d, np.array([2.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), 0.25, 0.5)[0] - 1.75) < 1e-12
    cap = ref.hit_capsule(o, d, np.array([2.0, 0.0, 0.6]), np.array([0.0, 0.0, 1.0]), 0.25, 0.5)[0]                          # the lower end cap
    assert abs(cap - (2.0 - np.sqrt(0.25 ** 2 - 0.1 ** 2))) < 1e-12
    assert np.isinf(ref.hit_sphere(o, d, np.array([-2.0, 0.0, 0.0]), 0.5)[0])
    R = ref.qmat(ref.pitch_quat(30.0))
    assert np.allclose(R[:, 0], [np.cos(np.radians(30)), 0, -np.sin(np.radians(30))])
    assert np.allclose(depth.pitch_quat(30.0), ref.pitch_quat(30.0))


def test_reference_philox_matches_the_known_answer_and_numpy():
    """Random123's known-answer vector for philox4x32-10, and the uniforms' form (top 24 bits)"""
    out = ref.philox4x32_10((0xa4093822, 0x299f31d0), np.array([[0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], np.uint32))
    assert [int(x) for x in out[0]] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    u = ref.noise_uniforms(7, 3, 11, 50)
    assert u.shape == (50, 3) and (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2 ** 24, np.round(u * 2 ** 24))
    assert not np.array_equal(u, ref.noise_uniforms(7, 3, 12, 50)) and not np.array_equal(u, ref.noise_uniforms(7, 4, 11, 50))
    img = np.full((5, 10), 1.0)
    noisy, dropped = ref.apply_noise(img, 0.1, 3.0, 0.02, 0.1, 7, 3, 11)
    assert (noisy[dropped] == 3.0).all() and np.abs(noisy[~dropped] - 1.0).max() < 0.2


def test_mount_follows_the_full_base_orientation():
    """the base's roll and pitch enter the camera basis (what the renderer's cameras cannot express)"""
    m = mjcf.load_model("flat_terrain")
    qpos = np.array(m["key_qpos"], float)
    roll = 0.3
    qpos[3:7] = [np.cos(roll / 2), np.sin(roll / 2), 0, 0]
    xpos, xquat = ref.body_poses(m, qpos)
    pos, fwd, right, up = ref.camera_basis(xpos, xquat, 0, (0.3, 0.0, 0.05), ref.pitch_quat(0.0))
    assert np.allclose(fwd, [1, 0, 0]) and np.allclose(up, [0, -np.sin(roll), np.cos(roll)]) and np.allclose(right, np.cross(fwd, up))
    assert np.allclose(pos, qpos[:3] + ref.qmat(qpos[3:7]) @ [0.3, 0.0, 0.05])


def test_struct_layout_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler (the oracle's build needs one too): the layout of pgtt_depth.h cannot be checked"
    fields = {"PgttDepthConfig": [n for n, _ in depth.PgttDepthConfig._fields_], "PgttDepthBuffers": [n for n, _ in depth.PgttDepthBuffers._fields_]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pgtt_depth.h"', 'int main(void) {']
    for s, names in fields.items():
        lines.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s}.{n} %zu\\n", offsetof({s}, {n}));' for n in names]
    lines += ['  printf("RS %d MAXDIM %d\\n", PGTT_RS_DEPTH, PGTT_DEPTH_MAX_DIM);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()[:-1])
    for s, cls in (("PgttDepthConfig", depth.PgttDepthConfig), ("PgttDepthBuffers", depth.PgttDepthBuffers)):
        assert int(got[s]) == C.sizeof(cls)
        for n in fields[s]:
            assert int(got[f"{s}.{n}"]) == getattr(cls, n).offset, (s, n)
    last = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1].split()
    assert int(last[1]) == depth.RS_DEPTH >= 32 and int(last[3]) == depth.MAX_DIM


# ---------------------------------------------------------------- the host side of the library
needs_lib = pytest.mark.skipif(not os.path.exists(depth.LIB_PATH), reason="libpgtt_depth.so not built (run __graft_entry__.build())")
GOOD = dict(width=24, height=18, fovy=58.0, near=0.1, far=3.0, mount_body=0, mount_pos=(0.30, 0.0, 0.05), mount_quat=(1.0, 0.0, 0.0, 0.0), every=1)
# one bad value of every field the camera's config has in common with the LiDAR's (the checks are stated once, csrc/pgtt_sensor.hip.h), in the
# order of the checks, and the words libpgtt_depth.so had for it before they were: byte for byte, behind the entry point's name
SHARED_REFUSALS = [(dict(near=0.0), "need 0 < near < far, finite"), (dict(far=float("inf")), "need 0 < near < far, finite"),
                   (dict(mount_body=13), "mount_body outside [0, PGTT_NBODY)"), (dict(every=0), "every must be >= 1"),
                   (dict(see_robot=2), "see_robot must be 0 or 1"), (dict(sigma=-0.1), "noise_sigma must be >= 0"),
                   (dict(sigma=float("inf")), "noise_sigma must be >= 0"), (dict(dropout=1.0), "dropout must be in [0, 1)"),
                   (dict(mount_quat=(0.0, 0.0, 0.0, 0.0)), "mount_quat must be a non-zero quaternion"),
                   (dict(mount_pos=(0.0, float("nan"), 0.0)), "mount_pos must be finite")]


@needs_lib
def test_create_refusal_texts():
    """pgtt_depth_create refuses a config before it asks for a device: its exact message for each shared field, and for the camera's own
    checks, which come first: a config that is bad in a shared field AND has width = 0 is refused for the width"""
    from phase_guided_terrain_traversal_amd import abi
    L = depth.lib()
    ms = abi.model_struct(mjcf.load_model("flat_terrain"))

    def message(see_robot=True, **kw):
        cfg = depth.config_struct(**dict(GOOD, **kw))
        cfg.see_robot = int(see_robot)                                            # config_struct makes it 0 or 1
        h = C.c_void_p(1)
        assert L.pgtt_depth_create(C.byref(ms), C.byref(cfg), None, 0, 0, 1, C.byref(h)) == -1, kw
        assert not h                                                              # a refusal leaves no handle
        return L.pgtt_depth_last_error().decode()

    for kw, text in SHARED_REFUSALS:
        assert message(**kw) == "pgtt_depth_create: " + text, kw
        assert message(width=0, **kw) == "pgtt_depth_create: width and height must be in [1, PGTT_DEPTH_MAX_DIM]", kw
        assert message(fovy=180.0, **kw) == "pgtt_depth_create: fovy must be in (0, 180) degrees", kw
    assert message(near=0.0, every=0, mount_pos=(float("inf"), 0.0, 0.0)) == "pgtt_depth_create: need 0 < near < far, finite"
    assert message(every=0, mount_pos=(float("inf"), 0.0, 0.0)) == "pgtt_depth_create: every must be >= 1"


def test_settings_take_one_orientation():
    """the defaults carry a pitch; an override that gives mount_quat must not collide with it (DepthCamera refuses both)"""
    assert depth.settings()["pitch_deg"] == depth.DEFAULTS["pitch_deg"] and depth.settings().get("mount_quat") is None
    kw = depth.settings(dict(mount_body=2, mount_quat=(1.0, 0.0, 0.0, 0.0), width=8))
    assert "pitch_deg" not in kw and kw["mount_quat"] == (1.0, 0.0, 0.0, 0.0) and kw["width"] == 8 and kw["height"] == depth.DEFAULTS["height"]
    assert depth.settings(dict(pitch_deg=10.0))["pitch_deg"] == 10.0
    both = depth.settings(dict(pitch_deg=10.0, mount_quat=(1.0, 0.0, 0.0, 0.0)))
    assert both["pitch_deg"] == 10.0 and both["mount_quat"] is not None          # said twice on purpose: left for DepthCamera to refuse


def test_joystick_without_depth_never_imports_the_module():
    """in a fresh interpreter, importing the package, env.py and constructing Joystick(depth=None) leaves depth.py, and the loader it shares
    with render.py (_sidelib.py), unimported.  Without a GPU the constructor
    stops at pgtt_create, before the place where depth=... is looked at; tests/test_gpu_depth.py::test_the_env_is_untouched repeats the check
    where the constructor runs to its end."""
    code = ("import sys\n"
            "import phase_guided_terrain_traversal_amd\n"
            "name, shared = 'phase_guided_terrain_traversal_amd.depth', 'phase_guided_terrain_traversal_amd._sidelib'\n"
            "assert name not in sys.modules and shared not in sys.modules, 'the package imports depth.py or _sidelib.py'\n"
            "from phase_guided_terrain_traversal_amd import env, native\n"
            "assert name not in sys.modules, 'env.py imports depth.py'\n"
            "assert shared not in sys.modules, 'env.py imports _sidelib.py'\n"
            "try:\n"
            "    e = env.Joystick('flat_terrain', num_envs=2, device='cuda:0')\n"
            "    assert e.depth is None and e.depth_camera is None\n"
            "    e.reset(0); e.close()\n"
            "except native.PgttError:\n"
            "    pass\n"
            "assert name not in sys.modules, 'Joystick(depth=None) imported depth.py'\n"
            "assert shared not in sys.modules, 'Joystick(depth=None) imported _sidelib.py'\n"
            "print('clean')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("clean"), out.stderr[-2000:]


def test_video_tile_resize_is_nearest_neighbour():
    """evaluate.py --video_depth scales the sensor's image to the video tile (whose default, 320x240, is beyond the sensor's 256-pixel cap)"""
    import torch
    import evaluate
    a = torch.arange(2 * 3 * 4).reshape(2, 3, 4)
    assert torch.equal(evaluate.resize_nearest(a, 3, 4), a)
    up = evaluate.resize_nearest(a, 6, 8)
    assert up.shape == (2, 6, 8) and torch.equal(up[:, ::2, ::2], a) and torch.equal(up[:, 1::2, 1::2], a)
    big = evaluate.resize_nearest(torch.arange(48 * 64).reshape(1, 48, 64), 240, 320)
    assert big.shape == (1, 240, 320) and torch.equal(big[0, 2::5, 2::5], torch.arange(48 * 64).reshape(48, 64))
    down = evaluate.resize_nearest(a, 1, 2)
    assert down.tolist() == [[[5, 7]], [[17, 19]]]
    args = evaluate.make_parser().parse_args(["--video", "x.gif", "--video_depth"])
    w, h = (int(x) for x in args.video_size.lower().split("x"))
    assert max(w, h) > depth.MAX_DIM >= max(depth.DEFAULTS["width"], depth.DEFAULTS["height"])      # why the sensor keeps its own resolution
