"""The C-ABI library loads and exports every symbol include/pgtt.h and include/pgtt_train.h declare; struct layouts agree (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from phase_guided_terrain_traversal_amd import abi, configs, mjcf, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header="pgtt.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(pgtt_[a-z_0-9]+)\s*\(", text)) - {"pgtt_env"})


def test_header_symbols_exported():
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libpgtt.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  (load torch's HIP runtime first, see native.py)
    lib = C.CDLL(native.LIB_PATH)
    env_names, train_names = _declared(), _declared("pgtt_train.h")
    assert set(env_names) == set(native.EXPORTS)
    assert set(train_names) == set(native.TRAIN_EXPORTS) and not set(train_names) & set(env_names)      # trainer helpers stay out of the env ABI
    names = env_names + train_names
    for n in names:
        assert hasattr(lib, n), n
    assert lib.pgtt_sizeof_model() == C.sizeof(abi.PgttModel)
    assert lib.pgtt_sizeof_config() == C.sizeof(abi.PgttConfig)
    assert lib.pgtt_sizeof_buffers() == C.sizeof(abi.PgttBuffers)
    lib.pgtt_version.restype = C.c_char_p
    assert b"gfx950" in lib.pgtt_version()


def test_row_enums_match_header():
    text = open(os.path.join(ROOT, "include", "pgtt.h")).read()
    for name, val in re.findall(r"PGTT_([SIFP]_[A-Z_0-9]+)\s*=\s*(\d+)", text):
        assert getattr(abi, name) == int(val), name
    for name in ("NSTATE", "NISTATE", "NFRAME", "NPARAM"):
        assert getattr(abi, name) == int(re.search(rf"PGTT_{name}\s*=\s*(\d+)", text).group(1))
    for name in ("NQ", "NV", "NU", "NBODY", "MAX_BOX", "NCON", "NEFC", "NSCAN", "OBS", "PRIV", "NREW", "NMETRIC"):
        assert getattr(abi, name) == int(re.search(rf"#define PGTT_{name}\s+(\d+)", text).group(1))
    keys = re.search(r"enum \{\s*PGTT_R_TRACKING_LIN_VEL = 0,(.*?)\};", text, re.S).group(1)
    order = ["tracking_lin_vel"] + [k.strip()[len("PGTT_R_"):].lower() for k in keys.replace("\n", " ").split(",") if k.strip()]
    assert order == abi.REWARD_KEYS


def test_no_cpu_fallback_without_gpu():
    """On a box without a GPU the product must fail loudly, never route to the oracle."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libpgtt.so not built")
    L = native.lib()
    cs = abi.config_struct(configs.default_config()); ms = abi.model_struct(mjcf.load_model("flat_terrain"))
    h = C.c_void_p()
    rc = L.pgtt_create(C.byref(cs), C.byref(ms), 0, 64, C.byref(h))
    assert rc in (-4, -3), rc                              # PGTT_E_NODEVICE / PGTT_E_HIP
    assert b"no HIP device" in L.pgtt_last_error() or b"hip" in L.pgtt_last_error().lower()
    from phase_guided_terrain_traversal_amd.env import Joystick
    with pytest.raises(Exception):
        Joystick("flat_terrain", num_envs=8, device="cpu")


def test_create_refuses_what_the_kernels_cannot_compute():
    """argument checks run before the device is touched: values the kernels hold as compile-time shapes (two history samples, <= 4 box contacts per foot,
    the 4-row pyramid of condim 3) or need consistent (n_substeps, timestep) are a PGTT_E_ARG, never a silently different simulation"""
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libpgtt.so not built")
    L = native.lib()
    base_m = mjcf.load_model("stairs")
    h = C.c_void_p()

    def rc(cfg_over=None, model_over=None, n=64):
        c = abi.config_struct(dict(configs.training_config(), **(cfg_over or {})))
        if cfg_over and "n_substeps" in cfg_over:
            c.n_substeps = cfg_over["n_substeps"]
        m = abi.model_struct(dict(base_m, **(model_over or {})))
        return L.pgtt_create(C.byref(c), C.byref(m), 0, n, C.byref(h)), L.pgtt_last_error()
    for over, word in (({"history_len": 3}, b"history_len"), ({"history_update_steps": 0}, b"history_update_steps"), ({"episode_length": 0}, b"episode_length"),
                       ({"n_substeps": 3}, b"n_substeps"), ({"sim_dt": 0.004}, b"timestep")):
        r, msg = rc(cfg_over=over)
        assert r == -1 and word in msg, (over, r, msg)
    for over, word in (({"max_contact_points": 8}, b"max_contact_points"), ({"max_contact_points": -1}, b"max_contact_points"), ({"timestep": 0.002}, b"timestep"),
                       ({"box_margin": 0.002}, b"margin"), ({"foot_margin": 0.001, "foot_gap": 0.0005}, b"margin"), ({"floor_condim": 1, "foot_condim": 1}, b"condim"), ({"box_condim": 4}, b"condim"), ({"iterations": 0}, b"iteration")):
        r, msg = rc(model_over=over)
        assert r == -1 and word in msg, (over, r, msg)
    assert rc(n=0)[0] == -1 and rc(n=(1 << 22) + 1)[0] == -1
    r, msg = rc()                                           # the shipped values pass the checks (and then meet the device, or its absence)
    assert r in (0, -3, -4), (r, msg)
    if r == 0:
        L.pgtt_destroy(h)


def test_execution_options_come_through_the_abi_not_the_environment():
    """lane layout / observe form / test hooks are PgttConfig fields; the library reads no environment variable"""
    cfg = dict(configs.training_config(), lane_layout="oct", observe_form="split", test_hooks=True)
    c = abi.config_struct(cfg)
    assert (c.lane_layout, c.observe_form, c.test_hooks) == (2, 1, 1)
    c0 = abi.config_struct(configs.training_config())
    assert (c0.lane_layout, c0.observe_form, c0.test_hooks) == (0, 0, 0)
    text = open(os.path.join(ROOT, "include", "pgtt.h")).read()
    for name, val in (("AUTO", 0), ("QUAD", 1), ("OCT", 2), ("HEX", 4)):
        assert int(re.search(rf"PGTT_LAYOUT_{name}\s*=\s*(\d+)", text).group(1)) == val == abi.LAYOUTS[name.lower()]
    for f in os.listdir(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "csrc")):
        if f.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "csrc", f)).read(), f


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "phase_guided_terrain_traversal_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "from oracle" not in src and "import oracle" not in src and "liboracle" not in src, f


def test_model_struct_roundtrip():
    m = mjcf.load_model("stairs")
    s = abi.model_struct(m)
    assert np.allclose(np.ctypeslib.as_array(s.body_mass), m["body_mass"])
    assert list(s.act_dof) == [9, 10, 11, 6, 7, 8, 15, 16, 17, 12, 13, 14]
    assert s.iterations == 5 and s.ls_iterations == 5 and s.max_geom_pairs == 25 and s.max_contact_points == 4
    assert abs(s.timestep - 0.005) < 1e-9 and abs(s.impratio - 100) < 1e-6
    assert np.allclose(np.ctypeslib.as_array(s.act_bias)[0], [0, -40, -0.5])
    c = abi.config_struct(configs.training_config())
    assert c.n_substeps == 4 and abs(c.cmd_u_max[2] - 1.0) < 1e-7 and abs(c.gait_freq[1] - 3) < 1e-7
    assert abs(c.reward_scale[abi.REWARD_KEYS.index("feet_phase")] - 0.5) < 1e-7
    assert abs(c.reward_scale[abi.REWARD_KEYS.index("contact")] - 2.0) < 1e-7


def test_evaluation_config_has_the_reference_evaluators_command_range():
    """training/evaluate.py:127-129 evaluates on u_max = [0.4, 0.4, 0.7], gait_freq = [1, 3] - not on training's +-[0.6, 0.6, 1.0]"""
    for method in ("pgtt", "baseline"):
        c = configs.evaluation_config(method)
        assert c["command_config"]["u_max"] == [0.4, 0.4, 0.7] and c["command_config"]["u_min"] == [-0.4, -0.4, -0.7] and c["gait_freq"] == [1, 3]
        assert c["method"] == method and c["reward_config"] == configs.training_config(method)["reward_config"]
    assert configs.training_config()["command_config"]["u_max"] == [0.6, 0.6, 1.0]


def test_tools_and_entry_points_compile():
    """the GPU-side helper scripts cannot run here; at least they must be syntactically valid"""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = glob.glob(os.path.join(root, "tools", "*.py")) + [os.path.join(root, f) for f in ("bench.py", "train.py", "__graft_entry__.py")]
    assert len(files) > 10
    for f in files:
        compile(open(f).read(), f, "exec")


def test_source_hash_covers_the_physics_translation_unit_and_nothing_else(tmp_path):
    """srchash.py hashes what physics_kernel is built from: the project files its translation unit includes and the flags fragment.  An edit of
    the task kernels, the curriculum kernels or another rule of the Makefile leaves the hash alone; an edit of a physics header or of a flag changes it."""
    import shutil
    import subprocess
    from phase_guided_terrain_traversal_amd import srchash
    pkg = os.path.join(ROOT, "phase_guided_terrain_traversal_amd")
    csrc = os.path.join(pkg, "csrc")
    hashed = {os.path.realpath(f) for f in srchash.hashed_files()}
    assert os.path.realpath(os.path.join(csrc, "flags.mk")) in hashed
    assert native.source_sha256() == srchash.source_sha256()
    # on copies: what moves the hash and what does not
    cp = tmp_path / "phase_guided_terrain_traversal_amd"
    (cp / "csrc").mkdir(parents=True)
    (tmp_path / "include").mkdir()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h", ".mk")) or f == "Makefile":
            shutil.copy(os.path.join(csrc, f), cp / "csrc" / f)
    shutil.copy(os.path.join(ROOT, "include", "pgtt.h"), tmp_path / "include" / "pgtt.h")
    h0 = srchash.source_sha256(str(cp))
    assert h0 == srchash.source_sha256()

    def appended(name, text):
        p = cp / "csrc" / name
        old = p.read_text()
        p.write_text(old + text)
        h = srchash.source_sha256(str(cp))
        p.write_text(old)
        return h
    for name, text in (("pgtt_task.hip", "\nint pgtt_extra_statement;\n"), ("pgtt_curriculum.hip", "\nint pgtt_extra_statement;\n"), ("pgtt_api.hip", "\nint pgtt_extra_statement;\n"),
                       ("Makefile", "\nextra-rule:\n\t@true\n")):
        assert appended(name, text) == h0, name
    for name, text in (("pgtt_physics.hip.h", "\nint pgtt_extra_statement;\n"), ("pgtt_physics_quad.hip.h", "\nint pgtt_extra_statement;\n"), ("pgtt_common.hip.h", "\nint pgtt_extra_statement;\n"),
                       ("pgtt_physics_inst.hip", "\nint pgtt_extra_statement;\n"), ("flags.mk", "\nFLAGS += -O2\n")):
        assert appended(name, text) != h0, name
    assert appended("pgtt_physics_quad.hip.h", "\n// a comment\n") == h0 and appended("flags.mk", "\n# a comment\n") == h0


def test_source_hash_files_are_the_include_closure_of_the_physics_translation_unit():
    """the hashed files are exactly the project-local files the compiler reads for pgtt_physics_inst.hip, plus the flags fragment"""
    import shutil
    import subprocess
    from phase_guided_terrain_traversal_amd import srchash
    csrc = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "csrc")
    hashed = {os.path.realpath(f) for f in srchash.hashed_files()}
    if not (shutil.which("hipcc") and shutil.which("make")):
        pytest.skip("hipcc / make not on PATH: the include closure cannot be listed")
    flags = subprocess.run(["make", "-s", "flags-4_0_0_1"], cwd=csrc, check=True, capture_output=True, text=True).stdout.split()
    mm = subprocess.run(["hipcc"] + flags + ["--cuda-host-only", "-MM", "pgtt_physics_inst.hip"], cwd=csrc, check=True, capture_output=True, text=True).stdout
    deps = {os.path.realpath(os.path.join(csrc, t)) for t in mm.replace("\\\n", " ").split()[1:]}
    local = {d for d in deps if d.startswith(os.path.realpath(ROOT) + os.sep)}
    assert local | {os.path.realpath(os.path.join(csrc, "flags.mk"))} == hashed


# ---------------------------------------------------------------- the five side libraries (csrc/pgtt_side.mk)
SIDE = ("render", "depth", "perceive", "elevation", "learn")
RAYCAST = ("render", "depth")                              # the two over the shared ray-casting core


def _side_module(name):
    import importlib
    return importlib.import_module("phase_guided_terrain_traversal_amd." + name)


def _needs_side_lib(name):
    mod = _side_module(name)
    if not os.path.exists(mod.LIB_PATH):
        pytest.skip(f"libpgtt_{name}.so not built (run __graft_entry__.build())")
    return mod


@pytest.mark.parametrize("name", SIDE)
def test_side_hash_matches_the_built_library(name):
    """pgtt_<name>_build_info() carries srchash.side_sha256(name) of the sources as they are now, and the flavor of the shipped build"""
    from phase_guided_terrain_traversal_amd import srchash
    info = _needs_side_lib(name).build_info()
    assert info["src"] == srchash.side_sha256(name) and re.fullmatch(r"[0-9a-f]{64}", info["src"])
    assert info["flavor"] == "product"


@pytest.mark.parametrize("name", SIDE)
def test_side_hash_files_are_the_include_closure_of_the_unit(name):
    """SIDE_SOURCES[name] is exactly the set of project files csrc/pgtt_<name>.hip includes, transitively (quoted includes, followed by hand)"""
    from phase_guided_terrain_traversal_amd import srchash
    csrc = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "csrc")
    seen, todo = set(), [os.path.join(csrc, f"pgtt_{name}.hip")]
    while todo:
        f = os.path.realpath(todo.pop())
        if f in seen:
            continue
        seen.add(f)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), re.M):
            todo.append(os.path.join(os.path.dirname(f), inc))
    assert all(f.startswith(os.path.realpath(ROOT) + os.sep) for f in seen)
    assert seen == {os.path.realpath(f) for f in srchash.side_files(name)}
    in_csrc, in_include = srchash.SIDE_SOURCES[name]
    assert {os.path.basename(f) for f in seen} == set(in_csrc) | set(in_include)
    assert "pgtt_common.hip.h" not in in_csrc                  # the physics hash and the side hashes share include/pgtt.h only
    assert "pgtt_side_host.h" in in_csrc                       # every side library stands on the one host prelude
    # the ray-casting core - device algebra, scene tables, the renderer's public header - belongs to the two ray casters alone
    for f in ("pgtt_raycast.hip.h", "pgtt_raycast_host.h", "pgtt_render.h"):
        assert (f in in_csrc + in_include) == (name in RAYCAST), f


@pytest.mark.parametrize("name", SIDE)
def test_side_make_prerequisites_are_the_hashed_files(name):
    """csrc/pgtt_side.mk takes a unit's prerequisites from `srchash.py --files <name>`, which prints side_files(name); it names no header itself"""
    import subprocess
    import sys
    from phase_guided_terrain_traversal_amd import srchash
    out = subprocess.run([sys.executable, os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "srchash.py"), "--files", name],
                         check=True, capture_output=True, text=True).stdout
    assert out.split("\n") == srchash.side_files(name) + [""]
    mk = open(os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "csrc", "pgtt_side.mk")).read()
    rules = "\n".join(ln.split("#", 1)[0] for ln in mk.splitlines())
    assert "srchash.py --files" in rules and not re.search(r"\.h\b", rules)


@pytest.mark.parametrize("name", SIDE)
def test_side_header_functions_are_the_modules_exports(name):
    """every function include/pgtt_<name>.h declares is in the module's EXPORTS and the other way round; no name is the env ABI's or another
    side library's"""
    mod = _side_module(name)
    text = open(os.path.join(ROOT, "include", f"pgtt_{name}.h")).read()
    assert sorted(set(re.findall(rf"\b(pgtt_{name}[a-z_0-9]*)\s*\(", text))) == sorted(mod.EXPORTS)
    assert len(set(mod.EXPORTS)) == len(mod.EXPORTS) and all(fn == f"pgtt_{name}" or fn.startswith(f"pgtt_{name}_") for fn in mod.EXPORTS)
    assert not set(mod.EXPORTS) & set(native.EXPORTS + native.TRAIN_EXPORTS)
    for other in SIDE:
        assert other == name or not set(mod.EXPORTS) & set(_side_module(other).EXPORTS), other


@pytest.mark.parametrize("name", SIDE)
def test_side_library_exports_exactly_the_modules_exports(name):
    """nm -D: the library defines the module's EXPORTS and no other pgtt name (nothing of libpgtt.so, nothing of another side library)"""
    import subprocess
    mod = _needs_side_lib(name)
    out = subprocess.run(["nm", "-D", "--defined-only", mod.LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("nm not available")
    names = {ln.split()[-1] for ln in out.stdout.splitlines() if " T " in ln and ln.split()[-1].startswith("pgtt")}
    assert names == set(mod.EXPORTS)
    L = mod.lib()
    for fn in mod.EXPORTS:
        assert hasattr(L, fn), fn


def test_side_hashes_react_to_the_right_edits(tmp_path):
    """on a copied tree: a statement in the host prelude moves all five side hashes and not the physics hash, one in the ray-casting core moves
    render and depth only, one in a unit or in its public header moves that library's hash alone (pgtt_render.h: depth's too), one in the physics
    kernels' header moves the physics hash only, a comment moves nothing"""
    import shutil
    from phase_guided_terrain_traversal_amd import srchash
    csrc = os.path.join(ROOT, "phase_guided_terrain_traversal_amd", "csrc")
    cp = tmp_path / "phase_guided_terrain_traversal_amd"
    (cp / "csrc").mkdir(parents=True)
    (tmp_path / "include").mkdir()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h", ".mk")) or f == "Makefile":
            shutil.copy(os.path.join(csrc, f), cp / "csrc" / f)
    for f in os.listdir(os.path.join(ROOT, "include")):
        shutil.copy(os.path.join(ROOT, "include", f), tmp_path / "include" / f)

    def hashes():
        return {**{n: srchash.side_sha256(n, str(cp)) for n in SIDE}, "physics": srchash.source_sha256(str(cp))}
    h0 = hashes()
    assert h0 == {**{n: srchash.side_sha256(n) for n in SIDE}, "physics": srchash.source_sha256()} and len(set(h0.values())) == len(SIDE) + 1

    def moved(path, text="\nint pgtt_extra_statement;\n"):
        """the hashes that differ from h0 with `text` appended to `path`"""
        old = path.read_text()
        path.write_text(old + text)
        h = hashes()
        path.write_text(old)
        return {k for k in h if h[k] != h0[k]}
    assert moved(cp / "csrc" / "pgtt_side_host.h") == set(SIDE)
    for core in ("pgtt_raycast.hip.h", "pgtt_raycast_host.h"):
        assert moved(cp / "csrc" / core) == set(RAYCAST), core
    for name in SIDE:
        assert moved(cp / "csrc" / f"pgtt_{name}.hip") == {name}, name
        assert moved(tmp_path / "include" / f"pgtt_{name}.h") == ({name} if name != "render" else set(RAYCAST)), name
    assert moved(cp / "csrc" / "pgtt_common.hip.h") == {"physics"}    # the physics kernels' header is no part of a side library
    for f in ("pgtt_side_host.h", "pgtt_raycast.hip.h", "pgtt_raycast_host.h", "pgtt_common.hip.h") + tuple(f"pgtt_{n}.hip" for n in SIDE):
        assert moved(cp / "csrc" / f, "\n// a comment\n") == set(), f


def test_side_libraries_raise_their_own_error_class():
    errors = {}
    for name in SIDE:
        mod = _needs_side_lib(name)
        errors[name] = getattr(mod, name.capitalize() + "Error")
        mod.check(0)
        with pytest.raises(errors[name], match=f"libpgtt_{name} error 1"):
            mod.check(1)
    for a in SIDE:
        for b in SIDE:
            assert a == b or not issubclass(errors[a], errors[b]), (a, b)
