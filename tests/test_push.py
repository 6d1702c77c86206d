"""External torso wrench and random pushes, the parts that need no GPU: the ABI mirrors (include/pgtt.h PgttConfig.push_*, PgttBuffers.xfrc /
push_state, PGTT_PU_* rows, PGTT_RS_PUSH_* streams), the config forms (Joystick(push=...), Playground's pert_config), the --push_* command line
and pgtt_create's refusal of bad kick ranges (checked before any device is touched)."""
import argparse
import ctypes as C
import os
import re

import pytest

from phase_guided_terrain_traversal_amd import abi, configs, mjcf, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "pgtt.h")).read()


def _struct_body(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    return re.sub(r"/\*.*?\*/", "", body, flags=re.S)


def test_new_fields_are_appended_and_mirrored():
    """every existing offset stays put: the push fields are the last ones of PgttConfig, xfrc / push_state the last ones of PgttBuffers"""
    cfg = re.findall(r"\b([a-z_0-9]+)(?:\[\d\])?;", _struct_body("PgttConfig"))
    assert cfg[-5:] == ["test_hooks", "push_enable", "push_wait_s", "push_duration_s", "push_velocity"]
    assert [n for n, _ in abi.PgttConfig._fields_][-5:] == cfg[-5:]
    assert abi.PgttConfig.push_enable.offset == abi.PgttConfig.test_hooks.offset + 4
    assert C.sizeof(abi.PgttConfig) == abi.PgttConfig.push_velocity.offset + 8
    buf = re.findall(r"\*\s*([a-z_0-9]+);", _struct_body("PgttBuffers"))
    assert buf[-3:] == ["interval_sums", "xfrc", "push_state"]
    assert [n for n, _ in abi.PgttBuffers._fields_] == buf
    assert abi.PgttBuffers.xfrc.offset == abi.PgttBuffers.interval_sums.offset + 8


def test_push_rows_and_streams_match_header():
    for name, val in re.findall(r"PGTT_(PU_[A-Z_]+)\s*=\s*(\d+)", HEADER):
        assert getattr(abi, name) == int(val), name
    assert abi.NPUSH == int(re.search(r"PGTT_NPUSH\s*=\s*(\d+)", HEADER).group(1))
    assert abi.RS_PUSH_WAIT == int(re.search(r"PGTT_RS_PUSH_WAIT\s*=\s*(\d+)", HEADER).group(1))
    assert abi.RS_PUSH_KICK == int(re.search(r"PGTT_RS_PUSH_KICK\s*=\s*(\d+)", HEADER).group(1))
    used = [int(v) for v in re.findall(r"PGTT_RS_[A-Z_]+\s*=\s*(\d+)", HEADER)]
    assert len(used) == len(set(used))                    # no existing draw changes: the push streams are new ids
    assert "pgtt_push" in native.EXPORTS and re.search(r"\bint pgtt_push\(pgtt_handle h, void\* stream\);", HEADER)


def test_config_struct_push_forms():
    base = configs.training_config()
    s = abi.config_struct(base)
    assert s.push_enable == 0 and list(s.push_wait_s) == [0, 0] and list(s.push_velocity) == [0, 0]
    assert abi.push_ranges(base) is None
    s = abi.config_struct(dict(base, push=dict(wait=(1, 3), duration=(0.05, 0.2), velocity=(0, 1.5))))
    assert s.push_enable == 1
    assert list(s.push_wait_s) == [1.0, 3.0] and list(s.push_velocity) == [0.0, 1.5]
    assert list(s.push_duration_s) == pytest.approx([0.05, 0.2])
    # MuJoCo Playground's spelling (go2 joystick pert_config)
    pc = dict(enable=True, velocity_kick=[0.0, 3.0], kick_durations=[0.05, 0.2], kick_wait_times=[1.0, 3.0])
    s2 = abi.config_struct(dict(base, pert_config=pc))
    assert s2.push_enable == 1 and list(s2.push_velocity) == [0.0, 3.0] and list(s2.push_wait_s) == [1.0, 3.0]
    assert abi.config_struct(dict(base, pert_config=dict(pc, enable=False))).push_enable == 0
    with pytest.raises(ValueError):
        abi.push_ranges(dict(base, push=dict(wait=(1, 3))))


def test_push_command_line():
    ap = argparse.ArgumentParser()
    configs.add_push_args(ap)
    assert configs.push_from_args(ap.parse_args([])) is None
    p = configs.push_from_args(ap.parse_args(["--push_velocity", "0,1.5"]))
    assert p == {"wait": (1.0, 3.0), "duration": (0.05, 0.2), "velocity": (0.0, 1.5)}
    p = configs.push_from_args(ap.parse_args(["--push_wait", "0.5,1", "--push_duration", "0.1,0.1", "--push_velocity", "1,2"]))
    assert p == {"wait": (0.5, 1.0), "duration": (0.1, 0.1), "velocity": (1.0, 2.0)}
    with pytest.raises(ValueError):
        configs.push_from_args(ap.parse_args(["--push_velocity", "1"]))
    # both scripts take the flags
    import evaluate
    a = evaluate.make_parser().parse_args(["--push_velocity", "0,1.5"])
    assert configs.push_from_args(a)["velocity"] == (0.0, 1.5)
    src = open(os.path.join(ROOT, "train.py")).read()
    assert "configs.add_push_args(ap)" in src and "configs.push_from_args(args)" in src


@pytest.mark.parametrize("over", [
    dict(wait=(3, 1)), dict(duration=(0.2, 0.05)), dict(velocity=(-1, 1)), dict(wait=(-0.5, 1)), dict(duration=(0.01, 0.2)),
    dict(velocity=(0, float("inf"))), dict(enable=2)])
def test_create_refuses_bad_push_ranges(over):
    """PGTT_E_ARG before anything touches a device (so also on a box without one): lo > hi, negative values, a duration under one ctrl_dt"""
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libpgtt.so not built")
    L = native.lib()
    push = dict(wait=(1, 3), duration=(0.05, 0.2), velocity=(0, 1.5))
    enable = over.pop("enable", 1)
    push.update(over)
    cs = abi.config_struct(dict(configs.training_config(), push=push))
    cs.push_enable = enable
    ms = abi.model_struct(mjcf.load_model("flat_terrain"))
    h = C.c_void_p()
    assert L.pgtt_create(C.byref(cs), C.byref(ms), 0, 64, C.byref(h)) == -1
    assert b"push" in L.pgtt_last_error()
