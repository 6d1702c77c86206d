"""The host side of the odometry drift (include/pgtt_elevation.h): the struct's layout and size, the ranges pgtt_elevation_check_odometry holds,
elevation.odometry_settings, and the --odometry_drift flag of evaluate.py.  No GPU."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import evaluate  # noqa: E402
from phase_guided_terrain_traversal_amd import elevation  # noqa: E402

needs_lib = pytest.mark.skipif(not os.path.exists(elevation.LIB_PATH), reason="libpgtt_elevation.so not built (run __graft_entry__.build())")
NEW = ("pgtt_elevation_check_odometry", "pgtt_elevation_bind_odometry", "pgtt_elevation_odometry", "pgtt_elevation_sizeof_odometry")


def test_struct_layout_and_defaults_without_the_library():
    assert C.sizeof(elevation.PgttElevationOdometry) == 104 and elevation.ODO_WORDS == 12 and elevation.RS_ODOMETRY == 34
    assert elevation.ODOMETRY_DEFAULTS == dict(sigma_xy=0.02, sigma_z=0.01, sigma_yaw=0.01, yaw_bias=0.005, scale=0.02, seed=0)
    o = elevation.odometry_struct(0.02, **elevation.ODOMETRY_DEFAULTS, env_id_offset=2 ** 31 + 5)
    assert o.state is None and o.points is None and o.P == 0 and o.env_id_offset == 2 ** 31 + 5 and abs(o.sigma_xy - 0.02) < 1e-8
    assert elevation.odometry_struct(0.02, seed=-1).seed == 2 ** 64 - 1
    for name in NEW:
        assert name in elevation.EXPORTS


def test_header_states_the_constants():
    text = open(os.path.join(ROOT, "include", "pgtt_elevation.h")).read()
    assert "#define PGTT_RS_ODOMETRY 34" in text and "#define PGTT_ELEVATION_ODO_WORDS 12" in text


def test_odometry_settings():
    assert elevation.odometry_settings(None) is None and elevation.odometry_settings(False) is None
    assert elevation.odometry_settings(True) == elevation.ODOMETRY_DEFAULTS and elevation.odometry_settings(True) is not elevation.ODOMETRY_DEFAULTS
    assert elevation.odometry_settings(dict(sigma_yaw=0.0, seed=4)) == dict(elevation.ODOMETRY_DEFAULTS, sigma_yaw=0.0, seed=4)
    with pytest.raises(ValueError, match="unknown setting"):
        elevation.odometry_settings(dict(sigma=0.1))
    with pytest.raises(ValueError, match="unknown setting"):
        elevation.odometry_settings(dict(dt=0.02))                       # dt is the env's control step, not a setting
    for bad in (3, 0.5, "yes", (0.02, 0.01)):
        with pytest.raises(ValueError, match="True or a dict"):
            elevation.odometry_settings(bad)
    assert "odometry" not in elevation.settings(True) and elevation.settings(dict(odometry=True))["odometry"] is True


@needs_lib
def test_sizeof_and_null_arguments():
    L = elevation.lib()
    assert L.pgtt_elevation_sizeof_odometry() == C.sizeof(elevation.PgttElevationOdometry)
    for name in NEW:
        assert hasattr(L, name)
    assert L.pgtt_elevation_bind_odometry(None, C.byref(elevation.odometry_struct(0.02))) == -1 and L.pgtt_elevation_last_error()
    assert L.pgtt_elevation_odometry(None, None, 0, 0, None) == -1 and L.pgtt_elevation_last_error()


@needs_lib
def test_check_odometry_at_every_range_edge():
    L = elevation.lib()
    good = dict(dt=0.02, sigma_xy=0.02, sigma_z=0.01, sigma_yaw=0.01, yaw_bias=0.005, scale=0.02)
    check = lambda **kw: L.pgtt_elevation_check_odometry(C.byref(elevation.odometry_struct(**dict(good, **kw))))
    assert check() == 0
    for kw in (dict(sigma_xy=0.0), dict(sigma_z=0.0), dict(sigma_yaw=0.0), dict(yaw_bias=0.0), dict(scale=0.0), dict(scale=0.99999),
               dict(dt=1e-6), dict(sigma_xy=0.0, sigma_z=0.0, sigma_yaw=0.0, yaw_bias=0.0, scale=0.0)):
        assert check(**kw) == 0, kw
    nan, inf = float("nan"), float("inf")
    bad = {"dt_0": dict(dt=0.0), "dt_negative": dict(dt=-0.02), "dt_nan": dict(dt=nan), "dt_inf": dict(dt=inf),
           "scale_1": dict(scale=1.0), "scale_above_1": dict(scale=1.5), "scale_negative": dict(scale=-0.01), "scale_nan": dict(scale=nan)}
    for k in ("sigma_xy", "sigma_z", "sigma_yaw", "yaw_bias"):
        bad.update({k + "_negative": {k: -1e-3}, k + "_nan": {k: nan}, k + "_inf": {k: inf}})
    for name, kw in bad.items():
        assert check(**kw) == -1, name
        assert L.pgtt_elevation_last_error(), name
    assert L.pgtt_elevation_check_odometry(None) == -1 and L.pgtt_elevation_last_error()
    # the pointers are not looked at
    assert check(state=None, pose_est=None, odo=None, counter=None) == 0


def parse(*argv):
    return evaluate.make_parser().parse_args(list(argv))


def test_the_odometry_drift_parser():
    assert evaluate.odometry_drift(None) is None and evaluate.odometry_drift("") is True
    assert evaluate.odometry_drift("0.06") == dict(sigma_xy=0.06)
    assert evaluate.odometry_drift("0.06,0.03,0.03,0.015,0.06") == dict(sigma_xy=0.06, sigma_z=0.03, sigma_yaw=0.03, yaw_bias=0.015, scale=0.06)
    with pytest.raises(SystemExit, match="at most"):
        evaluate.odometry_drift("1,2,3,4,5,6")
    with pytest.raises(SystemExit, match="numbers"):
        evaluate.odometry_drift("0.02,much")


def test_the_flag_reaches_the_env_keywords():
    base = ("--task_name", "stairs")
    assert "odometry" not in str(evaluate.sensor_kwargs(parse(*base, "--elevation")))
    kw = evaluate.sensor_kwargs(parse(*base, "--elevation", "--odometry_drift"))
    assert kw["elevation"] == dict(odometry=True) and "depth" in kw
    kw = evaluate.sensor_kwargs(parse(*base, "--elevation", "48,0.05", "--odometry_drift", "0.06,0.03", "--elevation_fill", "--elevation_source", "lidar"))
    assert kw["elevation"] == dict(grid=48, res=0.05, fill=True, odometry=dict(sigma_xy=0.06, sigma_z=0.03), source="lidar") and "lidar" in kw
    kw = evaluate.sensor_kwargs(parse(*base, "--elevation", "--odometry_drift", "--sensor_every", "3"))
    assert kw["elevation"] == dict(follow_sensor=True, odometry=True)
    kw = evaluate.sensor_kwargs(parse(*base, "--elevation", "--odometry_drift", "--elevation_variance"))
    assert kw["elevation"] == dict(variance=True, odometry=True)


def test_the_flag_without_elevation_is_refused():
    with pytest.raises(SystemExit, match="--elevation"):
        evaluate.sensor_kwargs(parse("--task_name", "stairs", "--odometry_drift"))
    with pytest.raises(SystemExit, match="--elevation"):
        evaluate.sensor_kwargs(parse("--task_name", "stairs", "--odometry_drift", "0.02", "--student", "s.npz"))
