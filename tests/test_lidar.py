"""The LiDAR without a GPU: the fp64 reference (tests/lidar_reference.py) against closed forms, the facts of lidar.spherical_pattern, the ctypes
mirrors against the library's sizeof exports, every refusal of pgtt_lidar_check, and the ValueErrors of Joystick(lidar=..., elevation=...)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_reference as dref  # noqa: E402
import lidar_reference as ref  # noqa: E402

from phase_guided_terrain_traversal_amd import abi, configs, lidar, srchash  # noqa: E402

I3 = np.eye(3)


# ---------------------------------------------------------------- the reference against closed forms
def test_reference_flat_ground():
    """a level sensor at height h over the plane: range = h / -d.z for d.z < 0, far above the horizon and beyond reach; a point for every
    return strictly inside (near, far)"""
    h, near, far = 0.5, 0.05, 3.0
    pat = np.concatenate([lidar.spherical_pattern(24, 11, (-180, 180), (-85, 40)), [[0, 0, -1], [1, 0, 0], [0, 0, 1]]])
    yaw = 0.8
    R = dref.qmat([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
    o = np.array([0.3, -0.2, h])
    r = ref.scan(o, R, ref.unit_rows(pat), near, far)
    dz = ref.unit_rows(pat)[:, 2]
    t = h / np.where(dz < 0, -dz, 1.0)
    below = (dz < 0) & (t < far)
    assert below.sum() > 50 and (~below).sum() > 50
    assert np.abs(r["range"][below] - t[below]).max() < 1e-12 and (r["range"][~below] == far).all()
    assert (r["id"][below] == dref.ID_PLANE).all() and (r["id"][dz >= 0] == dref.ID_MISS).all()
    assert np.array_equal(np.isnan(r["points"]).all(1), ~below) and np.array_equal(np.isnan(r["points"]).any(1), ~below)
    assert np.abs(r["points"][below][:, 2]).max() < 1e-12                        # the points of floor returns lie on the floor
    assert np.abs(r["points"][below] - (o + t[below, None] * (ref.unit_rows(pat)[below] @ R.T))).max() < 1e-12


def test_reference_axis_aligned_box():
    """rays along +-x, +-y and -z (two components exactly 0 in the box frame) against one axis-aligned box"""
    box = [dict(c=np.array([1.0, 0.05, 0.3]), A=I3, h=np.array([0.25, 0.2, 0.3]))]      # x in [0.75, 1.25], y in [-0.15, 0.25], z in [0, 0.6]
    pat = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, -1]], float)
    far = 3.0
    cases = [((0.0, 0.0, 0.4), [0.75, far, far, far, 0.4]),                       # ahead of the box: +x meets the face, -z the floor
             ((1.0, 1.0, 0.5), [far, far, far, 0.75, 0.5]),                       # beside it: -y meets the face; +x is outside the y slab
             ((1.1, 0.1, 1.5), [far, far, far, far, 0.9]),                        # above it: -z meets the top
             ((0.0, 0.0, 0.9), [far, far, far, far, 0.9]),                        # too high for +x: outside the z slab
             ((2.0, 0.05, 0.3), [far, 0.75, far, far, 0.3])]                      # behind it: -x meets the far face
    for o, want in cases:
        r = ref.scan(np.array(o), I3, pat, 0.05, far, box)
        assert np.abs(r["range"] - want).max() < 1e-12, (o, r["range"])
    inside = ref.scan(np.array([1.0, 0.0, 0.3]), I3, pat, 0.05, far, box)         # a ray that starts inside the box does not see it
    assert np.abs(inside["range"] - [far, far, far, far, 0.3]).max() < 1e-12


def test_reference_clamp_and_ambiguity():
    near, far = 0.5, 2.0
    pat = np.array([[0, 0, -1.0], [1, 0, -1e-9], [0.6, 0, -0.8]])
    r = ref.scan(np.array([0.0, 0.0, 0.3]), I3, ref.unit_rows(pat), near, far)
    assert r["range"][0] == near and np.isnan(r["points"][0]).all()               # a hit below near reads near and has no point
    assert r["range"][1] == far and np.isnan(r["points"][1]).all()
    assert r["range"][2] == near
    # a ray that grazes a box's edge is ambiguous, one that meets the middle of a face is not; a hit at far is
    box = [dict(c=np.array([1.0, 0.0, 0.5]), A=I3, h=np.array([0.1, 0.5, 0.5]))]
    d = ref.unit_rows(np.array([[1, 0, 0.0], [0.9, 0.5 + 1e-4, 0.0]]))
    r = ref.scan(np.array([0.0, 0.0, 0.8]), I3, d, 0.05, 3.0, box)
    assert list(r["ambiguous"]) == [False, True]
    g = ref.scan(np.array([0.0, 0.0, 1.0]), I3, np.array([[0.0, 0.0, -1.0]]), 0.05, 1.0 + 5e-5)
    assert g["ambiguous"][0]


def test_reference_noise_stream():
    """stream 33, ray r in the place of pixel p: the camera's draws with the stream id changed, and no others"""
    u = ref.noise_uniforms(1234, 5, 7, 64)
    ctr = np.zeros((64, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = 5, 7, 33, np.arange(64)
    w = dref.philox4x32_10((1234, 0), ctr)
    assert np.array_equal(u, (w[:, :3] >> 8) / 16777216.0) and not np.array_equal(u, dref.noise_uniforms(1234, 5, 7, 64))
    assert ref.RS_LIDAR == lidar.RS_LIDAR == 33 and dref.RS_DEPTH == 32
    rng = np.full(64, 1.0)
    out, dropped, u0 = ref.apply_noise(rng, 0.05, 3.0, 0.0, 0.25, 1234, 5, 7)
    assert np.array_equal(dropped, u0 < 0.25) and 0 < dropped.sum() < 64
    assert (out[dropped] == 3.0).all() and (out[~dropped] == 1.0).all()


# ---------------------------------------------------------------- spherical_pattern
def test_spherical_pattern():
    n_az, n_el = 8, 5
    p = lidar.spherical_pattern(n_az, n_el, (-180, 180), (-85, 10))
    assert p.shape == (40, 3) and np.abs(np.linalg.norm(p, axis=1) - 1).max() < 1e-15
    assert np.abs(p - ref.spherical_pattern(n_az, n_el, (-180, 180), (-85, 10))).max() < 1e-15
    el = np.degrees(np.arcsin(p[:, 2])).reshape(n_az, n_el)
    az = np.degrees(np.arctan2(p[:, 1], p[:, 0])).reshape(n_az, n_el)
    # ray r = a * n_el + k: the elevation runs fastest, over the CLOSED interval; the azimuths sit at the centres of their cells
    assert np.allclose(el, np.linspace(-85, 10, n_el)[None, :]) and np.allclose(el[:, 0], -85) and np.allclose(el[:, -1], 10)
    assert np.allclose(az, (-180 + (np.arange(n_az) + 0.5) * 45)[:, None])
    assert len({tuple(np.round(r, 12)) for r in p}) == 40                        # a full turn repeats no direction
    one = lidar.spherical_pattern(4, 1, (0, 90), (-30, -10))
    assert np.allclose(np.degrees(np.arcsin(one[:, 2])), -20) and np.allclose(np.degrees(np.arctan2(one[:, 1], one[:, 0])), [11.25, 33.75, 56.25, 78.75])
    with pytest.raises(ValueError):
        lidar.spherical_pattern(0, 4)


def test_settings_and_defaults():
    s = lidar.settings()
    assert s == lidar.DEFAULTS and s["n_az"] * s["n_el"] <= lidar.MAX_RAYS and s["every"] == 1 and s["see_robot"]
    given = lidar.settings(dict(pattern=np.eye(3), far=2.0))
    assert "n_az" not in given and "n_el" not in given and given["far"] == 2.0 and given["near"] == lidar.DEFAULTS["near"]
    assert C.sizeof(lidar.PgttLidarConfig) == 72 and C.sizeof(lidar.PgttLidarBuffers) == 48
    with pytest.raises(ValueError):
        lidar.pattern_array(np.zeros((4, 2)))


# ---------------------------------------------------------------- the host side of the library
needs_lib = pytest.mark.skipif(not os.path.exists(lidar.LIB_PATH), reason="libpgtt_lidar.so not built (run __graft_entry__.build())")
GOOD = dict(near=0.05, far=3.0, mount_body=0, mount_pos=(0.29, 0.0, -0.04), mount_quat=(1.0, 0.0, 0.0, 0.0), every=1)


@needs_lib
def test_sizeof_exports_and_build_info():
    L = lidar.lib()
    assert L.pgtt_lidar_sizeof_config() == C.sizeof(lidar.PgttLidarConfig)
    assert L.pgtt_lidar_sizeof_buffers() == C.sizeof(lidar.PgttLidarBuffers)
    info = lidar.build_info()
    assert info["src"] == srchash.side_sha256("lidar") and info["flavor"] == "product"
    for name in lidar.EXPORTS:
        getattr(L, name)


@needs_lib
def test_check_refuses():
    """pgtt_lidar_check: host only, no GPU"""
    L = lidar.lib()
    pat = lidar.pattern_array(lidar.spherical_pattern(8, 4))

    def rc(dirs=pat, R=None, **kw):
        cfg = lidar.config_struct(**dict(GOOD, **kw))
        return L.pgtt_lidar_check(C.byref(cfg), None if dirs is None else dirs.ctypes.data, len(dirs) if R is None else R)

    assert rc() == 0
    assert rc(mount_body=abi.NBODY - 1) == 0 and rc(dropout=0.5, sigma=0.1) == 0 and rc(every=7) == 0
    full = lidar.pattern_array(np.tile(pat, (lidar.MAX_RAYS // len(pat) + 1, 1)))
    assert rc(dirs=full, R=lidar.MAX_RAYS) == 0 and rc(R=1) == 0
    zero_row, nan_row, inf_row = pat.copy(), pat.copy(), pat.copy()
    zero_row[5] = 0.0; nan_row[7, 1] = np.nan; inf_row[0, 2] = np.inf
    bad = {"R = 0": dict(R=0), "R = MAX + 1": dict(dirs=full, R=lidar.MAX_RAYS + 1), "a zero row": dict(dirs=zero_row), "a NaN row": dict(dirs=nan_row),
           "an infinite row": dict(dirs=inf_row), "a null pattern": dict(dirs=None, R=4), "near = far": dict(near=3.0), "near > far": dict(near=4.0),
           "near = 0": dict(near=0.0), "far infinite": dict(far=float("inf")), "every = 0": dict(every=0), "dropout = 1": dict(dropout=1.0),
           "sigma < 0": dict(sigma=-0.1), "a zero mount_quat": dict(mount_quat=(0.0, 0.0, 0.0, 0.0)), "mount_body = 13": dict(mount_body=13),
           "mount_body < 0": dict(mount_body=-1), "mount_pos NaN": dict(mount_pos=(0.0, float("nan"), 0.0))}
    assert abi.NBODY == 13
    for name, kw in bad.items():
        assert rc(**kw) == -1, name
        assert L.pgtt_lidar_last_error(), name
    assert L.pgtt_lidar_check(None, pat.ctypes.data, len(pat)) == -1
    with pytest.raises(lidar.LidarError, match="pgtt_lidar_check"):
        lidar.check_settings(lidar.config_struct(**dict(GOOD, every=0)), pat)
    lidar.check_settings(lidar.config_struct(**GOOD), pat)


# one bad value of every field the LiDAR's config has in common with the camera's (the checks are stated once, csrc/pgtt_sensor.hip.h), in the
# order of the checks, and the words libpgtt_lidar.so had for it before they were: byte for byte, behind the entry point's name
SHARED_REFUSALS = [(dict(near=0.0), "need 0 < near < far, finite"), (dict(far=float("inf")), "need 0 < near < far, finite"),
                   (dict(mount_body=13), "mount_body outside [0, PGTT_NBODY)"), (dict(every=0), "every must be >= 1"),
                   (dict(see_robot=2), "see_robot must be 0 or 1"), (dict(sigma=-0.1), "noise_sigma must be >= 0"),
                   (dict(sigma=float("inf")), "noise_sigma must be >= 0"), (dict(dropout=1.0), "dropout must be in [0, 1)"),
                   (dict(mount_quat=(0.0, 0.0, 0.0, 0.0)), "mount_quat must be a non-zero quaternion"),
                   (dict(mount_pos=(0.0, float("nan"), 0.0)), "mount_pos must be finite")]


@needs_lib
def test_check_refusal_texts():
    """pgtt_lidar_check's exact message for each shared field, and for the LiDAR's own checks, which come last: a config that is bad in a
    shared field AND has R = 0 is refused for the shared field"""
    L = lidar.lib()
    pat = lidar.pattern_array(lidar.spherical_pattern(8, 4))

    def message(R=len(pat), dirs=pat, see_robot=True, **kw):
        cfg = lidar.config_struct(**dict(GOOD, **kw))
        cfg.see_robot = int(see_robot)                                            # config_struct makes it 0 or 1
        assert L.pgtt_lidar_check(C.byref(cfg), None if dirs is None else dirs.ctypes.data, R) == -1, kw
        return L.pgtt_lidar_last_error().decode()

    for kw, text in SHARED_REFUSALS:
        assert message(**kw) == "pgtt_lidar_check: " + text, kw
        assert message(R=0, **kw) == "pgtt_lidar_check: " + text, kw
    assert message(near=0.0, every=0, mount_pos=(float("inf"), 0.0, 0.0)) == "pgtt_lidar_check: need 0 < near < far, finite"
    assert message(every=0, mount_pos=(float("inf"), 0.0, 0.0)) == "pgtt_lidar_check: every must be >= 1"
    assert message(R=0) == "pgtt_lidar_check: R must be in [1, PGTT_LIDAR_MAX_RAYS]"
    assert message(dirs=None) == "pgtt_lidar_check: null pattern"
    zero_row = pat.copy()
    zero_row[5] = 0.0
    assert message(dirs=zero_row) == "pgtt_lidar_check: pattern row 5 is zero or not finite"
    assert L.pgtt_lidar_check(None, pat.ctypes.data, len(pat)) == -1 and L.pgtt_lidar_last_error().decode() == "pgtt_lidar_check: null config"


def test_joystick_refusals():
    """before anything touches a device"""
    from phase_guided_terrain_traversal_amd.env import Joystick
    cfg = configs.training_config()
    with pytest.raises(ValueError, match="needs lidar"):
        Joystick("stairs", cfg, num_envs=4, elevation=dict(source="lidar"))
    with pytest.raises(ValueError, match="needs lidar"):
        Joystick("stairs", cfg, num_envs=4, depth={}, elevation=dict(source="lidar", grid=24))      # a camera does not stand in for the LiDAR
    with pytest.raises(ValueError, match="every=1"):
        Joystick("stairs", cfg, num_envs=4, lidar=dict(every=2), elevation=dict(source="lidar"))
    with pytest.raises(ValueError, match="source"):
        Joystick("stairs", cfg, num_envs=4, lidar={}, elevation=dict(source="radar"))
    with pytest.raises(ValueError, match="needs depth"):
        Joystick("stairs", cfg, num_envs=4, lidar={}, elevation=True)                               # the default source is the camera still
