"""The pieces of the Initializer that no scene of tests/test_initializer_cpu.py reaches, through the hooks of include/drfe_debug.h
(DESIGN.md section 19): CheckRT with accepted NaN cosines - a point triangulated onto the first camera's centre - against the numpy
restatement, and the order the accepted cosines are ranked in."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import initializer_numpy as inp  # noqa: E402

from dr_slam_amd import lib  # noqa: E402

F = np.float32

# (regular matches, matches on the epipole): 31 and 51 accepted points select the NaN (index min(50, size - 1) is the last), 52 and
# 82 select a number and keep the status, 2 are NaNs alone, 30 without a NaN is the control
EPIPOLE_CASES = [(30, 1), (50, 1), (51, 1), (80, 2), (0, 2), (30, 0)]


def same_check(a, b):
    for k in ("good", "status"):
        assert a[k] == b[k], k
    for k in ("cos", "parallax", "vbGood", "vP3D"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def expect_epipole(got, n_regular, n_epipole, at):
    """what the case is built to show, independent of either implementation"""
    total = n_regular + n_epipole
    assert got["good"] == total and int(got["vbGood"].sum()) == n_regular
    assert got["status"] == (inp.MOTION_NAN_COS if n_epipole else 0)
    assert not got["vbGood"][at].any() and not got["vP3D"][at].any()          # on the centre: stored, never good
    selected_nan = n_epipole > 0 and min(50, total - 1) >= n_regular         # the NaNs rank above the n_regular numbers
    assert np.isnan(got["cos"]) == selected_nan and np.isnan(got["parallax"]) == selected_nan


@pytest.mark.parametrize("n_regular,n_epipole", EPIPOLE_CASES)
def test_check_rt_with_points_on_the_camera_centre(n_regular, n_epipole):
    K, R, t, sigma, m, at = inp.epipole_scene(n_regular, n_epipole, seed=n_regular)
    inp.RT_LOG = {}
    try:
        want = inp.check_rt_matches(K, R, t, sigma, m)
        log = inp.RT_LOG
    finally:
        inp.RT_LOG = None
    assert log.get("counted", 0) == n_regular + n_epipole and log.get("good", 0) == n_regular
    got = lib.init_check_rt(K, R, t, sigma, m)
    same_check(got, want)
    expect_epipole(got, n_regular, n_epipole, at)


def test_cosine_keys_order_as_the_floats_do():
    """-0 and +0 share a key, every NaN has the top key, and the keys of the numbers order as `<` orders the numbers"""
    rng = np.random.default_rng(11)
    special = np.array([0.0, -0.0, 1.0, -1.0, 0.99998, 1e-45, -1e-45, 1.17549435e-38, np.inf, -np.inf, np.nan, -np.nan], F)
    c = np.concatenate([special, rng.uniform(-1, 1, 500).astype(F), rng.standard_normal(100).astype(F) * F(1e-20)])
    key, value = lib.init_cos_keys(c)
    assert key.tolist() == [inp.cos_key(x) for x in c]
    want = np.array([inp.cos_of_key(int(k)) for k in key], F)
    assert value.tobytes() == want.tobytes()
    nan = np.isnan(c)
    assert (key[nan] == 0xFFFFFFFF).all() and (key[~nan] < 0xFFFFFFFF).all() and key[0] == key[1]
    assert np.array_equal(value[~nan], c[~nan]) and not np.signbit(value[1])
    order = np.argsort(key[~nan], kind="stable")
    assert np.array_equal(c[~nan][order], np.sort(c[~nan]))
    a, b = c[~nan][:300], c[~nan][300:600]
    assert np.array_equal(a < b, key[~nan][:300] < key[~nan][300:600])
