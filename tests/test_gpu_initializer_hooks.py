"""-m gpu tests of the device's CheckRT kernel alone (drfe_debug_init_check_rt) on hypotheses whose accepted
cosines hold NaNs - points triangulated onto the first camera's centre - which no scene reaches: device == host == numpy on every
output, the status included, with the NaN selected (at most 51 accepted points) and not (more), in one and in several wavefront
passes over the matches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import initializer_numpy as inp  # noqa: E402
from test_initializer_hooks_cpu import EPIPOLE_CASES, expect_epipole, same_check  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    yield c
    c.close()


@pytest.mark.parametrize("n_regular,n_epipole", EPIPOLE_CASES + [(200, 3)])
def test_device_check_rt_with_points_on_the_camera_centre(ctx, n_regular, n_epipole):
    from dr_slam_amd import lib
    K, R, t, sigma, m, at = inp.epipole_scene(n_regular, n_epipole, seed=n_regular)
    host = lib.init_check_rt(K, R, t, sigma, m)
    dev = lib.init_check_rt(K, R, t, sigma, m, ctx=ctx)
    same_check(dev, host)
    same_check(dev, inp.check_rt_matches(K, R, t, sigma, m))
    expect_epipole(dev, n_regular, n_epipole, at)


def test_device_check_rt_after_a_batch_call(ctx):
    """the hook shares the context's staging blocks with drfe_init_ransac_batch: a batch call, the hook, the batch call again"""
    from dr_slam_amd import lib
    problems = inp.pack([inp.planted(np.random.default_rng(7), 40, max_iterations=4, seed=7)])
    a = ctx.init_ransac_batch(problems)
    K, R, t, sigma, m, at = inp.epipole_scene(30, 1, seed=30)
    same_check(lib.init_check_rt(K, R, t, sigma, m, ctx=ctx), lib.init_check_rt(K, R, t, sigma, m))
    b = ctx.init_ransac_batch(problems)
    assert not inp.differing(lib.init_table(a, 0), lib.init_table(b, 0))
