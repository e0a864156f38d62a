"""-m gpu tests that hold device triangulation to the hand-built cases of tests/triangulate_scenarios.py:
every case alone (device == host == numpy, and the case's stated outcome on the device result); a ladder of 17 float steps
across every gate the CPU tests find by bisection (5.991 / 7.8 sigma^2, 0.9998, equal stereo cosines, both ratio tests, mb at
the baseline), device == numpy at every rung; all cases merged into one call and repeated, rotated, over three workgroups, on a
context whose staging blocks hold a larger call's accepted points; and drfe_math.h's canonical atan2f / cosf evaluated by a
kernel of triangulate_kernels.hip over every depth and baseline that occurs, bit for bit the host's values (which
tests/test_triangulate_cpu.py holds to mpmath)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulate_numpy as TN  # noqa: E402
import triangulate_scenarios as TS  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("status", "branch", "x3d", "pair_skipped", "accepted")
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    return TS.cases()


def _same(got, want, what=""):
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def _host(scene, line):
    from dr_slam_amd import lib
    return (lib.triangulate_lines_host if line else lib.triangulate_points_host)(scene)


def _device(ctx, scene, line):
    return (ctx.triangulate_lines_batch if line else ctx.triangulate_points_batch)(scene)


def test_each_case_alone(ctx, cases):
    assert len(cases) >= 35 and sum(1 for c in cases if c[2]) >= 7
    for name, scene, line, expect in cases:
        dev = _device(ctx, scene, line)
        _same(dev, _host(scene, line), name)
        _same(dev, TN.triangulate(scene, line), name)
        TS.holds(expect, dev)


@pytest.mark.parametrize("name", TS.LADDERS)
def test_gate_ladder(ctx, name):
    """8 ulp below the flip to 8 ulp above it, 17 pairs of one call: device == numpy at every rung, and both decisions occur
    (a condition on the inputs; the decision need not flip once: cosParallaxRays is not monotone in tx at ulp steps)"""
    rungs = TS.ladder(name)
    assert len(rungs) == 17
    scene = TS.merge(rungs)
    want = TN.triangulate(scene)
    assert len(want["status"]) == 17
    if name == "baseline_mb":
        decisions = set(want["pair_skipped"].tolist())
    else:
        decide = TS.GATES[name]()[3]
        decisions = {bool(decide(st)) for st in want["status"]}
    assert len(decisions) == 2
    _same(_device(ctx, scene, False), want, name)


@pytest.mark.parametrize("line", [False, True])
def test_all_cases_in_one_call_at_many_lane_positions(ctx, cases, line):
    """the merged cases, repeated and rotated by one case per repetition until the call holds more than 512 matches (three
    workgroups of 256; every case on both sides of lanes 63 / 64 and 255 / 256), after a random scene whose accepted points
    filled the staging blocks: device == host, and every copy of a case is that case's single-call result"""
    own = [(n, s) for n, s, ln, _ in cases if ln == line]
    single = [_device(ctx, s, line) for _, s in own]
    rng = np.random.default_rng(41)
    big = TN.random_scene(rng, n_kf=8, n_feat=400, n_pairs=40, line=line)
    warm = _device(ctx, big, line)
    assert len(warm["status"]) > 1200 and int(warm["accepted"].sum()) > 300
    order = []
    rep = 0
    while len(order) <= 512:
        order += [(q + rep) % len(own) for q in range(len(own))]
        rep += 1
    scene = TS.merge([own[q][1] for q in order], line)
    assert 512 < len(scene["matches"]) == len(order) < len(warm["status"])
    for q in range(len(own)):
        at = [i for i, o in enumerate(order) if o == q]
        assert {i % 256 < 64 for i in at} == {True, False} and {i // 256 for i in at} >= {0, 1}
    dev = _device(ctx, scene, line)
    _same(dev, _host(scene, line))
    for i, q in enumerate(order):
        for k in KEYS:
            assert dev[k][i].tobytes() == single[q][k][0].tobytes(), (own[q][0], i, k)


@pytest.fixture(scope="module")
def math_inputs():
    """every raw depth 1..65535 at DepthMapFactor 5000 against the three mb / 2 of TUM1 / 2 / 3, and the log-uniform block of
    tests/test_triangulate_cpu.py; the doubled angles that result (from the host entry) and random angles of [0, pi]"""
    from dr_slam_amd import lib, synth
    rng = np.random.default_rng(9)
    depth = (np.arange(1, 65536, dtype=np.float32) * (F(1) / F(5000)))
    ys = [F(F(cam.bf) / F(cam.fx)) / F(2) for cam in (synth.TUM1, synth.TUM2, synth.TUM3)]
    y = np.concatenate([np.full(len(depth), v, np.float32) for v in ys] + [np.exp(rng.uniform(-12, 5, 100000)).astype(np.float32)])
    x = np.concatenate([depth] * len(ys) + [np.exp(rng.uniform(-12, 5, 100000)).astype(np.float32)])
    ang = np.concatenate([F(2) * lib.triangulate_math(0, y, x), rng.uniform(0, np.pi, 100000).astype(np.float32),
                          np.float32([0, np.pi, np.pi / 2])])
    ang = ang[ang <= F(np.pi)]
    return {0: (y, x), 1: (ang, None), 2: (F(2) * y, x)}


@pytest.mark.parametrize("which", [0, 1, 2])
def test_canonical_functions_on_the_device(ctx, math_inputs, which):
    """drfe_atan2f, drfe_cosf and the stereo parallax cos(2 atan2(mb / 2, z)) as triangulate_kernels.hip compiles them equal
    the host entry bit for bit, at 0, 1, 63, 64, 65 elements and over the whole array"""
    from dr_slam_amd import lib
    y, x = math_inputs[which]
    assert len(y) > 290000
    want = lib.triangulate_math(which, y, x)
    for n in (0, 1, 63, 64, 65, len(y)):
        got = ctx.triangulate_math(which, y[:n], None if x is None else x[:n])
        assert got.shape == (n,) and np.array_equal(got.view(np.int32), want[:n].view(np.int32)), (which, n)
