"""-m gpu: the device's line matchers on the hand-built key lines of line_match_scenarios.py, through the entries of
lib.Context: lsd_search_by_projection_map / _last (k_line_queries_last, k_line_search), is_in_frustum_lines (k_frustum_lines),
lsd_fuse_search / lsd_fuse_search_sim3 / lsd_search_by_projection_kf / lsd_search_by_sim3 (k_line_fuse_search and the host
replays around it) and lsd_search_by_descriptor / lsd_search_for_triangulation (k_bf_knn and line_mad).
Bar: every count and every output array equal to the CPU oracle AND to the outcome stated by hand from the reference
source.  Everything is an integer or an index; the projections is_in_frustum_lines hands back are compared bit for bit
(a NaN with a NaN).  tests/test_line_match_edges_cpu.py checks that the scenarios sit on their decision points."""
import numpy as np
import pytest

import line_match_scenarios as L
from match_scenarios import F32, hamming, scale_factors

pytestmark = pytest.mark.gpu

WINDOWED = ([L.window_gates()] + [L.motion_levels(*m) for m in L.MOTIONS] + L.scan_scenarios() + [L.scan_thresholds(r) for r in (0.9, 0.75)]
            + [L.claims(), L.claim_chain()] + L.fuse_ties() + [L.sized(n) for n in L.SIZES])
FRUSTUM = L.frustum()
I4 = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    assert np.array_equal(c.scale_tables()[0], scale_factors())
    for mine, theirs in ((L.MAPLINE_DTYPE, lib.MAPLINE_DTYPE), (L.TRACKED_LINE_DTYPE, lib.TRACKED_LINE_DTYPE),
                         (L.FRUSTUM_LINE_DTYPE, lib.FRUSTUM_LINE_DTYPE)):
        assert mine == theirs
    yield c
    c.close()


def _cam():
    from dr_slam_amd import lib
    return lib.Camera(**L.CAM)


def _kl(cur):
    from dr_slam_amd import lib
    k = np.zeros(len(cur), lib.KEYLINE_DTYPE)
    for f in ("pt_x", "pt_y", "angle", "octave"):
        k[f] = cur[f]
    return k


def _scaled(sim3):
    T = I4.copy()
    if sim3:
        T[:3, :] *= F32(2.0)
    return T


def _same(got, oracle, want, what):
    assert oracle[0] == want[0] and np.array_equal(oracle[1], want[1]), (what, "oracle")
    assert got[0] == want[0], (what, got[0], want[0])
    bad = np.flatnonzero(got[1] != want[1])
    assert bad.size == 0, (what, [(int(k), int(got[1][k]), int(want[1][k])) for k in bad[:8]])


def dev_map(c, s):
    return c.lsd_search_by_projection_map(s.scene.tracked(), _kl(s.scene.cur), s.scene.desc, s.r0 / 5.0, s.nnratio, s.cur_ml(), s.cur_obs)


def dev_last(c, s):
    return c.lsd_search_by_projection_last(I4, s.Tcw_last, _cam(), s.scene.map_lines(), _kl(s.scene.cur), s.scene.desc, s.r0, s.mono,
                                           s.nnratio, s.cur_ml(), s.cur_obs)


def dev_fuse(c, s, sim3):
    fn = c.lsd_fuse_search_sim3 if sim3 else c.lsd_fuse_search
    return fn(_scaled(sim3), _cam(), s.scene.frustum_lines(), s.scene.descs(), s.scene.skip(), _kl(s.scene.cur), s.scene.desc, s.r0)


@pytest.mark.parametrize("s", WINDOWED, ids=lambda s: s.name)
def test_windowed(ctx, oracle_mod, s):
    if "map" in s.expect:
        _same(dev_map(ctx, s), L.oracle_map(oracle_mod, s), s.expected("map"), "map")
    if "last" in s.expect:
        _same(dev_last(ctx, s), L.oracle_last(oracle_mod, s), s.expected("last"), "last")
    if "fuse" in s.expect:
        ei, ed = s.expected_fuse()
        for sim3 in (False, True):
            oi, od = L.oracle_fuse(oracle_mod, s, sim3)
            bi, bd = dev_fuse(ctx, s, sim3)
            assert np.array_equal(oi, ei) and np.array_equal(od, ed), (sim3, "oracle")
            assert np.array_equal(bi, ei) and np.array_equal(bd, ed), (sim3, list(bi), list(ei), list(bd), list(ed))


def test_empty_lists_and_capacity(ctx):
    """No map lines, no key lines (both entries, and a keyframe without key lines for Fuse); 4 097 key lines are one more than
    line_search_run takes: DRFE_ERR_CAPACITY with its reason, and the context goes on working."""
    from dr_slam_amd import lib
    s = L.sized(64)
    sc = s.scene
    kl = _kl(sc.cur)
    n, m = ctx.lsd_search_by_projection_map(sc.tracked()[:0], kl, sc.desc, 1.0, 0.9, s.cur_ml())
    assert n == 0 and (m == -1).all()
    n, m = ctx.lsd_search_by_projection_last(I4, I4, _cam(), sc.map_lines()[:0], kl, sc.desc, 5.0, False, 0.9, s.cur_ml())
    assert n == 0 and (m == -1).all()
    n, m = ctx.lsd_search_by_projection_map(sc.tracked(), kl[:0], sc.desc[:0], 1.0, 0.9, s.cur_ml()[:0])
    assert n == 0 and len(m) == 0
    n, m = ctx.lsd_search_by_projection_last(I4, I4, _cam(), sc.map_lines(), kl[:0], sc.desc[:0], 5.0, False, 0.9, s.cur_ml()[:0])
    assert n == 0 and len(m) == 0
    bi, bd = ctx.lsd_fuse_search(I4, _cam(), sc.frustum_lines(), sc.descs(), sc.skip(), kl[:0], sc.desc[:0], 5.0)
    assert list(bi) == [-1]
    big = L.sized(4097)
    for run in (dev_map, dev_last):
        with pytest.raises(lib.DrfeError, match=r"\(-3\).*too many lines"):
            run(ctx, big)
    n, m = dev_map(ctx, s)
    assert (n, int(m[63])) == (1, 0)


# ---------------------------------------------------------------------------------------------------------------------
# projection gates, bands, cones, PredictScale

def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def test_frustum_lines(ctx, oracle_mod):
    """k_frustum_lines against the oracle (every field of every line) and the hand-stated in_view / level.  The levels of the eleven
    lines whose distance ratio is an exact product of the scale table (FrustumScenario.level is None: band_max_on, level_neg_* and
    ratio_scale_0 .. 7) are compared with the oracle alone - the only cases of this file without a hand-stated outcome.  The
    level_neg_* lines must hand back the raw -1 (the CPU test holds the oracle to -1 there)."""
    f = FRUSTUM
    o = oracle_mod.is_in_frustum_lines(L.cam9(), I4, 1.2, f.lines, 0.5)
    g = ctx.is_in_frustum_lines(I4, _cam(), f.lines, 0.5)
    assert list(g["in_view"]) == list(o["in_view"]) == f.in_view
    assert np.array_equal(g["level"], o["level"])
    assert [int(v) for v, lv in zip(g["level"], f.level) if lv is not None] == [lv for lv in f.level if lv is not None]
    for k in ("x1", "y1", "x2", "y2", "view_cos"):
        assert _bits_equal(g[k], o[k]), k
    for mx in L.NEGATIVE_LEVEL_MAX:
        k = f.names.index(f"level_neg_{mx}")
        assert (g["in_view"][k], g["level"][k]) == (1, -1), mx
    z = f.names.index("depth_zero")
    assert np.isnan(g["x1"][z]) and np.isnan(g["y1"][z]) and (g["x2"][z], g["y2"][z]) == (320.0, 240.0)


@pytest.mark.parametrize("sim3", [False, True], ids=["Tcw", "Scw"])
def test_frustum_fuse(ctx, oracle_mod, sim3):
    """The same lines through k_line_fuse_search: a level outside the pyramid, above (8, 9) or below (-1), is reported as -2; the
    nine exact-ratio lines inside the pyramid are compared with the oracle alone."""
    f = FRUSTUM
    skip = np.zeros(len(f.lines), np.uint8)
    T = _scaled(sim3)
    oi, od = (oracle_mod.lsd_fuse_search_sim3 if sim3 else oracle_mod.lsd_fuse_search)(L.cam9(), T, 1.2, scale_factors(), f.lines, f.descs,
                                                                                       skip, f.cur, f.cur_desc, 5.0)
    bi, bd = (ctx.lsd_fuse_search_sim3 if sim3 else ctx.lsd_fuse_search)(T, _cam(), f.lines, f.descs, skip, _kl(f.cur), f.cur_desc, 5.0)
    assert np.array_equal(bi, oi) and np.array_equal(bd, od), [(f.names[k], int(bi[k]), int(oi[k])) for k in np.flatnonzero(bi != oi)]
    for k, fu in enumerate(f.fuse):
        if fu is not None:
            assert bi[k] == fu, (f.names[k], int(bi[k]), fu)
            assert fu < 0 or bd[k] == hamming(f.descs[k], f.cur_desc[fu])


def test_frustum_last(ctx, oracle_mod):
    f = FRUSTUM
    free = np.full(len(f.cur), -1, np.int32)
    ml = L.frustum_map_lines(f)
    want = free.copy()
    for k, q in f.last_expect[1].items():
        want[k] = q
    o = oracle_mod.lsd_search_by_projection_last(L.cam9(), I4, I4, scale_factors(), ml, f.cur, f.cur_desc, 5.0, False, 0.9, free)
    g = ctx.lsd_search_by_projection_last(I4, I4, _cam(), ml, _kl(f.cur), f.cur_desc, 5.0, False, 0.9, free)
    _same(g, o, (f.last_expect[0], want), "last")


# ---------------------------------------------------------------------------------------------------------------------
# keyframe entries

@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_search_by_projection_kf(ctx, oracle_mod, scale):
    s = L.kf_first_come()
    sc = s.scene
    T = I4.copy()
    T[:3, :] *= F32(scale)
    o = oracle_mod.lsd_search_by_projection_kf(L.cam9(), T, 1.2, scale_factors(), sc.frustum_lines(), sc.descs(), sc.skip(), sc.cur, sc.desc,
                                               s.matched, 5)
    g = ctx.lsd_search_by_projection_kf(T, _cam(), sc.frustum_lines(), sc.descs(), sc.skip(), _kl(sc.cur), sc.desc, s.matched, 5)
    _same(g, o, s.expected(), "kf")
    n, new = ctx.lsd_search_by_projection_kf(T, _cam(), sc.frustum_lines(), sc.descs(), sc.skip(), _kl(sc.cur)[:0], sc.desc[:0], s.matched[:0], 5)
    assert n == 0 and len(new) == 0


def test_search_by_sim3(ctx, oracle_mod):
    s = L.sim3_pairs()
    pose, sides = L.sim3_args(s)
    o = oracle_mod.lsd_search_by_sim3(L.cam9(), *pose, 1.2, scale_factors(), *sides, 5.0)
    dev_sides = list(sides)
    dev_sides[3], dev_sides[8] = _kl(s.kl1), _kl(s.kl2)
    g = ctx.lsd_search_by_sim3(_cam(), *pose, *dev_sides, 5.0)
    _same(g, o, s.expected(), "sim3")


# ---------------------------------------------------------------------------------------------------------------------
# descriptor matchers

def test_ratio_rule(ctx, oracle_mod):
    Q, T, has, n_e, out_e, _ = L.ratio_rule()
    _same(ctx.lsd_search_by_descriptor(Q, T, has, mode=0), oracle_mod.lsd_search_by_descriptor(Q, has, T), (n_e, out_e), "ratio")
    n, out = ctx.lsd_search_by_descriptor(Q, T[:1], has, mode=0)                 # fewer than two train rows
    assert n == 0 and list(out) == [-1]
    # the 2-NN lists themselves: ties in ascending train order
    idx, dist = ctx.bf_knn(Q, T, 2)
    oi, od = oracle_mod.bf_knn(Q, T, 2)
    assert np.array_equal(idx, oi) and np.array_equal(dist, od) and list(idx[4]) == [8, 9] and list(dist[4]) == [0, 0]


@pytest.mark.parametrize("n", [1, 2, 4, 5])
def test_gap_rule(ctx, oracle_mod, n):
    Q, T, gaps, half, tenth = L.gap_rule(n)
    _same(ctx.lsd_search_by_descriptor(Q, T, None, mode=1), oracle_mod.lsd_search_by_gap(Q, T), L.gap_expected(n, half), "gap")
    has_t = np.ones(len(T), np.uint8)
    has_t[2 * (n - 1)] = 0
    _same(ctx.lsd_search_by_descriptor(Q, T, has_t, mode=1), oracle_mod.lsd_search_by_gap(Q, T, has_t), L.gap_expected(n, half, has_t),
          "gap, train mask")
    h1, h2 = np.zeros(n, np.uint8), np.zeros(len(T), np.uint8)
    _same(ctx.lsd_search_for_triangulation(Q, T, h1, h2), oracle_mod.lsd_search_for_triangulation(Q, T, h1, h2), L.gap_expected(n, tenth),
          "triangulation")
    h1[0], h2[2 * (n - 1)] = 1, 1
    acc = [a and q != 0 and q != n - 1 for q, a in enumerate(tenth)]
    _same(ctx.lsd_search_for_triangulation(Q, T, h1, h2), oracle_mod.lsd_search_for_triangulation(Q, T, h1, h2), L.gap_expected(n, acc),
          "triangulation, masks")


@pytest.mark.parametrize("gap,accept", [(0, 0), (5, 1)])
def test_gap_rule_with_zero_mad(ctx, oracle_mod, gap, accept):
    Q, T = L.gap_rule_equal(gap)
    want = L.gap_expected(3, [accept] * 3)
    _same(ctx.lsd_search_by_descriptor(Q, T, None, mode=1), oracle_mod.lsd_search_by_gap(Q, T), want, "gap")
    z1, z2 = np.zeros(3, np.uint8), np.zeros(6, np.uint8)
    _same(ctx.lsd_search_for_triangulation(Q, T, z1, z2), oracle_mod.lsd_search_for_triangulation(Q, T, z1, z2), want, "triangulation")
    n, out = ctx.lsd_search_by_descriptor(Q, T[:1], None, mode=1)
    assert n == 0 and (out == -1).all()
    n, out = ctx.lsd_search_for_triangulation(Q, T[:1], z1, z2[:1])
    assert n == 0 and (out == -1).all()
