"""The CPU oracle of the line matchers (LSDmatcher, Frame::GetLinesInArea, Frame::isInFrustum(MapLine*), lineDescriptorMAD)
against the outcomes stated by hand from the reference source for the key lines of line_match_scenarios.py - and the
conditions that make those scenarios what they claim to be: stated Hamming distances by unpackbits, floats exactly on their
bounds with their neighbours on the other side, the window membership of every named candidate from a float32 / float64
evaluation of the reference expression, the lane of every named index, and scan outcomes that change under the two wrong
tie rules.  tests/test_gpu_line_match_edges.py holds the device to the same outcomes."""
import numpy as np
import pytest

import line_match_scenarios as L
from match_scenarios import F32, hamming, scale_factors, ulp_above, ulp_below

WINDOW = L.window_gates()
MOTION = [L.motion_levels(*m) for m in L.MOTIONS]
SCAN = L.scan_scenarios()
THRESH = [L.scan_thresholds(r) for r in (0.9, 0.75)]
CLAIMS = [L.claims(), L.claim_chain()]
TIES = L.fuse_ties()
SIZED = [L.sized(n) for n in L.SIZES]
WINDOWED = [WINDOW] + MOTION + SCAN + THRESH + CLAIMS + TIES + SIZED
FRUSTUM = L.frustum()
KF = L.kf_first_come()
SIM3 = L.sim3_pairs()
_ID = dict(ids=lambda s: s.name)


def test_scenarios_cite_the_reference():
    for s in WINDOWED:
        assert "src/LSDmatcher.cpp" in s.ref or "src/Frame.cc" in s.ref, s.name
    assert len(SCAN) == 3 * 6 * 4 and len({s.name for s in WINDOWED}) == len(WINDOWED)


# ---------------------------------------------------------------------------------------------------------------------
# conditions

def _named_ok(scene, r0, named):
    sc = scale_factors()
    for c in named:
        q = scene.q[c.q]
        assert hamming(q["desc"], scene.desc[c.idx]) == c.dist, (c.q, c.idx)
        kl = scene.cur[c.idx]
        r = F32(F32(r0) * sc[q["level"]])
        got = L.area_gates(q["x1"], q["y1"], q["x2"], q["y2"], r, kl["pt_x"], kl["pt_y"], kl["angle"])
        assert got[0] == c.radius, (c.q, c.idx, "radius")
        if got[0]:                                      # the slope test is only reached inside the radius (src/Frame.cc:795-800)
            assert got[1] == c.slope, (c.q, c.idx, "slope")
        if c.lane is not None:
            assert c.idx % L.WAVE == c.lane


@pytest.mark.parametrize("s", WINDOWED, **_ID)
def test_named_candidates_sit_where_they_are_claimed(s):
    assert s.scene.named
    _named_ok(s.scene, s.r0, s.scene.named)
    # every key line nobody names is parked outside every window
    named = {c.idx for c in s.scene.named}
    parked = np.array([k for k in range(len(s.scene.cur)) if k not in named], int)
    assert (s.scene.cur["pt_x"][parked] >= 5000).all()


def test_scan_scenarios_sit_in_the_lanes_they_name():
    for s in SCAN:
        lanes = [k % L.WAVE for k in s.idx]
        winner, best, second = s.table
        b, c = s.idx[s.order.index(best)], s.idx[s.order.index(second)]
        assert list(s.idx) == sorted(s.idx) and len(s.scene.cur) >= 130
        if s.name.endswith("three_lanes"):
            assert len(set(lanes)) == 3
        elif s.name.endswith("pair_one_lane"):
            assert b % L.WAVE == c % L.WAVE and len(set(lanes)) == 2
        elif s.name.endswith("all_one_lane"):
            assert len(set(lanes)) == 1 and s.idx[1] == s.idx[0] + 64 and s.idx[2] == s.idx[0] + 128
        else:
            assert s.idx[:2] == (63, 64) and lanes[:2] == [63, 0]
    # Fuse's ties: one lane one trip apart, neighbouring lanes, one lane three times
    for (idxs, lanes, win), s in zip(L.FUSE_TIES, TIES):
        assert [k % L.WAVE for k in idxs] == list(lanes) and win == min(idxs)
        assert [c.lane for c in s.scene.named if c.q == 0 and c.idx in idxs] == list(lanes)
    assert [len(set(t[1])) for t in L.FUSE_TIES] == [1, 2, 1] and L.FUSE_TIES[1][0] == (69, 70)


def test_scan_outcomes_follow_the_reference_loop_and_no_other_tie_rule():
    """The hand-stated table against a restatement of src/LSDmatcher.cpp:97-136, and against the same loop with the tie rule
    flipped: every scan scenario changes its outcome under `last index wins a tie` or under `second = the other candidate of
    equal distance`.  Scenarios with the same index order state the same outcome whatever their placement."""
    by_order = {}
    for s in SCAN:
        cands, _ = L.SCAN_SETS[s.set_name]
        seq = [(k, *cands[c]) for c, k in zip(s.order, s.idx)]
        winner, best, second = s.table
        want = s.idx[s.order.index(winner)] if winner else None
        assert L.reference_scan(seq, s.nnratio) == want, s.name
        n_e, m_e = s.expected("map")
        assert (n_e, {int(k): int(v) for k, v in enumerate(m_e) if v >= 0}) == ((1, {want: 0}) if winner else (0, {})), s.name
        wrong = {L.reference_scan(seq, s.nnratio, tie_last=True), L.reference_scan(seq, s.nnratio, second_other=True)}
        assert wrong != {want}, s.name
        # best / second of the table: the first minimum, and the first minimum of the rest
        ds = sorted(seq, key=lambda c: (c[1], c[0]))
        assert (ds[0][0], ds[1][0]) == (s.idx[s.order.index(best)], s.idx[s.order.index(second)]), s.name
        by_order.setdefault((s.set_name, s.order), set()).add(winner)
    assert len(by_order) == 18 and all(len(v) == 1 for v in by_order.values())


def test_float_boundaries_are_where_they_are_claimed():
    f = F32
    sc = scale_factors()
    # radius: (3, 4) at r = 5 is on `distance > r * r`, the next float is beyond; level 1 has a rounded r * r
    assert L.area_gates(90, 100, 110, 100, 5.0, 103.0, 104.0, 0.0)[0]
    assert not L.area_gates(90, 100, 110, 100, 5.0, 103.0, ulp_above(104.0), 0.0)[0]
    r1 = f(f(5.0) * sc[1])
    r2 = f(f(5.0) * sc[2])
    assert WINDOW.edges["r1"] == float(r1) == 6.0 and float(f(5.0)) * float(sc[1]) != 6.0        # 5 * 1.2f rounds to 6.0f
    assert WINDOW.edges["r2"] == float(r2) and float(f(r2 * r2)) != float(r2) * float(r2)        # r * r rounded in float
    assert L.radius_edge(100.0, r1)[0] == 106.0
    for r in (r1, r2):
        y_in, y_out = L.radius_edge(100.0, r)
        assert y_out == ulp_above(y_in) and L.area_gates(0, 100, 0, 100, r, 0, y_in, 0)[0] and not L.area_gates(0, 100, 0, 100, r, 0, y_out, 0)[0]
    # slope: float(0.05) is above the double 0.05 (= 5.0f * 0.01), the float below passes
    s_in, s_out = WINDOW.edges["s0"]
    assert s_out == float(f(0.05)) and s_in == ulp_below(0.05) and s_out > 5.0 * 0.01 >= s_in
    s_in, s_out = WINDOW.edges["s1"]
    assert s_out == ulp_above(s_in) and s_out > float(r1) * 0.01 >= s_in
    with np.errstate(all="ignore"):
        assert f(20.0) / f(0.0) == np.inf and f(-20.0) / f(0.0) == -np.inf and np.isnan(f(0.0) / f(0.0))
        assert np.isnan(f(f(512.0) * f(0.0)) * (f(1.0) / f(0.0)))              # fx * 0 * (1 / 0)
    # motion flags: strict comparisons with mb = bf / fx
    assert float(L.MB) == float(f(51.2)) / 512.0
    for name, tz, mono, mode in L.MOTIONS:
        fwd, bwd = (f(tz) > L.MB) and not mono, (-f(tz) > L.MB) and not mono
        assert ("fwd" if fwd else "bwd" if bwd else "none") == mode, name
    assert {m[1] for m in L.MOTIONS} >= {float(L.MB), ulp_above(L.MB), -float(L.MB), -ulp_above(L.MB)}
    # ratio test: the float product is the integer, the pairs straddle it
    for s in THRESH:
        assert len(s.pairs) == 4
        for p, d2 in s.pairs:
            assert p + 1 < d2
            assert f(f(s.nnratio) * f(d2)) == f(p) and not f(p) > f(f(s.nnratio) * f(d2)) and f(p + 1) > f(f(s.nnratio) * f(d2))
    assert float(f(0.9)) * 10 < 9.0                                              # accepted in float, rejected in double
    # bands and cone
    assert f(f(0.8) * f(2.5)) == f(2.0) and f(f(1.2) * f(2.5)) == f(3.0)
    assert ulp_below(0.5) * 2.0 < 1.0 == 0.5 * 2.0
    # 1.0f / 1.5f
    m = f(1.0) / f(1.5)
    for a, b in ((2, 3), (20, 30), (40, 60)):
        assert float(f(a) / f(b)) == float(m)
    assert float(f(19) / f(30)) < float(m)
    # image bounds: the projections of the bound cases are the bounds, and the first float outside them
    uv = FRUSTUM.uv
    assert uv["u1_min_on"][0][0] == 0.0 and uv["u2_max_on"][1][0] == 640.0 and uv["u1_max_on"][0][0] == 640.0
    assert uv["v1_min_on"][0][1] == 0.0 and uv["v2_max_on"][1][1] == 480.0 and uv["v2_min_on"][1][1] == 0.0
    assert uv["u2_max_out"][1][0] == ulp_above(640.0) and uv["u1_max_out"][0][0] == ulp_above(640.0)
    assert uv["v2_max_out"][1][1] == ulp_above(480.0)
    assert -2.0 ** -14 < uv["u1_min_out"][0][0] < 0 and -2.0 ** -14 < uv["v1_min_out"][0][1] < 0 and -2.0 ** -14 < uv["v2_min_out"][1][1] < 0
    for name, ((u1, v1), (u2, v2)) in uv.items():
        inside = [0 <= u1 <= 640, 0 <= v1 <= 480, 0 <= u2 <= 640, 0 <= v2 <= 480]
        assert all(inside) == name.endswith("_on") and sum(inside) >= 3, name


# ---------------------------------------------------------------------------------------------------------------------
# the oracle on the windowed scenarios

def _same(got, want, what):
    n_g, m_g = got
    n_e, m_e = want
    assert n_g == n_e, (what, n_g, n_e)
    bad = np.flatnonzero(m_g != m_e)
    assert bad.size == 0, (what, [(int(k), int(m_g[k]), int(m_e[k])) for k in bad[:8]])


@pytest.mark.parametrize("s", WINDOWED, **_ID)
def test_oracle_windowed(oracle_mod, s):
    if "map" in s.expect:
        _same(L.oracle_map(oracle_mod, s), s.expected("map"), "map")
    if "last" in s.expect:
        _same(L.oracle_last(oracle_mod, s), s.expected("last"), "last")
    if "fuse" in s.expect:
        for sim3 in (False, True):
            bi, bd = L.oracle_fuse(oracle_mod, s, sim3)
            ei, ed = s.expected_fuse()
            assert np.array_equal(bi, ei) and np.array_equal(bd, ed), (sim3, list(bi), list(ei))


def test_oracle_empty_lists(oracle_mod):
    s = L.sized(64)
    sc = s.scene
    n, m = oracle_mod.lsd_search_by_projection_map(scale_factors(), sc.tracked()[:0], sc.cur, sc.desc, 1.0, 0.9, s.cur_ml())
    assert n == 0 and (m == -1).all()
    n, m = oracle_mod.lsd_search_by_projection_map(scale_factors(), sc.tracked(), sc.cur[:0], sc.desc[:0], 1.0, 0.9, s.cur_ml()[:0])
    assert n == 0 and len(m) == 0
    I = np.eye(4, dtype=np.float32)
    n, m = oracle_mod.lsd_search_by_projection_last(L.cam9(), I, I, scale_factors(), sc.map_lines()[:0], sc.cur, sc.desc, 5.0, False, 0.9,
                                                    s.cur_ml())
    assert n == 0 and (m == -1).all()
    n, m = oracle_mod.lsd_search_by_projection_last(L.cam9(), I, I, scale_factors(), sc.map_lines(), sc.cur[:0], sc.desc[:0], 5.0, False,
                                                    0.9, s.cur_ml()[:0])
    assert n == 0 and len(m) == 0
    bi, bd = oracle_mod.lsd_fuse_search(L.cam9(), np.eye(4, dtype=np.float32), 1.2, scale_factors(), sc.frustum_lines(), sc.descs(),
                                        sc.skip(), sc.cur[:0], sc.desc[:0], 5.0)
    assert list(bi) == [-1]


# ---------------------------------------------------------------------------------------------------------------------
# projection gates, bands, cones, PredictScale

def test_frustum_inputs():
    f = FRUSTUM
    for c in f.named:
        assert hamming(f.descs[c.q], f.cur_desc[c.idx]) == c.dist
    D = f.descs[f.names.index("level_0")]
    for o in range(L.N_CENTRE):
        assert hamming(D, f.cur_desc[o]) == 30 - 2 * o and f.cur["octave"][o] == o
    # the zero-depth line scans every key line: none of octave 0 .. 1 but key line 1 is nearer than 30
    z = f.names.index("depth_zero")
    near = sorted((hamming(f.descs[z], f.cur_desc[k]), k) for k in range(len(f.cur)) if f.cur["octave"][k] <= 1)
    assert near[0] == (28, 1) and near[1] == (30, 0) and near[2][0] > 60
    # distance ratios of the hand-stated levels are far from a level boundary
    for n, l, lv in zip(f.names, f.lines, f.level):
        if lv is not None and n.startswith("level_"):
            x = np.log(float(l["max_distance"]) / 2.0) / np.log(1.2)
            assert abs(x - (lv - 0.5)) < 1e-5
    assert sum(lv is None for lv in f.level) == 11 and sum(fu is None for fu in f.fuse) == 9
    # the negative-level lines sit on the far edge of their band: dist == 1.2f * max, which `dist > maxDistance` keeps
    for mx in L.NEGATIVE_LEVEL_MAX:
        l = f.lines[f.names.index(f"level_neg_{mx}")]
        assert l["world"][2] == l["world"][5] == float(F32(F32(1.2) * l["max_distance"])) and l["max_distance"] == F32(mx)


def _frustum_oracle(orc):
    return orc.is_in_frustum_lines(L.cam9(), np.eye(4, dtype=np.float32), 1.2, FRUSTUM.lines, 0.5)


def test_oracle_frustum_lines(oracle_mod):
    """in_view of every line and the level of every line whose distance ratio is well inside a level, against the hand-stated
    values; the levels at exact products of the scale table (level None) are not stated by hand."""
    f = FRUSTUM
    o = _frustum_oracle(oracle_mod)
    assert list(o["in_view"]) == f.in_view
    for k, lv in enumerate(f.level):
        if lv is not None:
            assert o["level"][k] == lv, f.names[k]
    # the exact-ratio lines on the far band edge: the oracle must say -1 there (the Fuse expectation -2 rests on it), and 0 at 2.5
    for mx in L.NEGATIVE_LEVEL_MAX:
        assert o["level"][f.names.index(f"level_neg_{mx}")] == -1 and o["in_view"][f.names.index(f"level_neg_{mx}")] == 1, mx
    assert o["level"][f.names.index("band_max_on")] == 0
    z = f.names.index("depth_zero")
    assert np.isnan(o["x1"][z]) and np.isnan(o["y1"][z]) and (o["x2"][z], o["y2"][z]) == (320.0, 240.0)
    on = f.names.index("cone_on")
    assert o["view_cos"][on] == 0.5
    for name, ((u1, v1), (u2, v2)) in f.uv.items():
        if name.endswith("_on"):
            k = f.names.index(name)
            assert (o["x1"][k], o["y1"][k], o["x2"][k], o["y2"][k]) == (u1, v1, u2, v2), name


@pytest.mark.parametrize("sim3", [False, True])
def test_oracle_frustum_fuse(oracle_mod, sim3):
    f = FRUSTUM
    T = np.eye(4, dtype=np.float32)
    if sim3:
        T[:3, :] *= F32(2.0)
    fn = oracle_mod.lsd_fuse_search_sim3 if sim3 else oracle_mod.lsd_fuse_search
    bi, bd = fn(L.cam9(), T, 1.2, scale_factors(), f.lines, f.descs, np.zeros(len(f.lines), np.uint8), f.cur, f.cur_desc, 5.0)
    for k, fu in enumerate(f.fuse):
        if fu is not None:
            assert bi[k] == fu, (f.names[k], int(bi[k]), fu)
            if fu >= 0:
                assert bd[k] == hamming(f.descs[k], f.cur_desc[fu])


def test_oracle_frustum_last(oracle_mod):
    f = FRUSTUM
    got = oracle_mod.lsd_search_by_projection_last(L.cam9(), np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), scale_factors(),
                                                   L.frustum_map_lines(f), f.cur, f.cur_desc, 5.0, False, 0.9,
                                                   np.full(len(f.cur), -1, np.int32))
    want = np.full(len(f.cur), -1, np.int32)
    for k, q in f.last_expect[1].items():
        want[k] = q
    _same(got, (f.last_expect[0], want), "last")


# ---------------------------------------------------------------------------------------------------------------------
# keyframe entries

def test_oracle_search_by_projection_kf(oracle_mod):
    s = KF
    _named_ok(s.scene, 5.0, s.scene.named)
    for scale in (1.0, 2.0):
        T = np.eye(4, dtype=np.float32)
        T[:3, :] *= F32(scale)
        got = oracle_mod.lsd_search_by_projection_kf(L.cam9(), T, 1.2, scale_factors(), s.scene.frustum_lines(), s.scene.descs(),
                                                     s.scene.skip(), s.scene.cur, s.scene.desc, s.matched, 5)
        _same(got, s.expected(), "kf")


def test_oracle_search_by_sim3(oracle_mod):
    s = SIM3
    for d, ml, kl, dist in s.named:
        a, b = (s.descs1[ml], s.kd2[kl]) if d == "12" else (s.descs2[ml], s.kd1[kl])
        assert hamming(a, b) == dist
    k = s.names.index("u_max")
    assert L.project(*s.lines1["world"][k][3:])[0] == 640.0 and L.project(*s.lines2["world"][k][3:])[0] < 640.0
    assert L.project(*s.lines1["world"][s.names.index("u_min")][:3])[0] == 0.0
    pose, sides = L.sim3_args(s)
    _same(oracle_mod.lsd_search_by_sim3(L.cam9(), *pose, 1.2, scale_factors(), *sides, 5.0), s.expected(), "sim3")


# ---------------------------------------------------------------------------------------------------------------------
# descriptor matchers

def _knn_is(Q, T, rows):
    """the two nearest train rows of every query are at the stated distances, and the third is farther away"""
    d = np.array([[hamming(q, t) for t in T] for q in Q])
    for q, (d0, d1) in enumerate(rows):
        o = np.argsort(d[q], kind="stable")
        assert (d[q][o[0]], d[q][o[1]]) == (d0, d1) and (len(T) == 2 or d[q][o[2]] > d1), q
    return d


def test_oracle_ratio_rule(oracle_mod):
    Q, T, has, n_e, out_e, rows = L.ratio_rule()
    d = _knn_is(Q, T, rows)
    assert np.argmin(d[7]) == np.argmin(d[8]) == 14 and (d[4][8], d[4][9]) == (0, 0)
    n, out = oracle_mod.lsd_search_by_descriptor(Q, has, T)
    assert n == n_e and np.array_equal(out, out_e)
    n, out = oracle_mod.lsd_search_by_descriptor(Q, has, T[:1])
    assert n == 0 and list(out) == [-1]


@pytest.mark.parametrize("n", [1, 2, 4, 5])
def test_oracle_gap_rule(oracle_mod, n):
    Q, T, gaps, half, tenth = L.gap_rule(n)
    _knn_is(Q, T, [(5, 5 + g) for g in gaps])
    # the two readings of the gap median differ at n = 4, and the match with gap 10 flips between them
    g = np.array(gaps, float)
    desc_med, asc_med = np.sort(g)[::-1][n // 2], np.sort(g)[n // 2]
    th = lambda med: 0.5 * 1.4826 * np.sort(np.abs(g - med))[n // 2]
    assert [int(x > th(desc_med)) for x in g] == list(half)
    if n == 4:
        assert desc_med == 10 and asc_med == 22 and th(desc_med) < 10 < th(asc_med)
    got = oracle_mod.lsd_search_by_gap(Q, T)
    _same(got, L.gap_expected(n, half), "gap")
    has_t = np.ones(len(T), np.uint8)
    has_t[2 * (n - 1)] = 0                                # the train row of the last query carries no map line (:306-307)
    _same(oracle_mod.lsd_search_by_gap(Q, T, has_t), L.gap_expected(n, half, has_t), "gap, train mask")
    zeros1, zeros2 = np.zeros(n, np.uint8), np.zeros(len(T), np.uint8)
    _same(oracle_mod.lsd_search_for_triangulation(Q, T, zeros1, zeros2), L.gap_expected(n, tenth), "triangulation")
    # SearchForTriangulation skips a pair when EITHER line has a map line (:355): query 0 and the train row of the last query
    h1, h2 = zeros1.copy(), zeros2.copy()
    h1[0], h2[2 * (n - 1)] = 1, 1
    acc = [a and q != 0 and q != n - 1 for q, a in enumerate(tenth)]
    _same(oracle_mod.lsd_search_for_triangulation(Q, T, h1, h2), L.gap_expected(n, acc), "triangulation, masks")


@pytest.mark.parametrize("gap,accept", [(0, 0), (5, 1)])
def test_oracle_gap_rule_with_zero_mad(oracle_mod, gap, accept):
    Q, T = L.gap_rule_equal(gap)
    _knn_is(Q, T, [(5, 5 + gap)] * 3)
    _same(oracle_mod.lsd_search_by_gap(Q, T), L.gap_expected(3, [accept] * 3), "gap")
    _same(oracle_mod.lsd_search_for_triangulation(Q, T, np.zeros(3, np.uint8), np.zeros(6, np.uint8)), L.gap_expected(3, [accept] * 3), "tri")
    n, out = oracle_mod.lsd_search_by_gap(Q, T[:1])
    assert n == 0 and (out == -1).all()
