"""The CPU oracle of SearchByProjection(Cur, Last) and SearchByProjection(F, MapPoints) against the outcomes stated by hand
from the reference source for the adversarial frames of match_scenarios.py (ties, thresholds, window / grid edges, level
rules, rotation histogram, claims).  tests/test_gpu_match_edges.py holds the device to the same outcomes."""
import numpy as np
import pytest

import match_scenarios as ms

LAST = {s.name: s for s in ms.last_scenarios() + [ms.claim_chain()]}
MAP = {s.name: s for s in ms.map_scenarios()}


def test_scenarios_cite_the_reference():
    for s in list(LAST.values()) + list(MAP.values()):
        assert "src/ORBmatcher.cc" in s.ref or "src/Frame.cc" in s.ref, s.name


@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("name", sorted(LAST))
def test_oracle_search_last(oracle_mod, name, check_ori):
    s = LAST[name]
    n, m = ms.oracle_search_last(oracle_mod, s, check_ori)
    n_e, m_e = s.expected(check_ori)
    assert n == n_e, (n, n_e)
    assert np.array_equal(m, m_e), np.flatnonzero(m != m_e)[:10]


@pytest.mark.parametrize("name", sorted(MAP))
def test_oracle_search_map(oracle_mod, name):
    s = MAP[name]
    n, m = ms.oracle_search_map(oracle_mod, s)
    n_e, m_e = s.expected()
    assert n == n_e, (n, n_e)
    assert np.array_equal(m, m_e), np.flatnonzero(m != m_e)[:10]


def test_float_boundaries_are_where_they_are_claimed():
    """The edges the scenarios rely on, restated in numpy float32: PosInGrid's 4.5 (src/Frame.cc:817), the rotation bin's
    4.5 (src/ORBmatcher.cc:1505), 0.1f*max1 (:1698) and the ratio products (:121)."""
    f32 = np.float32
    inv = f32(64) / f32(640)
    assert f32(f32(45.0) * inv) == f32(4.5) and f32(f32(ms.ulp_below(45.0)) * inv) < f32(4.5)
    assert f32(f32(135.0) * (f32(1) / f32(30))) == f32(4.5)
    assert f32(f32(0.1) * f32(10)) == f32(1.0) and float(f32(0.1)) * 10 > 1.0
    assert f32(f32(0.9) * f32(10)) == f32(9.0) and float(f32(0.9)) * 10 < 9.0
    assert ms.ratio_accepts(0.9, 9, 10) and not ms.ratio_accepts(0.9, 10, 10)


def _kf_oracle(orc, s):
    fo = orc.FrameOracle(s.kps, s.desc, np.zeros((ms.H, ms.W), np.float32), ms.K4, ms.BF, ms.W, ms.H, ms.scale_factors())
    return fo


def test_oracle_keyframe_matchers(oracle_mod):
    """Fuse (raw best per point), SearchByProjection(pKF, Scw) at TH_LOW and the relocalisation search at ORBdist 64 / 100,
    against the hand-stated winners of match_scenarios.keyframe_points."""
    orc = oracle_mod
    s = ms.keyframe_points()
    fo = _kf_oracle(orc, s)
    inv_s2 = (1.0 / (ms.scale_factors() ** 2)).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    n = len(s.pts)
    skip = np.zeros(n, np.uint8)
    for fn in (orc.fuse_search, orc.fuse_search_sim3):
        bi, bd = fn(fo, T, 1.2, inv_s2, s.pts, s.pdesc, skip, 3.0)
        assert list(bi) == s.winner and list(bd) == s.dist
    matched = np.zeros(len(s.kps), np.uint8)
    nm, new = orc.search_by_projection_kf(fo, T, 1.2, 8, s.pts, s.pdesc, skip, matched, 3.0)
    assert (nm, list(new)) == (lambda e: (e[0], list(e[1])))(ms.kf_expected_new(s, ms.TH_LOW))
    angles = np.zeros(n, np.float32)
    for orb_dist in (64, 100):
        for ori in (False, True):
            nm, new = orc.search_by_projection_reloc(fo, T, 1.2, 8, s.pts, s.pdesc, angles, skip, matched, 3.0, orb_dist, ori)
            e_n, e_new = ms.kf_expected_new(s, orb_dist)
            assert nm == e_n and np.array_equal(new, e_new), (orb_dist, ori)


@pytest.mark.parametrize("s", ms.init_scenarios(), ids=lambda s: s.name)
def test_oracle_search_for_initialization(oracle_mod, s):
    sc = ms.scale_factors()
    z = np.zeros((ms.H, ms.W), np.float32)
    f1 = oracle_mod.FrameOracle(s.kps1, s.desc1, z, ms.K4, ms.BF, ms.W, ms.H, sc)
    f2 = oracle_mod.FrameOracle(s.kps2, s.desc2, z, ms.K4, ms.BF, ms.W, ms.H, sc)
    for ori in (False, True):
        n, m12, _ = oracle_mod.search_for_initialization(f1, f2, s.prev, 10, s.nnratio, ori)
        assert n == s.expect[0] and np.array_equal(m12, s.expect[1]), ori


def test_oracle_match_orb_points_and_bf_ties(oracle_mod):
    cur, last, last_mp, outlier, n_e, out_e = ms.orb_points()
    n, out = oracle_mod.match_orb_points(cur, last, last_mp, outlier)
    assert n == n_e and np.array_equal(out, out_e)
    q, t, ei, ed = ms.bf_ties()
    idx, dist = oracle_mod.bf_knn(q[:2], t, 2)
    assert np.array_equal(idx, ei) and np.array_equal(dist, ed)
    idx, dist = oracle_mod.bf_knn(q[2:], t[:1], 2)
    assert idx[0, 1] == -1
