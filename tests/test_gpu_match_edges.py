"""-m gpu: the device's ORB matchers on the hand-built frames of match_scenarios.py, loaded with drfe_frame_load:
SearchByProjection(Cur, Last), SearchByProjection(F, MapPoints), Fuse (both overloads), SearchByProjection(pKF, Scw),
the relocalisation search, SearchForInitialization, MatchORBPoints and the brute-force k-NN.  Bar: match arrays and counts equal to the CPU oracle AND to the outcome
stated by hand from the reference source, with the orientation check on and off.

SearchByProjection(Cur, Last) runs through both entries: drfe_search_by_projection_last (host map points, pre-existing
claims) and drfe_match_consecutive_batch, the benchmark's path.  The batch path builds the map points itself from the last
slot's mvDepth and Twc (k_mappoints_last: valid = depth > 0, one observation each), so it is fed the way the pipeline
feeds it: frame_load with the oracle frame's mvuRight / mvDepth, slots [last A, cur A, last B, cur B, ...] with the
scenarios mixed in one call.  The pairs (cur A -> last B) in between have no map points (the current frames have no
depth) and must come out empty."""
import numpy as np
import pytest

import match_scenarios as ms

pytestmark = pytest.mark.gpu

LAST = ms.last_scenarios() + [ms.claim_chain()]


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(nfeatures=1500, max_batch=8)          # 1532 keypoints per slot: the 1200-point chain fits
    assert np.array_equal(c.scale_tables()[0], ms.scale_factors())
    yield c
    c.close()


def _cam():
    from dr_slam_amd import lib
    return lib.make_camera(ms.FX, ms.FY, ms.CX, ms.CY, ms.BF, 1.0, ms.W, ms.H)


def _load_pair(c, orc, s, cur_slot, last_slot, cam):
    cur, last, mp = ms.oracle_last(orc, s)
    c.frame_load(cur_slot, s.cur_kps, s.cur_desc.reshape(-1, 32), cam, kps_un=s.cur_kps_un, u_right=cur.uRight,
                 depth_m=cur.depth)
    c.frame_load(last_slot, s.last_kps, s.last_desc.reshape(-1, 32), cam, u_right=last.uRight, depth_m=last.depth)
    return cur, last, mp


def _gmp(mp):
    from dr_slam_amd import lib
    g = np.zeros(len(mp), lib.MAPPOINT_DTYPE)
    g["valid"], g["obs_positive"], g["world"], g["desc"] = mp["valid"], mp["obsPositive"], mp["world"], mp["desc"]
    return g


def _host_search(c, orc, s, check_ori, cam):
    cur, last, mp = _load_pair(c, orc, s, 0, 1, cam)
    return c.search_by_projection_last(0, 1, s.Tcw_cur, s.Tcw_last, cam, _gmp(mp), len(s.cur_kps), s.th, False, check_ori,
                                       s.pre, s.cur_obs)


def _check(s, check_ori, n_g, m_g, orc):
    n_o, m_o = ms.oracle_search_last(orc, s, check_ori)
    n_e, m_e = s.expected(check_ori)
    assert n_o == n_e and np.array_equal(m_o, m_e), "oracle"
    assert n_g == n_o, (n_g, n_o)
    bad = np.flatnonzero(m_g != m_o)
    assert bad.size == 0, [(int(k), int(m_g[k]), int(m_o[k])) for k in bad[:8]]


@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("s", LAST, ids=lambda s: s.name)
def test_search_last_host(ctx, oracle_mod, s, check_ori):
    n_g, m_g = _host_search(ctx, oracle_mod, s, check_ori, _cam())
    _check(s, check_ori, n_g, m_g, oracle_mod)


def _batches():
    """the scenarios the batch path can carry, grouped by th (one th per call), at most four per call"""
    by_th = {}
    for s in LAST:
        if not s.host_only:
            by_th.setdefault(s.th, []).append(s)
    out = []
    for th, ss in sorted(by_th.items()):
        for k in range(0, len(ss), 4):
            out.append((th, ss[k:k + 4]))
    return out


@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("group", _batches(), ids=lambda g: "+".join(s.name for s in g[1]))
def test_search_last_batch(ctx, oracle_mod, group, check_ori):
    th, ss = group
    cam = _cam()
    Tcw, Twc = [], []
    for k, s in enumerate(ss):
        _load_pair(ctx, oracle_mod, s, 2 * k + 1, 2 * k, cam)
        Tcw += [s.Tcw_last, s.Tcw_cur]
        Twc += [s.Twc_last, np.linalg.inv(s.Tcw_cur.astype(np.float64)).astype(np.float32)]
    ctx.match_consecutive_batch(np.stack(Tcw), np.stack(Twc), cam, th=th, mono=False, check_ori=check_ori,
                                nframes=2 * len(ss))
    for k, s in enumerate(ss):
        m_g, n_g = ctx.match_download(2 * k + 1)
        _check(s, check_ori, n_g, m_g[:len(s.cur_kps)], oracle_mod)
        if k:                                             # (cur of the previous scenario -> this last): no map points
            m_j, n_j = ctx.match_download(2 * k)
            assert n_j == 0 and (m_j[:len(s.last_kps)] == -1).all()


@pytest.mark.parametrize("s", ms.map_scenarios(), ids=lambda s: s.name)
def test_search_map(ctx, oracle_mod, s):
    """k_resolve_map's best / second and the float ratio test (src/ORBmatcher.cc:99-125)."""
    cam = _cam()
    fo = oracle_mod.FrameOracle(s.kps, s.desc, np.zeros((ms.H, ms.W), np.float32), ms.K4, ms.BF, ms.W, ms.H, ms.scale_factors())
    ctx.frame_load(0, s.kps, s.desc, cam, u_right=fo.uRight, depth_m=fo.depth)
    n_g, m_g = ctx.search_by_projection_map(0, s.tracked, len(s.kps), s.th, s.nnratio)
    n_o, m_o = ms.oracle_search_map(oracle_mod, s)
    n_e, m_e = s.expected()
    assert n_o == n_e and np.array_equal(m_o, m_e), "oracle"
    assert n_g == n_o and np.array_equal(m_g, m_o), (n_g, n_o, np.flatnonzero(m_g != m_o)[:8])


def test_capacity_4096(oracle_mod):
    """4096 map points, the most k_resolve_last holds, against a current frame at the slot's full size: nfeatures = 4064
    gives 4096 keypoints per slot (the level quotas plus four per level).  Both entries, orientation on and off."""
    from dr_slam_amd import lib
    c = lib.Context(nfeatures=4064, max_batch=2)
    try:
        assert c.max_kp == 4096
        s = ms.capacity(4096, 4096)
        cam = _cam()
        for check_ori in (False, True):
            n_g, m_g = _host_search(c, oracle_mod, s, check_ori, cam)
            _check(s, check_ori, n_g, m_g, oracle_mod)
            _load_pair(c, oracle_mod, s, 1, 0, cam)
            Twc_cur = np.linalg.inv(s.Tcw_cur.astype(np.float64)).astype(np.float32)
            c.match_consecutive_batch(np.stack([s.Tcw_last, s.Tcw_cur]), np.stack([s.Twc_last, Twc_cur]), cam, th=s.th,
                                      check_ori=check_ori, nframes=2)
            m_g, n_g = c.match_download(1)
            _check(s, check_ori, n_g, m_g[:4096], oracle_mod)
    finally:
        c.close()


def test_capacity_above_4096_is_a_stated_error(oracle_mod):
    """4097 map points: DRFE_ERR_CAPACITY with the reason, no partial result; the batch path refuses a context whose slots
    hold more than 4096 keypoints.  The context stays usable afterwards."""
    from dr_slam_amd import lib
    c = lib.Context(nfeatures=4065, max_batch=2)
    try:
        assert c.max_kp == 4097
        s = ms.capacity(4097, 4097)
        cam = _cam()
        cur, last, mp = _load_pair(c, oracle_mod, s, 0, 1, cam)
        pre = np.full(len(s.cur_kps), -1, np.int32)
        with pytest.raises(lib.DrfeError, match=r"\(-3\).*4096"):
            c.search_by_projection_last(0, 1, s.Tcw_cur, s.Tcw_last, cam, _gmp(mp), len(s.cur_kps), s.th, False, True, pre)
        with pytest.raises(lib.DrfeError, match=r"\(-3\).*4096"):
            Twc_cur = np.linalg.inv(s.Tcw_cur.astype(np.float64)).astype(np.float32)
            c.match_consecutive_batch(np.stack([s.Tcw_last, s.Tcw_cur]), np.stack([s.Twc_last, Twc_cur]), cam, th=s.th, nframes=2)
        # one point fewer in the last frame is within the limit on the same context
        t = ms.capacity(4096, 4097)
        n_g, m_g = _host_search(c, oracle_mod, t, True, cam)
        _check(t, True, n_g, m_g, oracle_mod)
    finally:
        c.close()


def _plain(c, orc, slot, kps, desc):
    cam = _cam()
    fo = orc.FrameOracle(kps, desc, np.zeros((ms.H, ms.W), np.float32), ms.K4, ms.BF, ms.W, ms.H, ms.scale_factors())
    c.frame_load(slot, kps, desc, cam, u_right=fo.uRight, depth_m=fo.depth)
    return fo


def test_keyframe_matchers(ctx, oracle_mod):
    """Fuse / Fuse(Scw) (raw best per point), SearchByProjection(pKF, Scw) at TH_LOW, the relocalisation search at ORBdist
    64 and 100 with and without the rotation check: the cross-cell tie (higher index first) and the thresholds +-1."""
    s = ms.keyframe_points()
    fo = _plain(ctx, oracle_mod, 0, s.kps, s.desc)
    inv_s2 = ctx.scale_tables()[3]
    T = np.eye(4, dtype=np.float32)
    n = len(s.pts)
    skip = np.zeros(n, np.uint8)
    for dev, orc in ((ctx.fuse_search, oracle_mod.fuse_search), (ctx.fuse_search_sim3, oracle_mod.fuse_search_sim3)):
        bi, bd = dev(0, T, s.pts, s.pdesc, skip, 3.0)
        obi, obd = orc(fo, T, 1.2, inv_s2, s.pts, s.pdesc, skip, 3.0)
        assert np.array_equal(bi, obi) and np.array_equal(bd, obd)
        assert list(bi) == s.winner and list(bd) == s.dist
    matched = np.zeros(len(s.kps), np.uint8)
    nm, new = ctx.search_by_projection_kf(0, T, s.pts, s.pdesc, skip, matched, 3.0)
    onm, onew = oracle_mod.search_by_projection_kf(fo, T, 1.2, 8, s.pts, s.pdesc, skip, matched, 3.0)
    e_n, e_new = ms.kf_expected_new(s, ms.TH_LOW)
    assert nm == onm == e_n and np.array_equal(new, onew) and np.array_equal(new, e_new)
    angles = np.zeros(n, np.float32)
    for orb_dist in (64, 100):
        for ori in (False, True):
            nm, new = ctx.search_by_projection_reloc(0, T, s.pts, s.pdesc, angles, skip, matched, 3.0, orb_dist, ori)
            onm, onew = oracle_mod.search_by_projection_reloc(fo, T, 1.2, 8, s.pts, s.pdesc, angles, skip, matched, 3.0, orb_dist, ori)
            e_n, e_new = ms.kf_expected_new(s, orb_dist)
            assert nm == onm == e_n, (orb_dist, ori, nm, onm, e_n)
            assert np.array_equal(new, onew) and np.array_equal(new, e_new), (orb_dist, ori)


@pytest.mark.parametrize("s", ms.init_scenarios(), ids=lambda s: s.name)
def test_search_for_initialization(ctx, oracle_mod, s):
    """`bestDist<=TH_LOW` and `bestDist<(float)bestDist2*mfNNratio` on the float boundary (src/ORBmatcher.cc:463-465)."""
    f1 = _plain(ctx, oracle_mod, 0, s.kps1, s.desc1)
    f2 = _plain(ctx, oracle_mod, 1, s.kps2, s.desc2)
    for ori in (False, True):
        n, m12, prev = ctx.search_for_initialization(0, 1, s.prev, 10, s.nnratio, ori)
        on, om12, oprev = oracle_mod.search_for_initialization(f1, f2, s.prev, 10, s.nnratio, ori)
        assert n == on == s.expect[0], (ori, n, on)
        assert np.array_equal(m12, om12) and np.array_equal(m12, s.expect[1]), ori
        assert np.array_equal(prev.view(np.uint32), oprev.view(np.uint32))


def test_match_orb_points_and_bf_ties(ctx, oracle_mod):
    """MatchORBPoints' max(2*min_dist, 15) threshold, its train-index tie and the good-match-counter outlier quirk
    (src/ORBmatcher.cc:1332-1394); cv::BFMatcher 2-NN ties in ascending train order."""
    cur, last, last_mp, outlier, n_e, out_e = ms.orb_points()
    kc = ms.kps_array([(20.0 + 30.0 * i, 50.0) for i in range(len(cur))])
    kl = ms.kps_array([(20.0 + 30.0 * i, 90.0) for i in range(len(last))])
    _plain(ctx, oracle_mod, 0, kc, cur)
    _plain(ctx, oracle_mod, 1, kl, last)
    n, out = ctx.match_orb_points(0, 1, last_mp, outlier, len(cur))
    on, oout = oracle_mod.match_orb_points(cur, last, last_mp, outlier)
    assert n == on == n_e and np.array_equal(out, oout) and np.array_equal(out, out_e)
    q, t, ei, ed = ms.bf_ties()
    for k in (1, 2):
        gi, gd = ctx.bf_knn(q[:2], t, k)
        oi, od = oracle_mod.bf_knn(q[:2], t, k)
        assert np.array_equal(gi, oi) and np.array_equal(gd, od)
        assert np.array_equal(gi, ei[:, :k]) and np.array_equal(gd, ed[:, :k])
    gi, gd = ctx.bf_knn(q[2:], t[:1], 2)
    oi, od = oracle_mod.bf_knn(q[2:], t[:1], 2)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od) and gi[0, 1] == -1
