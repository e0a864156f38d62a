"""-m gpu: the device's bag-of-words path on the hand-built vocabularies and frames of bow_scenarios.py, loaded with
drfe_frame_load: the vocabulary descent (k_bow_transform) through drfe_bow_transform_slot and drfe_bow_transform_batch,
SearchByBoW in both overloads (k_bow_match_groups, k_bow_rot_filter) and SearchForTriangulation
(k_bow_triangulation_groups).  Bar: identical word ids, weights, node ids and match arrays to the CPU oracle AND to the
outcome stated by hand.  Also: the upload's limits, one ORB-SLAM-shaped case (k = 10, L = 6, levelsup 4 on real frames),
and the rule that a slot whose descriptors were rewritten has no words until it is transformed again."""
import numpy as np
import pytest

import bow_scenarios as bs

pytestmark = pytest.mark.gpu

DESCENT = {s.name: s for s in bs.descent_scenarios()}
MTREE, MATCH_LIST = bs.match_scenarios()
MATCH = {s.name: s for s in MATCH_LIST}
TTREE, TRI_LIST = bs.tri_scenarios()
TRI = {s.name: s for s in TRI_LIST}
MODES = ["slot", "batch"]


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(nfeatures=1000, max_batch=4)
    assert np.array_equal(c.scale_tables()[0], bs.scale_tables()[0])
    assert np.array_equal(c.scale_tables()[2], bs.scale_tables()[1])
    yield c
    c.close()


def _cam():
    from dr_slam_amd import lib
    return lib.make_camera(bs.FX, bs.FY, bs.CX, bs.CY, 25.6, 1.0, bs.W, bs.H)


def _dummy_kps(n):
    k = np.zeros(n, bs.KP_DTYPE)
    k["x"], k["y"] = 20.0 + 10 * (np.arange(n) % 60), 20.0 + 10 * (np.arange(n) // 60)
    k["size"], k["response"], k["class_id"] = 31.0, 1.0, -1
    return k


def _transform(c, levelsup, slots, mode):
    if mode == "slot":
        for s in slots:
            c.bow_transform_slot(levelsup, s)
    else:
        c.bow_transform_batch(levelsup, max(slots) + 1)


def _state_error(fn):
    from dr_slam_amd import lib
    with pytest.raises(lib.DrfeError, match=r"failed \(-4\)"):
        fn()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(DESCENT))
def test_descent(ctx, oracle_mod, name, mode):
    s = DESCENT[name]
    c, cam = ctx, _cam()
    s.tree.voc.upload(c)
    ov = oracle_mod.VocabularyOracle(s.tree.text)
    n = len(s.desc)
    c.frame_load(0, _dummy_kps(n), s.desc, cam)
    c.frame_load(1, _dummy_kps(n), s.desc[::-1].copy(), cam)          # a second slot, features in reverse order
    for levelsup in s.levelsups:
        _transform(c, levelsup, [0, 1], mode)
        ew, ewt, enid = s.expected(levelsup)
        enid = np.array([0 if e is None else e for e in enid], np.int32)  # the product's choice where the reference leaves nid unset
        ow, owt, onid = ov.transform_each(s.desc, levelsup)
        for slot, order in ((0, slice(None)), (1, slice(None, None, -1))):
            w, wt, nid = c.bow_download(slot)
            assert np.array_equal(w[:n], ew[order]), (levelsup, slot, [s.why[i] for i in np.flatnonzero(w[:n][order] != ew)])
            assert np.array_equal(wt[:n].view(np.uint64), ewt[order].view(np.uint64))
            assert np.array_equal(nid[:n], enid[order]), (levelsup, slot)
            assert np.array_equal(w[:n], ow[order]) and np.array_equal(nid[:n], onid[order])


def test_upload_rejects_33_children_and_mismatched_leaf_flags(ctx):
    """33 children exceed the 32-lane descent step; a leaf flag that disagrees with the children is not a DBoW2 file (the
    reference would give an internal childless node word_id 0).  A rejected upload keeps the previous vocabulary."""
    from dr_slam_amd import lib
    c, cam = ctx, _cam()
    good, inner_childless, leaf_with_children = bs.leaf_flag_mismatch()
    good.upload(c)
    c.frame_load(0, _dummy_kps(3), good.desc[[1, 3, 4]], cam)
    c.bow_transform_slot(0, 0)
    before = c.bow_download(0)
    with pytest.raises(lib.DrfeError, match="more than 32 children"):
        bs.wide33_tree().voc.upload(c)
    with pytest.raises(lib.DrfeError, match="flagged internal but has no children"):
        inner_childless.upload(c)
    with pytest.raises(lib.DrfeError, match="flagged a leaf but has children"):
        leaf_with_children.upload(c)
    c.bow_transform_slot(0, 0)
    after = c.bow_download(0)
    assert all(np.array_equal(a[:3], b[:3]) for a, b in zip(before, after))
    assert list(after[0][:3]) == [0, 1, 2]


def _load_match(c, s):
    cam = _cam()
    kk, dk, mpk, _ = s.kf.arrays()
    kf, df, mpf, _ = s.f.arrays()
    c.frame_load(0, kk, dk, cam)
    c.frame_load(1, kf, df, cam)
    return kk, dk, mpk, kf, df, mpf


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("overload", ["frame", "kf"])
@pytest.mark.parametrize("name", sorted(MATCH))
def test_search_by_bow(ctx, oracle_mod, name, overload, check_ori, mode):
    s = MATCH[name]
    c = ctx
    MTREE.voc.upload(c)
    kk, dk, mpk, kf, df, mpf = _load_match(c, s)
    _transform(c, bs.MATCH_LEVELSUP, [0, 1], mode)
    ov = oracle_mod.VocabularyOracle(MTREE.text)
    _, wk, nk = ov.transform_each(dk, bs.MATCH_LEVELSUP)
    _, wf, nf = ov.transform_each(df, bs.MATCH_LEVELSUP)
    nk, nf = np.where(wk > 0, nk, -1), np.where(wf > 0, nf, -1)
    if overload == "frame":
        n_o, m_o = oracle_mod.search_by_bow(nk, nf, dk, kk["angle"], mpk, df, kf["angle"], s.nnratio, check_ori)
        n_g, m_g = c.search_by_bow(0, 1, mpk, len(df), s.nnratio, check_ori)
    else:
        n_o, m_o = oracle_mod.search_by_bow_kf(nk, nf, dk, kk["angle"], mpk, df, kf["angle"], mpf, s.nnratio, check_ori)
        n_g, m_g = c.search_by_bow_kf(0, 1, mpk, mpf, s.nnratio, check_ori)
    n_e, m_e = s.expected_array(overload, check_ori)
    assert n_o == n_e and np.array_equal(m_o, m_e), "oracle"
    assert n_g == n_e, (n_g, n_e)
    assert np.array_equal(m_g, m_e), [(i, m_g[i], m_e[i]) for i in np.flatnonzero(m_g != m_e)[:8]]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("only_stereo", [False, True])
@pytest.mark.parametrize("name", sorted(TRI))
def test_search_for_triangulation(ctx, oracle_mod, name, only_stereo, check_ori, mode):
    s = TRI[name]
    c, cam = ctx, _cam()
    TTREE.voc.upload(c)
    k1, d1, mp1, ur1 = s.k1.arrays()
    k2, d2, mp2, ur2 = s.k2.arrays()
    c.frame_load(0, k1, d1, cam, u_right=ur1)
    c.frame_load(1, k2, d2, cam, u_right=ur2)
    _transform(c, bs.MATCH_LEVELSUP, [0, 1], mode)
    ov = oracle_mod.VocabularyOracle(TTREE.text)
    kfs = []
    for k, d, mp, ur in ((k1, d1, mp1, ur1), (k2, d2, mp2, ur2)):
        _, w, nid = ov.transform_each(d, bs.MATCH_LEVELSUP)
        kfs.append(dict(x=k["x"], y=k["y"], angle=k["angle"], u_right=ur, octave=k["octave"], mp=mp,
                        nid=np.where(w > 0, nid, -1), desc=d))
    scale, sigma2 = bs.scale_tables()
    T2w = np.eye(4, dtype=np.float32)
    C2 = s.Cw1
    ex = np.float32(np.float32(np.float32(bs.FX) * C2[0]) * (np.float32(1) / C2[2])) + np.float32(bs.CX)
    ey = np.float32(np.float32(np.float32(bs.FY) * C2[1]) * (np.float32(1) / C2[2])) + np.float32(bs.CY)
    n_o, m_o = oracle_mod.search_for_triangulation(kfs[0], kfs[1], s.F12, ex, ey, scale, sigma2, only_stereo, check_ori)
    n_g, m_g = c.search_for_triangulation(0, 1, mp1, mp2, s.F12, s.Cw1, T2w, cam, only_stereo, check_ori)
    n_e, m_e = s.expected_array(only_stereo, check_ori)
    assert n_o == n_e and np.array_equal(m_o, m_e), "oracle"
    assert n_g == n_e and np.array_equal(m_g, m_e), (n_g, n_e, m_g, m_e)


def test_orbslam_shaped_vocabulary(frames_room, oracle_mod):
    """Frame::ComputeBoW's call on a full k = 10, L = 6 tree (1 111 111 nodes) with levelsup 4: words, weights and node ids
    of four real frames through both transform entries, then both SearchByBoW overloads on them."""
    import torch
    from dr_slam_amd import lib, vocabulary as V
    c = lib.Context(max_batch=4)
    try:
        gray = torch.from_numpy(np.stack([f[0] for f in frames_room])).cuda()
        c.orb_extract_batch_ptr(gray.data_ptr(), 640 * 480, 640, 640, 480, 4, 0)
        frames = [c.orb_download(s) for s in range(4)]
        voc = V.make_synthetic(10, 6, seed=3, stop_fraction=0.02)
        ov = oracle_mod.VocabularyOracle(voc.to_text())
        voc.upload(c)
        want = [ov.transform_each(d, 4) for _, d in frames]
        for mode in MODES:
            _transform(c, 4, [0, 1, 2, 3], mode)
            for s, (kps, _) in enumerate(frames):
                n = len(kps)
                w, wt, nid = c.bow_download(s)
                assert np.array_equal(w[:n], want[s][0]) and np.array_equal(nid[:n], want[s][2])
                assert np.array_equal(wt[:n].view(np.uint64), want[s][1].view(np.uint64))
        assert len(set(want[0][2])) > 20 and (want[0][1] == 0).any()
        rng = np.random.default_rng(4)
        nids = [np.where(w[1] > 0, w[2], -1) for w in want]
        (k0, d0), (k1, d1) = frames[0], frames[1]
        mp0 = np.where(rng.random(len(k0)) > 0.2, 1, -1).astype(np.int32)
        mp1 = np.where(rng.random(len(k1)) > 0.2, 1, -1).astype(np.int32)
        n_o, m_o = oracle_mod.search_by_bow(nids[0], nids[1], d0, k0["angle"], mp0, d1, k1["angle"], 0.7, True)
        n_g, m_g = c.search_by_bow(0, 1, mp0, len(k1), 0.7, True)
        assert n_g == n_o and np.array_equal(m_g, m_o) and n_o > 30
        n_o, m_o = oracle_mod.search_by_bow_kf(nids[0], nids[1], d0, k0["angle"], mp0, d1, k1["angle"], mp1, 0.75, True)
        n_g, m_g = c.search_by_bow_kf(0, 1, mp0, mp1, 0.75, True)
        assert n_g == n_o and np.array_equal(m_g, m_o) and n_o > 20
    finally:
        c.close()


# ----------------------------------------------------------------------------------------------------------------------
# stale words: every writer of a slot's descriptors drops the slot's words until it is transformed again

def _stale_checks(c, oracle_mod, ov, slots, levelsup, descs, both=False):
    """Every BoW call on a rewritten slot fails with DRFE_ERR_STATE; after a transform they agree with the oracle.
    both: slot b was rewritten too (a whole batch) - the searches keep failing until it is transformed as well."""
    a, b = slots
    n_a, n_b = len(descs[a]), len(descs[b])
    mp_a, mp_b = np.ones(n_a, np.int32), np.ones(n_b, np.int32)
    _state_error(lambda: c.bow_download(a))
    _state_error(lambda: c.search_by_bow(b, a, mp_b, n_a, 0.75, True))
    _state_error(lambda: c.search_by_bow_kf(a, b, mp_a, mp_b, 0.75, True))
    c.bow_transform_slot(levelsup, a)
    w, wt, nid = c.bow_download(a)
    ow, owt, onid = ov.transform_each(descs[a], levelsup)
    assert np.array_equal(w[:n_a], ow) and np.array_equal(nid[:n_a], onid)
    if both:
        _state_error(lambda: c.bow_download(b))
        _state_error(lambda: c.search_by_bow(b, a, mp_b, n_a, 0.75, True))
        c.bow_transform_slot(levelsup, b)
    ka, kb = [np.where(ov.transform_each(descs[s], levelsup)[1] > 0, ov.transform_each(descs[s], levelsup)[2], -1) for s in (a, b)]
    n_g, m_g = c.search_by_bow(b, a, mp_b, n_a, 0.75, False)
    n_o, m_o = oracle_mod.search_by_bow(kb, ka, descs[b], np.zeros(n_b, np.float32), mp_b, descs[a], np.zeros(n_a, np.float32),
                                        0.75, False)
    assert n_g == n_o and np.array_equal(m_g, m_o) and n_o > 10


@pytest.fixture(scope="module")
def stale_env(frames_room, oracle_mod):
    from dr_slam_amd import vocabulary as V
    voc = V.make_synthetic(10, 3, seed=9, stop_fraction=0.02)
    return voc, oracle_mod.VocabularyOracle(voc.to_text())


def test_stale_words_after_orb_extract_batch(frames_room, oracle_mod, stale_env):
    import torch
    from dr_slam_amd import lib
    voc, ov = stale_env
    c = lib.Context(max_batch=2)
    try:
        voc.upload(c)
        g = [torch.from_numpy(np.stack([frames_room[i][0] for i in idx])).cuda() for idx in ((0, 1), (2, 3))]
        c.orb_extract_batch_ptr(g[0].data_ptr(), 640 * 480, 640, 640, 480, 2, 0)
        c.bow_transform_batch(1, 2)
        c.orb_extract_batch_ptr(g[1].data_ptr(), 640 * 480, 640, 640, 480, 2, 0)      # same slots, new descriptors
        descs = [c.orb_download(s)[1] for s in range(2)]
        _stale_checks(c, oracle_mod, ov, (0, 1), 1, descs, both=True)
    finally:
        c.close()


def test_stale_words_after_orb_extract(frames_room, oracle_mod, stale_env):
    from dr_slam_amd import lib
    voc, ov = stale_env
    c = lib.Context(max_batch=2)
    try:
        voc.upload(c)
        k1 = c.orb_extract(frames_room[1][0])
        c.orb_extract(frames_room[2][0])                                                # slot 0 (and lastBatch 1)
        c.frame_load(1, *k1, _cam())
        c.bow_transform_slot(1, 0)
        c.bow_transform_slot(1, 1)
        _, d0 = c.orb_extract(frames_room[3][0])                                        # slot 0 rewritten
        _stale_checks(c, oracle_mod, ov, (0, 1), 1, [d0, k1[1]])
    finally:
        c.close()


def test_stale_words_after_frame_submit(frames_room, oracle_mod, stale_env):
    from dr_slam_amd import lib, synth
    voc, ov = stale_env
    cam = synth.TUM3
    camera = lib.make_camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.bf, cam.depth_factor, cam.w, cam.h)
    c = lib.Context(max_batch=2)
    try:
        voc.upload(c)
        for s in (0, 1):
            c.frame_submit(s, frames_room[s][0], frames_room[s][1], camera)
            c.frame_collect(s)
        c.bow_transform_batch(1, 2)
        c.frame_submit(0, frames_room[2][0], frames_room[2][1], camera)
        _, d0 = c.frame_collect(0)
        _stale_checks(c, oracle_mod, ov, (0, 1), 1, [d0, c.orb_download(1)[1]])
        # the tracked submission writes its slot too
        Tcw = [np.linalg.inv(f[2]).astype(np.float32) for f in frames_room]
        c.bow_transform_slot(1, 1)
        c.frame_submit_tracked(1, frames_room[3][0], frames_room[3][1], camera, 0, Tcw[3], Tcw[2],
                               Twc_last=frames_room[2][2].astype(np.float32))
        d1 = c.frame_collect_tracked(1)[1]
        _stale_checks(c, oracle_mod, ov, (1, 0), 1, [d0, d1])
    finally:
        c.close()


def test_stale_words_after_pipeline_submit(frames_room, oracle_mod, stale_env):
    import torch
    from dr_slam_amd import lib
    voc, ov = stale_env
    p = lib.Pipeline(1, max_batch=2)
    try:
        c = p.contexts[0]
        voc.upload(c)
        g = [torch.from_numpy(np.stack([frames_room[i][0] for i in idx])).cuda() for idx in ((0, 1), (3, 2))]
        p.sync(p.submit(g[0].data_ptr(), 0, 640 * 480, 640, 640, 480, None, None, None, nframes=2))
        c.bow_transform_batch(1, 2)
        p.sync(p.submit(g[1].data_ptr(), 0, 640 * 480, 640, 640, 480, None, None, None, nframes=2))
        descs = [c.orb_download(s)[1] for s in range(2)]
        _stale_checks(c, oracle_mod, ov, (0, 1), 1, descs, both=True)
    finally:
        p.close()


def test_stale_words_after_frame_load(frames_room, oracle_mod, stale_env):
    """drfe_frame_load already dropped the words; kept here with the other writers."""
    from dr_slam_amd import lib
    voc, ov = stale_env
    c = lib.Context(max_batch=2)
    try:
        voc.upload(c)
        k = [c.orb_extract(frames_room[i][0]) for i in range(3)]
        c.frame_load(0, *k[0], _cam())
        c.frame_load(1, *k[1], _cam())
        c.bow_transform_batch(1, 2)
        c.frame_load(0, *k[2], _cam())
        _stale_checks(c, oracle_mod, ov, (0, 1), 1, [k[2][1], k[1][1]])
    finally:
        c.close()
