"""-m gpu tests of the PnP solver on the device: drfe_pnp_ransac_batch equals the host entry byte for byte at
0, 1, 2, 63, 64, 65 and 1 000 solvers in one call, over solver sizes up to the cap through both variants of the counting kernel, and
with refine jobs of 4, 5, 63, 64, 65, 1 000 and 4 096 points; the degenerate and planted scenes, also against numpy; the inlier sweep at Zc == 0; the counters;
on the synthetic room the chain SearchByBoW(KF, F) -> PnP -> the relocalisation SearchByProjection; and the native caller
tests/native/pnp_caller.cpp (Tracking::Relocalization's candidate loop over the adaptor) against the ctypes path."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_numpy as pn  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    yield c
    c.close()


def _same(got, want):
    diff = pn.tables_equal(got, want)
    assert not diff, f"tables differ in {diff}"


@pytest.fixture(scope="module")
def many():
    """1 000 small solvers of mixed size, iteration count and tail"""
    rng = np.random.default_rng(3)
    sizes = (0, 3, 4, 5, 19, 20, 21, 63, 64, 65, 40, 100)
    out = []
    for i in range(1000):
        N = sizes[i % len(sizes)]
        f, _ = pn.random_solver(rng, N, min_inliers=min(10, max(N - 1, 0)), max_iterations=(1, 5, 30)[i % 3], tail=(0, 5, 2)[i % 3],
                                seed=i, noise=0.3)
        out.append(f)
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1000])
def test_device_equals_host_over_solver_counts(ctx, many, n):
    from dr_slam_amd import lib
    problems = pn.pack(many[-n:] if n else [])
    host = lib.pnp_ransac_host(problems)
    _same(ctx.pnp_ransac_batch(problems), host)
    if n == 1000:
        assert host["returns"].sum() > 50 and (host["hypotheses"] == 0).sum() > 100 and host["refines"].max() >= 2


def test_device_equals_host_over_solver_sizes_and_both_variants(ctx):
    """N up to the cap: at most 2 048 correspondences are kept in LDS, more are read from global memory"""
    from dr_slam_amd import lib
    rng = np.random.default_rng(5)
    solvers = []
    for i, N in enumerate((1000, pn.LDS_CORR, pn.LDS_CORR + 1, 3000, pn.MAX_CORR)):
        f, _ = pn.random_solver(rng, N, min_inliers=10, max_iterations=(40, 12, 12, 9, 20)[i], tail=(5, 0, 3, 5, 5)[i], seed=50 + i,
                                noise=0.2)
        solvers.append(f)
    problems = pn.pack(solvers)
    before = ctx.pnp_stats()
    dev = ctx.pnp_ransac_batch(problems)
    after = ctx.pnp_stats()
    _same(dev, lib.pnp_ransac_host(problems))
    d = {k: after[k] - before[k] for k in after}
    assert d["solvers"] == 5 and d["solvers_global"] == 3 and d["solvers_empty"] == 0
    assert dev["returns"].any()


def test_refine_jobs_of_many_sizes(ctx):
    """scenes without an outlier and without noise: a good sample makes every correspondence an inlier, so Refine runs over all N"""
    from dr_slam_amd import lib
    rng = np.random.default_rng(13)
    sizes = (4, 5, 63, 64, 65, 1000, 4096)
    solvers = []
    for i, N in enumerate(sizes):
        for rep in range(3):
            solvers.append(pn.random_solver(rng, N, min_inliers=4, epsilon=0.5, max_iterations=8, tail=2, seed=100 + 7 * i + rep,
                                            outlier_frac=0.0)[0])
    problems = pn.pack(solvers)
    host = lib.pnp_ransac_host(problems)
    # a condition on the inputs: for every size some job runs over all N points, and there are many jobs
    for i, N in enumerate(sizes):
        full = False
        for s in range(3 * i, 3 * i + 3):
            t = lib.pnp_table(host, s)
            jobs = sorted(set(int(b) for b in t["best"] if b >= 0))
            full |= any(int(t["inliers"][b]) == N for b in jobs)
        assert full, N
    assert host["refines"].sum() >= 3 * len(sizes)
    before = ctx.pnp_stats()
    dev = ctx.pnp_ransac_batch(problems)
    after = ctx.pnp_stats()
    _same(dev, host)
    assert after["refine_jobs"] - before["refine_jobs"] == int(host["refines"].sum())
    assert after["refine_points"] - before["refine_points"] >= 4096


def test_device_equals_numpy_on_degenerate_scenes(ctx):
    from dr_slam_amd import lib
    problems = pn.pack(list(pn.degenerate_solvers(np.random.default_rng(23)).values()))
    dev = ctx.pnp_ransac_batch(problems)
    _same(dev, lib.pnp_ransac_host(problems))
    _same(dev, pn.table(problems))
    assert np.isnan(dev["R"]).any()


def test_device_sweep_at_zero_depth(ctx):
    """CheckInliers at Zc == 0 through the device's sweep (pnp_sweep, what k_pnp_count and k_pnp_refine run per row): 1 / 0 = +inf
    stored to float, fu * 0 * inf a NaN projection, and the comparison a NaN must fail - byte for byte the host's and numpy's; and
    on a planted scene under a perturbed pose, where both answers occur, at sizes on both sides of a wavefront"""
    from dr_slam_amd import lib
    R, t, K, p2d, Xw, me, kind = pn.zc_zero_case()
    want = pn.check_inliers(R, t, K, p2d, Xw, me)
    assert np.array_equal(want, kind == 0) and set(kind) == {0, 1, 2}
    assert np.array_equal(lib.pnp_inliers(R, t, K, p2d, Xw, me), want)
    assert np.array_equal(lib.pnp_inliers(R, t, K, p2d, Xw, me, ctx=ctx), want)
    for n in (1, 63, 64, 65, 132):
        assert np.array_equal(lib.pnp_inliers(R, t, K, p2d[:n], Xw[:n], me[:n], ctx=ctx), want[:n])
    f, truth = pn.random_solver(np.random.default_rng(41), 1000, outlier_frac=0.3, noise=1.0)
    Rp = (truth["R"] @ pn.rot([0, 1, 0], 2e-4)).reshape(9).tolist()
    tp = truth["t"].tolist()
    me = (f["sigma2"] * np.float32(5.991)).astype(np.float32)
    host = lib.pnp_inliers(Rp, tp, K, f["p2d"], f["Xw"], me)
    assert 100 < host.sum() < 900
    assert np.array_equal(lib.pnp_inliers(Rp, tp, K, f["p2d"], f["Xw"], me, ctx=ctx), host)
    assert np.array_equal(pn.check_inliers(Rp, tp, K, f["p2d"][:200], f["Xw"][:200], me[:200]), host[:200])


def test_planted_scene_on_the_device(ctx):
    from dr_slam_amd import lib
    rng = np.random.default_rng(33)
    f, truth = pn.random_solver(rng, 60, min_inliers=10, max_iterations=12, tail=5, seed=33, outlier_frac=0.3)
    problems = pn.pack([f])
    want = pn.table(problems)
    assert want["returns"].any()                       # a condition on the inputs
    dev = ctx.pnp_ransac_batch(problems)
    _same(dev, want)
    t = lib.pnp_table(dev, 0)
    h = int(np.argmax(t["returns"]))
    assert np.array_equal(pn.unpack_mask(t["refined_mask"][t["best"][h]], 60), truth["inliers"])


def test_stats_add_up():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    try:
        assert set(c.pnp_stats().values()) == {0}
        rng = np.random.default_rng(7)
        solvers = [pn.random_solver(rng, N, min_inliers=mi, max_iterations=7, tail=2, seed=N)[0]
                   for N, mi in ((30, 5), (10, 20), (2, 0), (2500, 20))]
        problems = pn.pack(solvers)
        r = c.pnp_ransac_batch(problems)
        c.pnp_ransac_batch(pn.pack([]))
        st = c.pnp_stats()
        assert st["calls"] == 2 and st["solvers"] == 4 and st["correspondences"] == 2542
        assert st["hypotheses"] == int(r["hypotheses"].sum()) > 0
        assert st["solvers_global"] == 1 and st["solvers_empty"] == 2
        assert st["refine_jobs"] == int(r["refines"].sum())
        pts = 0
        for s in range(4):
            t = lib.pnp_table(r, s)
            pts += sum(int(t["inliers"][b]) for b in set(int(b) for b in t["best"] if b >= 0))
        assert st["refine_points"] == pts
        _same(r, lib.pnp_ransac_host(problems))
    finally:
        c.close()


@pytest.fixture(scope="module")
def room():
    """a keyframe and a frame of the seed-2 room_boxes sequence"""
    from dr_slam_amd import synth
    return [next(synth.sequence(2, 1, start=k)) for k in (0, 6)]


def test_chain_on_room_frames(room):
    """extract, glue, BoW-transform, SearchByBoW(KF, F) on the device, the PnP table of the matches (device == host), the returned
    pose against the frame's true pose, then the relocalisation SearchByProjection under that pose"""
    import torch
    from dr_slam_amd import lib, synth, vocabulary as V
    from dr_slam_amd.pipeline import FrontEnd
    cam = synth.TUM3
    fe = FrontEnd(cam, max_batch=2)
    try:
        gray = torch.from_numpy(np.stack([f[0] for f in room])).cuda()
        depth = torch.from_numpy(np.stack([f[1] for f in room]).view(np.int16)).cuda()
        fe.process(gray, depth, None, None, stream=torch.cuda.current_stream().cuda_stream)
        c = fe.ctx
        voc = V.make_synthetic(10, 4, seed=5, stop_fraction=0.02)
        voc.upload(c)
        c.bow_transform_batch(2, 2)
        _, _, sigma2, _ = c.scale_tables()
        kps0, desc0 = c.orb_download(0)
        n0 = len(kps0)
        un0 = c.download_keys_un(0, n0)
        _, z = c.download_stereo(0)
        z = z[:n0]
        Twc0 = room[0][2].astype(np.float64)
        Pc = np.stack([(un0["x"] - cam.cx) * z / cam.fx, (un0["y"] - cam.cy) * z / cam.fy, z], 1).astype(np.float64)
        world = (Pc @ Twc0[:3, :3].T + Twc0[:3, 3]).astype(np.float32)          # a map point per keyframe keypoint with depth
        has = z > 0
        kps1, _ = c.orb_download(1)
        n1 = len(kps1)
        un1 = c.download_keys_un(1, n1)
        nm, m = c.search_by_bow(0, 1, np.where(has, np.arange(n0), -1), n1, 0.75, True)
        iF = np.flatnonzero(m >= 0)                                             # the constructor compacts in frame-keypoint order
        iK = m[iF]
        assert nm == len(iF) >= 15
        K = np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float32)
        f = dict(K=K, probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991, tail=5, seed=1,
                 p2d=np.stack([un1["x"][iF], un1["y"][iF]], 1), Xw=world[iK], sigma2=sigma2[un1["octave"][iF]])
        problems = pn.pack([f])
        dev = c.pnp_ransac_batch(problems)
        _same(dev, lib.pnp_ransac_host(problems))
        t = lib.pnp_table(dev, 0)
        assert t["returns"].any()
        h = int(np.argmax(t["returns"]))
        b = int(t["best"][h])
        Tcw1 = np.linalg.inv(room[1][2].astype(np.float64))
        assert np.allclose(t["refined_R"][b].reshape(3, 3), Tcw1[:3, :3], atol=3e-2)
        assert np.allclose(t["refined_t"][b], Tcw1[:3, 3], atol=8e-2)
        inl = pn.unpack_mask(t["refined_mask"][b], len(iF))
        # SearchByProjection(F, KF, sFound, 10, 100) over the map points the inliers leave free
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = t["refined_R"][b].reshape(3, 3)
        T[:3, 3] = t["refined_t"][b]
        matched = np.zeros(n1, np.uint8)
        matched[iF[inl]] = 1
        skip = ~has
        skip[iK[inl]] = True
        p = np.zeros(n0, lib.FRUSTUM_POINT_DTYPE)
        v = world.astype(np.float64) - Twc0[:3, 3]
        dist = np.linalg.norm(v, axis=1)
        ok = ~skip
        lvl = un0["octave"].astype(np.float64)
        p["world"][ok] = world[ok]
        p["normal"][ok] = (v[ok] / dist[ok, None]).astype(np.float32)
        p["min_distance"][ok] = (dist / 1.2 ** (7 - lvl) * 0.8)[ok]
        p["max_distance"][ok] = (dist * 1.2 ** lvl * 1.2)[ok]
        nf, new = c.search_by_projection_reloc(1, T, p, desc0, kps0["angle"], skip.astype(np.uint8), matched, 10.0, 100, True)
        print(f"chain: {len(iF)} BoW matches, {int(inl.sum())} PnP inliers, {nf} more by SearchByProjection")
        assert nf == (new >= 0).sum() and not (new[matched.astype(bool)] >= 0).any()
        assert len(set(new[new >= 0].tolist())) == nf and not skip[new[new >= 0]].any()
    finally:
        fe.ctx.close()


@pytest.mark.parametrize("mode", ("device", "auto"))
@pytest.mark.parametrize("verdicts", ((0, 0, 1), (0,) * 40), ids=("third", "none"))
def test_native_candidate_loop_matches_ctypes(ctx, tmp_path, verdicts, mode):
    """tests/native/pnp_caller.cpp: the candidate loop of Tracking::Relocalization over three candidates with the reference's
    signatures, the tables filled by one drfe::PnPBatch call - forced to the device, or `auto`: the batch's default threshold, which
    sends three solvers to the host entry - then find() of a fresh solver, against the walk over the ctypes device table"""
    from dr_slam_amd import lib
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "pnp_caller")
    blob, problems, indices, n_keys = pn.caller_scene(np.random.default_rng(61), verdicts)
    (tmp_path / "in.bin").write_bytes(blob)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "pnp_caller ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    problems["tail"][:] = pn.MAX_TAIL
    r = ctx.pnp_ransac_batch(problems)
    want, handed, past = pn.caller_expected([lib.pnp_table(r, s) for s in range(3)], indices, n_keys, verdicts)
    assert handed >= 3 and (tmp_path / "out.bin").read_bytes() == want
    if not any(verdicts):
        assert past
