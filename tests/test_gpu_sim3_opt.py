"""GPU tests of OptimizeSim3's device entry (drfe_sim3_opt_batch): the same bytes as the host entry and as
the numpy restatement (tests/sim3_opt_numpy.py) on the behaviour scenes, the match counts, random problems and every problem count
of a call; the caps; two calls on one context, the counters, the free-scale hand-over, the hand-back; the native caller; the loop
closer's chain on the synthetic room."""
import os
import subprocess

import numpy as np
import pytest

import sim3_opt_numpy as sn
from dr_slam_amd import lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context()
    yield c
    c.close()


def _both(ctx, problems):
    P = sn.pack(problems)
    return lib.sim3_opt_host(P), ctx.sim3_opt_batch(P)


@pytest.mark.parametrize("which", ("behaviour", "size", "random"))
def test_device_equals_host_and_the_restatement(ctx, which):
    problems = {"behaviour": lambda: list(sn.behaviour_problems().values()), "size": sn.size_problems,
                "random": sn.random_problems}[which]()
    assert max(len(p["index"]) for p in problems) <= 150 or which == "size"      # no problem above 300 edges but the sizes' own
    before = ctx.sim3_opt_stats()
    h, d = _both(ctx, problems)
    assert sn.tables_equal(d, h) == []
    assert sn.tables_equal(d, sn.numpy_table(which, problems)) == []
    after = ctx.sim3_opt_stats()
    assert after["handed_back"] == before["handed_back"]        # no seeded fixed-scale problem meets an argument the device cannot certify
    assert after["free_scale"] - before["free_scale"] == sum(1 for p in problems if not p["fix_scale"])


@pytest.mark.parametrize("n", (0, 1, 2, 63, 64, 65, 300))
def test_problems_per_call(ctx, n):
    problems = sn.mix_problems(n, seed=n, n=12)
    h, d = _both(ctx, problems)
    assert d["S12"].shape == (n, 8) and sn.tables_equal(d, h) == []


def test_caps(ctx):
    rng = np.random.default_rng(9)
    problems = [sn.problem(rng, lib.SIM3_OPT_MAX_MATCHES, outlier_frac=0.1), sn.problem(rng, 1000, outlier_frac=0.2)]
    h, d = _both(ctx, problems)
    assert sn.tables_equal(d, h) == [] and (d["returns"] > 700).all()
    with pytest.raises(lib.DrfeError, match="DRFE_SIM3_OPT_MAX_MATCHES"):
        ctx.sim3_opt_batch(sn.pack([sn.problem(rng, lib.SIM3_OPT_MAX_MATCHES + 1)]))
    with pytest.raises(lib.DrfeError, match="DRFE_SIM3_OPT_MAX_PROBLEMS"):
        ctx.sim3_opt_batch(sn.pack([sn.problem(rng, 3)] * (lib.SIM3_OPT_MAX_PROBLEMS + 1)))


def test_two_calls_counters_free_scale_and_hand_back():
    c = lib.Context()
    try:
        a = sn.mix_problems(7, seed=31, n=40)                    # problems 1 and 4 have a free scale
        b = sn.mix_problems(3, seed=32, n=15) + [sn.problem(np.random.default_rng(5), 6)]
        free_a = sum(1 for p in a if not p["fix_scale"])
        free_b = sum(1 for p in b if not p["fix_scale"])
        assert (free_a, free_b) == (2, 1)
        ha, hb = lib.sim3_opt_host(sn.pack(a)), lib.sim3_opt_host(sn.pack(b))
        da = c.sim3_opt_batch(sn.pack(a))
        db = c.sim3_opt_batch(sn.pack(b))                        # a smaller call after a larger one on the same buffers
        da2 = c.sim3_opt_batch(sn.pack(a))
        assert sn.tables_equal(da, ha) == [] and sn.tables_equal(db, hb) == [] and sn.tables_equal(da2, ha) == []
        st = c.sim3_opt_stats()
        assert st["calls"] == 3 and st["problems"] == 18 and st["free_scale"] == 2 * free_a + free_b
        assert st["matches"] == 2 * sum(len(p["index"]) for p in a) + sum(len(p["index"]) for p in b)
        assert st["early_returns"] == 1 and st["handed_back"] == 0
        assert st["iterations"] == 2 * int(ha["iterations"].sum()) + int(hb["iterations"].sum())
        assert st["trials"] == 2 * int(ha["trials"].sum()) + int(hb["trials"].sum())
        c.sim3_opt_hand_back(2)                                  # problems 0, 2, 4, 6 of which 4 has a free scale: three run again
        da3 = c.sim3_opt_batch(sn.pack(a))
        c.sim3_opt_hand_back(0)
        st = c.sim3_opt_stats()
        assert sn.tables_equal(da3, ha) == [] and st["handed_back"] == 3 and st["free_scale"] == 3 * free_a + free_b
    finally:
        c.close()


def _run_caller(tmp_path, blob, mode):
    exe = os.path.join(HERE, "native", "sim3_opt_caller")
    (tmp_path / "in.bin").write_bytes(blob)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "sim3_opt_caller ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    return p.stdout, (tmp_path / "out.bin").read_bytes()


def test_native_caller_matches_ctypes(ctx, tmp_path):
    """tests/native/sim3_opt_caller.cpp forced to the device: Planar_SLAM::Optimizer::OptimizeSim3 candidate by candidate (a device
    call each), then drfe::Sim3OptBatch over all candidates in one call, against the ctypes device path"""
    blob, problems = sn.caller_scene()
    out, got = _run_caller(tmp_path, blob, "device")
    assert "batch device calls 1, problems 4, handed back 0" in out, out
    assert got == sn.caller_expected(ctx.sim3_opt_batch(sn.pack(problems)), problems)


def test_native_caller_switches_to_the_device_at_the_threshold(tmp_path):
    """the caller in auto mode with DRFE_SIM3OPT_DEVICE_FROM candidates and with one fewer: the candidate-by-candidate Optimizer
    stays on the host entry, drfe::Sim3OptBatch goes to the device entry on its own at the threshold, and both write what the ctypes
    path writes"""
    for n, calls in ((lib.SIM3OPT_DEVICE_FROM, 1), (lib.SIM3OPT_DEVICE_FROM - 1, 0)):
        blob, problems = sn.caller_scene(n_cand=n, n_keys=60, seed=40 + calls)
        out, got = _run_caller(tmp_path, blob, "auto")
        assert f"batch device calls {calls}, problems {n * calls}," in out, out
        assert got == sn.caller_expected(lib.sim3_opt_host(sn.pack(problems)), problems)


def test_chain_on_room_keyframes():
    """LoopClosing::ComputeSim3's steps on the synthetic room, the current key frame against three candidates: SearchByBoW(KF, KF),
    the Sim3 tables of the three candidates by one drfe_sim3_ransac_batch, SearchBySim3 on the device with each best hypothesis,
    OptimizeSim3 of the three by one call, then SearchByProjection(current KF, Scw) with the Scw the entry returns over the
    candidate's map points.  Once with drfe_sim3_opt_batch, once with drfe_sim3_opt_host: the last matcher's output is the same,
    byte for byte."""
    import torch
    import sim3_numpy as s3
    from dr_slam_amd import synth, vocabulary as V
    from dr_slam_amd.pipeline import FrontEnd
    cam = synth.TUM3
    room = [next(synth.sequence(2, 1, start=k)) for k in (0, 10, 6, 14)]
    fe = FrontEnd(cam, max_batch=4)
    try:
        gray = torch.from_numpy(np.stack([f[0] for f in room])).cuda()
        depth = torch.from_numpy(np.stack([f[1] for f in room]).view(np.int16)).cuda()
        fe.process(gray, depth, None, None, stream=torch.cuda.current_stream().cuda_stream)
        c = fe.ctx
        V.make_synthetic(10, 4, seed=5, stop_fraction=0.02).upload(c)
        c.bow_transform_batch(4, 4)
        _, _, sigma2, inv_sigma2 = c.scale_tables()
        world, octave, desc, Tcw, has, un = [], [], [], [], [], []
        for s, (_, _, Twc) in enumerate(room):
            kps, d = c.orb_download(s)
            n = len(kps)
            u = c.download_keys_un(s, n)
            _, z = c.download_stereo(s)
            z = z[:n]
            Twc = Twc.astype(np.float64)
            Pc = np.stack([(u["x"] - cam.cx) * z / cam.fx, (u["y"] - cam.cy) * z / cam.fy, z], 1).astype(np.float64)
            world.append((Pc @ Twc[:3, :3].T + Twc[:3, 3]).astype(np.float32))     # a map point per keypoint with depth
            octave.append(u["octave"])
            desc.append(d)
            has.append(z > 0)
            un.append(u)
            Tcw.append(np.linalg.inv(Twc).astype(np.float32))
        mp = [np.where(h, np.arange(len(h)), -1) for h in has]
        K = np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float32)

        def frustum(s, skip):
            p = np.zeros(len(skip), lib.FRUSTUM_POINT_DTYPE)
            Ow = room[s][2].astype(np.float64)[:3, 3]
            v = world[s].astype(np.float64) - Ow
            dist = np.linalg.norm(v, axis=1)
            ok = ~skip
            p["world"][ok] = world[s][ok]
            p["normal"][ok] = (v[ok] / dist[ok, None]).astype(np.float32)
            lvl = octave[s].astype(np.float64)
            p["min_distance"][ok] = (dist / 1.2 ** (7 - lvl) * 0.8)[ok]
            p["max_distance"][ok] = (dist * 1.2 ** lvl * 1.2)[ok]
            return p
        pairs, solver = [], []
        for cand in (1, 2, 3):
            n, m2 = c.search_by_bow_kf(0, cand, mp[0], mp[cand], 0.75, True)
            i2 = np.flatnonzero(m2 >= 0)
            i1 = m2[i2]
            order = np.argsort(i1)
            i1, i2 = i1[order], i2[order]
            assert n == len(i1) > 30
            pairs.append((i1, i2))
            solver.append(dict(Tcw1=Tcw[0][:3].reshape(12), Tcw2=Tcw[cand][:3].reshape(12), K1=K, K2=K, fix_scale=1, probability=0.99,
                               min_inliers=20, max_iterations=300, seed=cand, Xw1=world[0][i1], Xw2=world[cand][i2],
                               sigma2_1=sigma2[octave[0][i1]], sigma2_2=sigma2[octave[cand][i2]]))
        tables = c.sim3_ransac_batch(s3.pack(solver))
        problems, matches = [], []
        for k, cand in enumerate((1, 2, 3)):
            i1, i2 = pairs[k]
            t = lib.sim3_table(tables, k)
            assert t["returns"].any()
            h = int(np.argmax(t["returns"]))
            inl = np.unpackbits(t["mask"][h].view(np.uint8), bitorder="little")[:len(i1)].astype(bool)
            m12 = np.full(len(mp[0]), -1, np.int32)
            m12[i1[inl]] = i2[inl]
            skip1 = (m12 >= 0) | ~has[0]
            skip2 = ~has[cand]
            skip2[m12[m12 >= 0]] = True
            nf, ms = c.search_by_sim3(0, cand, Tcw[0], Tcw[cand], float(t["s12"][h]), t["R12"][h], t["t12"][h], frustum(0, skip1), desc[0],
                                      skip1.astype(np.uint8), frustum(cand, skip2), desc[cand], skip2.astype(np.uint8), 7.5)
            m12[ms >= 0] = ms[ms >= 0]
            keep = np.flatnonzero(m12 >= 0)
            j = m12[keep]
            # g2o::Sim3 gScm(toMatrix3d(R), toVector3d(t), s): Quaterniond(R) as it is
            R = t["R12"][h].reshape(3, 3).astype(np.float64)
            q = sn.pon.quat_from_matrix([[float(R[r, cc]) for cc in range(3)] for r in range(3)])
            S12 = np.array(q + [float(v) for v in t["t12"][h]] + [float(t["s12"][h])], np.float64)
            problems.append(dict(S12=S12, K1=K, K2=K, R1w=Tcw[0][:3, :3].reshape(9), t1w=Tcw[0][:3, 3], R2w=Tcw[cand][:3, :3].reshape(9),
                                 t2w=Tcw[cand][:3, 3], th2=np.float32(10), fix_scale=np.uint8(1), index=keep.astype(np.int32),
                                 P3D1w=world[0][keep], P3D2w=world[cand][j],
                                 obs1=np.stack([un[0]["x"][keep], un[0]["y"][keep]], 1), obs2=np.stack([un[cand]["x"][j], un[cand]["y"][j]], 1),
                                 inv_sigma2_1=inv_sigma2[octave[0][keep]], inv_sigma2_2=inv_sigma2[octave[cand][j]]))
            matches.append(m12)
        P = sn.pack(problems)
        results = {"device": c.sim3_opt_batch(P), "host": lib.sim3_opt_host(P)}
        assert sn.tables_equal(results["device"], results["host"]) == []
        off = P["match_offsets"]
        last = {}
        for name, r in results.items():
            out = []
            for k, cand in enumerate((1, 2, 3)):
                assert r["returns"][k] >= 20
                # both maps are the same world: Scw is the current key frame's pose
                assert np.abs(r["Scw"][k].reshape(4, 4) - Tcw[0]).max() < 0.03
                m12 = matches[k].copy()
                m12[problems[k]["index"][r["outlier"][off[k]:off[k + 1]] != 0]] = -1
                matched = (m12 >= 0).astype(np.uint8)
                skip = ~has[cand]
                skip[m12[m12 >= 0]] = True                       # the candidate's map points already matched
                n2, new = c.search_by_projection_kf(0, r["Scw"][k], frustum(cand, skip), desc[cand], skip.astype(np.uint8), matched, 10.0)
                assert n2 == (new >= 0).sum()
                out.append((n2, new.tobytes(), matched.tobytes()))
            last[name] = out
        assert last["device"] == last["host"]
        print("chain:", [(len(p["index"]), int(results["device"]["returns"][k]), last["device"][k][0]) for k, p in enumerate(problems)])
    finally:
        fe.ctx.close()
