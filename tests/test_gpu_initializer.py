"""-m gpu tests of the Initializer on the device: drfe_init_ransac_batch equals the host entry byte for byte
on every output at 0, 1, 2, 63, 64 and 65 solvers in one call, over the match counts at the sampling, wavefront and LDS boundaries,
on the planted and the degenerate scenes (those also against numpy), twice in a row on one context; the counters; on two frames of
the synthetic room the chain SearchForInitialization -> Initialize; and the native caller tests/native/initializer_caller.cpp
(Planar_SLAM::Initializer with the reference's signatures) against the ctypes path in both modes of the adaptor."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import initializer_numpy as inp  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    yield c
    c.close()


def _same(a, b, n):
    from dr_slam_amd import lib
    for s in range(n):
        diff = inp.differing(lib.init_table(a, s), lib.init_table(b, s))
        assert not diff, f"solver {s} differs in {diff}"


def _both(ctx, solvers):
    from dr_slam_amd import lib
    problems = inp.pack(solvers)
    host = lib.init_ransac_host(problems)
    dev = ctx.init_ransac_batch(problems)
    _same(dev, host, len(solvers))
    return dev


@pytest.fixture(scope="module")
def many():
    """65 small solvers of mixed size, key count and iteration count, the two planted successes among them"""
    rng = np.random.default_rng(3)
    sizes = (0, 7, 8, 9, 30, 63, 64, 65, 100)
    out = [inp.planted(rng, sizes[i % len(sizes)], planar=(i % 3 == 1), extra1=i % 4, extra2=(3 * i) % 5, max_iterations=(1, 2, 12)[i % 3],
                       seed=i) for i in range(63)]
    return out + [inp.planted_planar(20), inp.planted_general(200)]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65])
def test_device_equals_host_over_solver_counts(ctx, many, n):
    dev = _both(ctx, many[-n:] if n else [])
    if n == 65:
        assert (dev["hypotheses"] == 0).sum() >= 14 and dev["ok"].sum() >= 2
        assert (dev["branch"] == 1).any() and (dev["branch"] == 2).any()
    if n == 2:
        assert dev["ok"].tolist() == [1, 1] and dev["branch"].tolist() == [1, 2]


def test_device_equals_host_over_match_counts(ctx):
    """8 and 9: the sampling's end; 63, 64, 65, 128, 129: the wavefront and mask word boundaries; 300: the largest solver the other
    tests use.  With unmatched keys in both frames."""
    rng = np.random.default_rng(5)
    sizes = (8, 9, 63, 64, 65, 128, 129, 300)
    solvers = [inp.planted(rng, n, planar=bool(i & 1) and [0.6, -0.3, 1.0], baseline=0.8 if i & 1 else 0.35, extra1=3, extra2=1,
                           max_iterations=40, seed=50 + i) for i, n in enumerate(sizes)]
    dev = _both(ctx, solvers)
    assert dev["N"].tolist() == list(sizes)
    assert dev["motion_good"].max() >= 150 and dev["ok"].sum() >= 2


def test_device_equals_host_at_the_lds_bound_and_the_cap(ctx):
    """Beyond the 300 matches the other tests stop at, because two paths change only there: the scoring kernel keeps at most 2 048
    matches in LDS (2 048 and 2 049 matches), and a frame holds at most DRFE_INIT_MAX_KEYS keys (three below the cap with unmatched
    keys, and the cap itself).  Three iterations each keep the test short; little noise and few outliers let every sample give a model
    that CheckRT accepts nearly all matches under, so its ranking runs over thousands of cosines."""
    from dr_slam_amd import lib
    rng = np.random.default_rng(6)
    sizes = (lib.INIT_MAX_KEYS // 2, lib.INIT_MAX_KEYS // 2 + 1, lib.INIT_MAX_KEYS - 3)
    solvers = [inp.planted(rng, n, extra1=3, extra2=1, max_iterations=3, seed=60 + i, noise=0.02, outliers=0.05) for i, n in enumerate(sizes)]
    solvers.append(inp.planted(rng, lib.INIT_MAX_KEYS, max_iterations=3, seed=9, gaps=False, noise=0.02, outliers=0.05))
    dev = _both(ctx, solvers)
    assert dev["N"].tolist() == list(sizes) + [lib.INIT_MAX_KEYS]
    assert (dev["motion_good"].max(1) >= 1900).all() and dev["motion_good"].max() >= 3800 and dev["ok"].all()


def test_device_equals_numpy_on_degenerate_scenes(ctx):
    from dr_slam_amd import lib
    solvers = inp.degenerate_solvers(np.random.default_rng(23))
    dev = _both(ctx, list(solvers.values()))
    for s, (name, solver) in enumerate(solvers.items()):
        diff = inp.differing(lib.init_table(dev, s), inp.expected(solver))
        assert not diff, f"{name}: device and numpy differ in {diff}"
    flags = dict(zip(solvers, dev["flags"].tolist()))
    assert flags["identical"] == inp.H_DEGENERATE and flags["one_point"] == inp.NO_MODEL and flags["all_far"] == inp.NO_MODEL


def test_device_equals_numpy_on_planted_scenes(ctx):
    from dr_slam_amd import lib
    solvers = [inp.planted_planar(20), inp.planted(np.random.default_rng(1), 85, extra1=4, extra2=2, max_iterations=20, baseline=0.01),
               inp.planted(np.random.default_rng(64), 64, max_iterations=6, seed=64, gaps=False)]
    dev = _both(ctx, solvers)
    for s, solver in enumerate(solvers):
        assert not inp.differing(lib.init_table(dev, s), inp.expected(solver))
    assert dev["ok"].tolist() == [1, 0, 0]


def test_two_calls_in_a_row_on_one_context(ctx, many):
    """the second call reuses the first one's staging blocks: a smaller call after a larger one, then the larger one again"""
    big, small = many[20:50], many[3:6]
    a = _both(ctx, big)
    _both(ctx, small)
    b = _both(ctx, big)
    _same(a, b, len(big))


def test_stats_add_up(many):
    from dr_slam_amd import lib
    c = lib.Context(max_batch=1)
    try:
        assert set(c.init_stats().values()) == {0}
        solvers = many[:9] + many[-2:]
        r = c.init_ransac_batch(inp.pack(solvers))
        c.init_ransac_batch(inp.pack([]))
        st = c.init_stats()
        assert st["calls"] == 2 and st["solvers"] == 11 and st["matches"] == int(r["N"].sum()) == sum(int((s["matches12"] >= 0).sum()) for s in solvers)
        assert st["rows"] == int(r["hypotheses"].sum()) > 220 and st["empty"] == int((r["hypotheses"] == 0).sum()) == 2
        assert st["branch_h"] == int((r["branch"] == 1).sum()) and st["branch_f"] == int((r["branch"] == 2).sum())
        assert st["branch_h"] + st["branch_f"] + int((r["branch"] == 0).sum()) == 11 and st["ok"] == int(r["ok"].sum()) >= 2
    finally:
        c.close()


def test_chain_on_room_frames():
    """extract two frames, ORBmatcher::SearchForInitialization on the device, then Initialize of its vnMatches12 over every
    undistorted key of both frames through both entries: equal outputs.  No claim that the room initialises."""
    import torch
    from dr_slam_amd import lib, synth
    from dr_slam_amd.pipeline import FrontEnd
    frames = [next(synth.sequence(2, 1, start=k)) for k in (0, 3)]
    cam = synth.TUM3
    fe = FrontEnd(cam, max_batch=2)
    try:
        gray = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
        depth = torch.from_numpy(np.stack([f[1] for f in frames]).view(np.int16)).cuda()
        fe.process(gray, depth, None, None, stream=torch.cuda.current_stream().cuda_stream)
        c = fe.ctx
        kps0, _ = c.orb_download(0)
        kps1, _ = c.orb_download(1)
        un0, un1 = c.download_keys_un(0, len(kps0)), c.download_keys_un(1, len(kps1))
        prev = np.stack([un0["x"], un0["y"]], 1).astype(np.float32)
        nm, m12, _ = c.search_for_initialization(0, 1, prev, 100, 0.9, True)
        if nm < 8:
            pytest.skip(f"SearchForInitialization found {nm} matches on these frames: fewer than a sample")
        K = np.array([cam.fx, 0, cam.cx, 0, cam.fy, cam.cy, 0, 0, 1], np.float32)
        keys1 = prev[:lib.INIT_MAX_KEYS]
        keys2 = np.stack([un1["x"], un1["y"]], 1).astype(np.float32)[:lib.INIT_MAX_KEYS]
        m12 = np.where(m12[:len(keys1)] < len(keys2), m12[:len(keys1)], -1)
        s = dict(K=K, sigma=1.0, max_iterations=200, seed=0, keys1=keys1, keys2=keys2, matches12=m12)
        problems = inp.pack([s])
        dev = c.init_ransac_batch(problems)
        _same(dev, lib.init_ransac_host(problems), 1)
        t = lib.init_table(dev, 0)
        print(f"chain: {nm} matches of {len(keys1)} / {len(keys2)} keys, RH {t['RH']:.3f}, branch {t['branch']}, nGood {t['motion_good'].tolist()}, ok {t['ok']}")
        assert t["N"] == int((m12 >= 0).sum()) and t["hypotheses"] == 200
    finally:
        fe.ctx.close()


@pytest.mark.parametrize("mode", ("device", "auto", "host"))
@pytest.mark.parametrize("which", ("planar", "general", "short_baseline"))
def test_native_initialize_matches_ctypes(ctx, tmp_path, which, mode):
    """tests/native/initializer_caller.cpp: Planar_SLAM::Initializer(mInitialFrame, sigma, iterations) and its Initialize with the
    reference's signature, then MonocularInitialization's loop over vbTriangulated - forced to the device entry, `auto` (the adaptor's
    constant DRFE_INIT_DEVICE_FROM decides) and forced to the host entry - against the ctypes device path"""
    from dr_slam_amd import lib
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "initializer_caller")
    s = dict(planar=inp.planted_planar(20), general=inp.planted_general(200),
             short_baseline=inp.planted(np.random.default_rng(1), 85, extra1=4, extra2=2, max_iterations=20, baseline=0.01))[which]
    (tmp_path / "in.bin").write_bytes(inp.caller_blob(s))
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "initializer_caller ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    t = lib.init_table(ctx.init_ransac_batch(inp.pack([s])), 0)
    assert t["ok"] == (which != "short_baseline")
    assert (tmp_path / "out.bin").read_bytes() == inp.caller_expected(t, s)
