"""CPU (-m "not gpu") tests of the Sim3 solver's host entry (drfe_sim3_ransac_host): the shared rand()
stream against this machine's libc, the whole hypothesis table byte for byte against the numpy restatement (tests/sim3_numpy.py) on
random, degenerate and planted scenes, iterate() as a walk over the table against the reference's loop run literally, the
correctly rounded double atan2 against mpmath, the refusals, the libm finish of a hypothesis that is not certified, and the native
caller tests/native/sim3_caller.cpp on the host entry."""
import ctypes
import os
import platform
import subprocess

import numpy as np
import pytest

import sim3_numpy as sn
from dr_slam_amd import lib

SEEDS = (0, 1, 2, 12345, 2 ** 31 - 1)


def _libc_rand(seed, n):
    libc = ctypes.CDLL(None)
    libc.srand.argtypes = [ctypes.c_uint]
    libc.rand.restype = ctypes.c_int
    libc.srand(seed)
    return np.array([libc.rand() for _ in range(n)], np.int64)


def _needs_glibc():
    if platform.libc_ver()[0] != "glibc":
        pytest.skip(f"the host's libc is {platform.libc_ver()[0] or 'unknown'}, not glibc: its rand() is another generator")


@pytest.mark.parametrize("seed", SEEDS)
def test_rand_stream_is_this_libc(seed):
    _needs_glibc()
    want = _libc_rand(seed, 1000)
    assert np.array_equal(lib.sim3_rand(seed, 1000), want)
    g = sn.GlibcRand(seed)
    assert np.array_equal([g.rand() for _ in range(1000)], want)


@pytest.mark.parametrize("seed", SEEDS)
def test_sample_triples_are_random_int_of_this_libc(seed):
    """the 900 draws of a 300-iteration solver, mapped through RandomInt and the swap-with-back list"""
    _needs_glibc()
    N = 50
    f, _ = sn.random_solver(np.random.default_rng(7), N, min_inliers=5, max_iterations=300, seed=seed)
    tab = lib.sim3_table(lib.sim3_ransac_host(sn.pack([f])), 0)
    assert tab["iterations"] == 300 and len(tab["sample"]) == 300
    draws = _libc_rand(seed, 900)
    want = np.zeros((300, 3), np.int32)
    for h in range(300):
        avail = list(range(N))
        for q in range(3):
            r = int((float(draws[3 * h + q]) / (2147483647.0 + 1.0)) * len(avail))
            want[h, q] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    assert np.array_equal(tab["sample"], want)
    assert np.array_equal(sn.sample_triples(seed, N, 300), want)


def _assert_same(problems, got=None):
    got = lib.sim3_ransac_host(problems) if got is None else got
    want = sn.table(problems)
    diff = sn.tables_equal(got, want)
    assert not diff, f"host table differs from the numpy restatement in {diff}"
    return got, want


@pytest.mark.parametrize("fix_scale", (False, True))
def test_host_table_equals_numpy_over_sizes(fix_scale):
    rng = np.random.default_rng(11 + fix_scale)
    solvers = []
    for i, N in enumerate((0, 2, 3, 19, 20, 21, 63, 64, 65)):
        f, _ = sn.random_solver(rng, N, fix_scale=fix_scale, min_inliers=min(20, max(N - 1, 0)), max_iterations=(1, 5, 12)[i % 3],
                                seed=100 + i, scale=1.3, noise=0.002)
        solvers.append(f)
    got, _ = _assert_same(sn.pack(solvers))
    assert list(got["hypotheses"][:2]) == [0, 0] and np.all(got["hypotheses"][2:] == got["iterations"][2:])


def test_host_table_equals_numpy_min_inliers_is_n():
    rng = np.random.default_rng(13)
    solvers = []
    for N in (3, 20, 64):
        f, _ = sn.random_solver(rng, N, min_inliers=N, max_iterations=300, seed=N, outlier_frac=0.0)
        solvers.append(f)
    got, _ = _assert_same(sn.pack(solvers))
    assert list(got["iterations"]) == [1, 1, 1] and list(got["hypotheses"]) == [1, 1, 1]


def test_host_table_equals_numpy_1000_correspondences_300_iterations():
    rng = np.random.default_rng(17)
    f, _ = sn.random_solver(rng, 1000, min_inliers=20, max_iterations=300, seed=9, scale=0.8, noise=0.001)
    g, _ = sn.random_solver(rng, 1000, fix_scale=True, min_inliers=20, max_iterations=300, seed=10, noise=0.001)
    got, _ = _assert_same(sn.pack([f, g]))
    assert list(got["iterations"]) == [300, 300]


def test_bounds_truncate_where_rounding_would_differ():
    """9.210 * sigma2 of the pyramid levels 1.2^(2 l): truncation and rounding give different integers at several levels, and an
    error between the two decides an inlier"""
    sig = ((np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32)
    prod = 9.210 * sig.astype(np.float64)
    assert np.any(np.floor(prod) != np.rint(prod))
    assert np.array_equal(sn.bound32(sig), np.floor(prod).astype(np.float32))
    rng = np.random.default_rng(19)
    f, _ = sn.random_solver(rng, 200, min_inliers=20, max_iterations=40, seed=21, noise=0.004)   # errors of a few px^2
    _assert_same(sn.pack([f]))


def test_degenerate_scenes_are_reproduced_not_special_cased():
    problems = sn.pack(sn.degenerate_solvers(np.random.default_rng(23)))
    got = lib.sim3_ransac_host(problems)
    want, proj = sn.table(problems, want_projections=True)
    assert not sn.tables_equal(got, want)
    # the table really holds a NaN hypothesis that is `best`, and the restatement really met an infinite projection
    nan_best = 0
    for s in range(3):
        t = lib.sim3_table(got, s)
        for h in range(len(t["best"])):
            b = t["best"][h]
            nan_best += bool(np.isnan(t["T12"][b]).any() and t["inliers"][b] == 0)
    assert nan_best > 0
    assert any(np.isinf(q).any() for pair in proj for q in pair)


def _planted(fix_scale, seed0):
    """a planted scene whose numpy table has a `returns` iteration within 300 (a condition on the inputs)"""
    rng = np.random.default_rng(seed0)
    for seed in range(seed0, seed0 + 20):
        f, truth = sn.random_solver(rng, 100, fix_scale=fix_scale, min_inliers=20, max_iterations=300, seed=seed, outlier_frac=0.3,
                                    scale=1.0 if fix_scale else 1.4)
        problems = sn.pack([f])
        want = sn.table(problems)
        if want["returns"].any():
            return problems, truth, want
    raise AssertionError("no planted scene with a returning iteration")


@pytest.mark.parametrize("fix_scale", (True, False))
def test_planted_scene_first_return_flags_the_planted_inliers(fix_scale):
    problems, truth, want = _planted(fix_scale, 31 + fix_scale)
    got = lib.sim3_ransac_host(problems)
    assert not sn.tables_equal(got, want)
    t = lib.sim3_table(got, 0)
    h = int(np.argmax(t["returns"]))
    assert t["returns"][h] == 1
    bits = np.unpackbits(t["mask"][h].view(np.uint8), bitorder="little")[:100].astype(bool)
    assert np.array_equal(bits, truth["inliers"])
    assert abs(float(t["s12"][h]) - truth["s"]) < 1e-3
    assert np.allclose(t["R12"][h].reshape(3, 3), truth["R"], atol=1e-3) and np.allclose(t["t12"][h], truth["t"], atol=5e-3)


def _run(solver, step):
    """the sequence of (T12, bNoMore, vbInliers, nInliers) until bNoMore, calling iterate(step) again after every return"""
    seq = []
    for _ in range(400):
        T, no_more, vb, n = solver.iterate(step)
        seq.append((None if T is None else np.asarray(T, np.float32).tobytes(), bool(no_more), vb.tobytes(), int(n)))
        if no_more:
            break
    return seq


def _walk_case(f, n1=None, indices1=None):
    problems = sn.pack([f])
    tab = lib.sim3_table(lib.sim3_ransac_host(problems), 0)
    N = len(f["sigma2_1"])
    a = _run(sn.TableWalker(tab, N, int(f["min_inliers"]), n1, indices1), 5)
    b = _run(sn.Solver(problems, 0, n1, indices1), 5)
    assert a == b
    Ta, va, na = sn.TableWalker(tab, N, int(f["min_inliers"]), n1, indices1).find()
    Tb, vb, nb = sn.Solver(problems, 0, n1, indices1).find()
    assert (Ta is None) == (Tb is None) and na == nb and np.array_equal(va, vb)
    if Ta is not None:
        assert np.asarray(Ta, np.float32).tobytes() == np.asarray(Tb, np.float32).tobytes()
    return a, tab


def test_walk_over_the_table_is_iterate():
    rng = np.random.default_rng(41)
    f, _ = sn.random_solver(rng, 60, min_inliers=20, max_iterations=37, seed=5, outlier_frac=0.3)
    idx = np.sort(rng.choice(90, 60, replace=False))           # mvnIndices1 into a longer vpMatched12
    seq, _ = _walk_case(f, 90, idx)
    assert any(s[0] is not None for s in seq) and seq[-1][1]
    # no hypothesis ever returns: bNoMore after the last round
    f, _ = sn.random_solver(rng, 40, min_inliers=10, max_iterations=11, seed=6, outlier_frac=0.8)
    seq, _ = _walk_case(f)
    assert all(s[0] is None for s in seq) and seq[-1][1] and len(seq) == 3


def test_walk_returns_at_the_very_last_iteration_without_no_more():
    rng = np.random.default_rng(43)
    f, _ = sn.random_solver(rng, 60, min_inliers=20, max_iterations=300, seed=8, outlier_frac=0.3)
    want = sn.table(sn.pack([f]))
    last = int(np.nonzero(want["returns"])[0][0])
    f["max_iterations"] = last + 1                             # the clamp keeps the count, so the table's prefix is the same
    assert sn.ransac_iterations(60, 0.99, 20, last + 1) == last + 1
    seq, tab = _walk_case(f)
    assert tab["returns"][last] == 1 and not tab["returns"][:last].any()
    returned = [s for s in seq if s[0] is not None]
    assert len(returned) == 1 and returned[0][1] is False      # handed back with bNoMore false ..
    assert seq[-1][0] is None and seq[-1][1] is True           # .. and only the next call says so


def test_walk_with_fewer_correspondences_than_min_inliers():
    f, _ = sn.random_solver(np.random.default_rng(47), 12, min_inliers=20, max_iterations=300, seed=2)
    seq, tab = _walk_case(f)
    assert seq == [(None, True, np.zeros(12, bool).tobytes(), 0)] and len(tab["inliers"]) == 0


def _atan2_sweep():
    rng = np.random.default_rng(53)
    y = [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 5e-324, 5e-324, 1e-310, 1.0, 2.0 ** -600, 1e-310, 3e-320, 1.0, np.inf, np.inf, 1.0]
    x = [0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 1.0, -1.0, 1e-310, 5e-324, -2.0 ** 600, -3e-310, 1e-310, 1e-310, 1.0, -np.inf, np.inf]
    # both signs of w over the unit disc a quaternion lives on, as floats widened and as full doubles
    ang = rng.uniform(0, np.pi, 4000)
    r = rng.uniform(0.2, 1.0, 4000)
    y += list((r * np.sin(ang)).astype(np.float32).astype(np.float64)) + list(r * np.sin(ang))
    x += list((r * np.cos(ang)).astype(np.float32).astype(np.float64)) + list(r * np.cos(ang))
    # 1 ulp steps either side of pi / 2: w around 0 in its smallest steps against norm = 1, and tiny ratios
    w = np.float32(0)
    for _ in range(20):
        w = np.nextafter(w, np.float32(1))
        y += [1.0, 1.0]
        x += [float(w), -float(w)]
    for e in range(-70, 0):
        y += [1.0, 2.0 ** e, 1.0]
        x += [2.0 ** e, 1.0, -(2.0 ** e)]
    v = 1e-17
    for _ in range(30):
        v = np.nextafter(v, 1.0)
        y += [1.0, 1.0]
        x += [v, -v]
    return np.array(y, np.float64), np.array(x, np.float64)


def test_double_atan2_is_correctly_rounded():
    import math
    y, x = _atan2_sweep()
    got, ok = lib.sim3_atan2(y, x)
    want = np.array([sn.cr_atan2(a, b) for a, b in zip(y, x)])
    cert = ok.astype(bool)
    # refusing is allowed only where the result is subnormal (a quotient there can sit on a rounding boundary)
    assert np.all(cert | (want < 2.0 ** -1022)), (y[~cert], x[~cert])
    assert got[cert].tobytes() == want[cert].tobytes()
    host = np.array([math.atan2(a, b) for a, b in zip(y, x)])
    print(f"atan2: {len(y)} arguments, {int((~cert).sum())} not certified, {int((host != want).sum())} last-bit differences of "
          f"the host's libm against mpmath")
    g, o = lib.sim3_atan2([np.nan, 1.0, -1.0], [1.0, np.nan, 1.0])
    assert np.isnan(g[0]) and np.isnan(g[1]) and list(o) == [1, 1, 0]


def test_invalid_shapes_are_refused():
    rng = np.random.default_rng(59)
    f, _ = sn.random_solver(rng, 30, seed=1)
    assert lib.sim3_ransac_host(sn.pack([]))["hypotheses"].size == 0
    for key, val in (("max_iterations", sn.MAX_ITERATIONS + 1), ("min_inliers", -1)):
        g = dict(f)
        g[key] = val
        with pytest.raises(lib.DrfeError):
            lib.sim3_ransac_host(sn.pack([g]))
    g = dict(f)
    g["sigma2_1"] = f["sigma2_1"].copy()
    g["sigma2_1"][3] = -1.0
    with pytest.raises(lib.DrfeError):
        lib.sim3_ransac_host(sn.pack([g]))
    g["sigma2_1"][3] = np.nan
    with pytest.raises(lib.DrfeError):
        lib.sim3_ransac_host(sn.pack([g]))
    big, _ = sn.random_solver(rng, sn.MAX_CORR + 1, seed=1, max_iterations=1)
    with pytest.raises(lib.DrfeError):
        lib.sim3_ransac_host(sn.pack([big]))
    p = sn.pack([f, f])
    p["offsets"] = np.array([0, 40, 30], np.int32)
    with pytest.raises(lib.DrfeError):
        lib.sim3_ransac_host(p)
    ok, _ = sn.random_solver(rng, sn.MAX_CORR, seed=1, max_iterations=2, min_inliers=20)
    assert lib.sim3_ransac_host(sn.pack([ok]))["hypotheses"][0] == 2


@pytest.mark.parametrize("fix_scale", (True, False))
def test_native_candidate_loop_on_the_host(tmp_path, fix_scale):
    """tests/native/sim3_caller.cpp without a device: Planar_SLAM::Sim3Solver's reference signatures over the host entry give what
    the walk over the ctypes table gives, through the adaptor's own compaction (bad, missing and unlisted map points)"""
    import native_build
    exe = native_build.caller("sim3_caller")          # built here if the tests directory holds no build products
    blob, problems, indices, n1 = sn.caller_scene(np.random.default_rng(61 + fix_scale), fix_scale)
    (tmp_path / "in.bin").write_bytes(blob)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "host"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "sim3_caller ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    r = lib.sim3_ransac_host(problems)
    walkers = [sn.TableWalker(lib.sim3_table(r, s), len(indices[s]), 20, n1, indices[s]) for s in range(3)]
    want, handed = sn.caller_expected(walkers)
    assert handed == 3
    assert (tmp_path / "out.bin").read_bytes() == want


def test_libm_finish_of_an_uncertified_hypothesis():
    """a hypothesis the core cannot certify is finished with the host's libm.  glibc's atan2 / sin / cos are within 1 ulp of a
    double, so after the rounding to float the two ways agree on almost every sample and differ by float rounding where not"""
    rng = np.random.default_rng(67)
    P1 = rng.uniform(-2, 2, (2000, 3, 3)).astype(np.float32)
    P2 = rng.uniform(-2, 2, (2000, 3, 3)).astype(np.float32)
    for fix in (0, 1):
        a, oka = lib.sim3_horn(P1, P2, fix, False)
        b, okb = lib.sim3_horn(P1, P2, fix, True)
        assert oka.all() and okb.all()
        same = (a.view(np.uint32) == b.view(np.uint32)).all(1)
        print(f"libm finish, fix_scale {fix}: {int(same.sum())} of {len(same)} samples identical")
        # a last-bit change of a double angle moves a float of magnitude <= 8 (|t| <= |O1| + s |O2|) by at most one float ulp
        assert same.mean() > 0.9 and np.allclose(a, b, rtol=2e-6, atol=2e-6)
