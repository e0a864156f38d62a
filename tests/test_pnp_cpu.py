"""CPU (-m "not gpu") tests of the PnP solver's host entry (drfe_pnp_ransac_host): the sample quadruples
against this machine's libc, the whole table byte for byte against the numpy restatement (tests/pnp_numpy.py) on random, planted and
degenerate scenes, iterate() as a walk over the table against the reference's `||` loop run literally, the refusals, and the double
Jacobi SVD as an SVD against numpy.linalg.svd."""
import ctypes
import platform

import numpy as np
import pytest

import pnp_numpy as pn
from dr_slam_amd import lib

# the largest difference of a singular value of tests/pnp_numpy.py's jacobi_svd from numpy.linalg.svd's, relative to the largest
# singular value, measured over the matrices of test_double_jacobi_svd_is_an_svd; the bound is four times it
SVD_MEASURED = 2.202e-15
SVD_BOUND = 4 * SVD_MEASURED


def _libc_rand(seed, n):
    libc = ctypes.CDLL(None)
    libc.srand.argtypes = [ctypes.c_uint]
    libc.rand.restype = ctypes.c_int
    libc.srand(seed)
    return np.array([libc.rand() for _ in range(n)], np.int64)


@pytest.mark.parametrize("seed", (0, 1, 2, 12345, 2 ** 31 - 1))
def test_sample_quadruples_are_random_int_of_this_libc(seed):
    """the 1 220 draws of a 300-iteration solver with a tail of 5, mapped through RandomInt and the swap-with-back list"""
    if platform.libc_ver()[0] != "glibc":
        pytest.skip(f"the host's libc is {platform.libc_ver()[0] or 'unknown'}, not glibc: its rand() is another generator")
    N = 50
    f, _ = pn.random_solver(np.random.default_rng(7), N, min_inliers=5, epsilon=0.1, max_iterations=300, tail=5, seed=seed)
    tab = lib.pnp_table(lib.pnp_ransac_host(pn.pack([f])), 0)
    assert tab["iterations"] == 300 and len(tab["sample"]) == 305
    draws = _libc_rand(seed, 4 * 305)
    want = np.zeros((305, 4), np.int32)
    for h in range(305):
        avail = list(range(N))
        for q in range(4):
            r = int((float(draws[4 * h + q]) / (2147483647.0 + 1.0)) * len(avail))
            want[h, q] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    assert np.array_equal(tab["sample"], want)
    assert np.array_equal(pn.sample_quads(seed, N, 305), want)


def _assert_same(problems, traces=None):
    got = lib.pnp_ransac_host(problems)
    want = pn.table(problems, traces)
    diff = pn.tables_equal(got, want)
    assert not diff, f"host table differs from the numpy restatement in {diff}"
    return got, want


def test_host_table_equals_numpy_over_sizes_min_inliers_is_n():
    rng = np.random.default_rng(11)
    sizes = (0, 3, 4, 5, 9, 10, 11, 63, 64, 65)
    solvers = [pn.random_solver(rng, N, min_inliers=N, max_iterations=300, tail=2, seed=100 + N, outlier_frac=0.0)[0] for N in sizes]
    got, _ = _assert_same(pn.pack(solvers))
    assert list(got["iterations"]) == [1] * len(sizes)
    assert list(got["hypotheses"]) == [0, 0] + [3] * (len(sizes) - 2)
    assert list(got["min_inliers"]) == [4, 4] + list(sizes[2:])
    assert got["returns"].sum() == 0                   # refined > N never holds


def test_host_table_equals_numpy_over_sizes_with_outliers():
    rng = np.random.default_rng(12)
    solvers = [pn.random_solver(rng, N, min_inliers=min(8, N), max_iterations=6, tail=2, seed=200 + N, noise=0.4)[0]
               for N in (4, 5, 9, 30, 63, 64, 65)]
    got, _ = _assert_same(pn.pack(solvers))
    assert got["returns"].any() and (got["refines"] > 0).sum() >= 2


def test_set_ransac_parameters():
    """SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991): N * epsilon in float, truncated; epsilon raised to minInliers / N"""
    solvers = [pn.random_solver(np.random.default_rng(N), N, min_inliers=10, max_iterations=300, epsilon=0.5, tail=0, seed=N)[0]
               for N in (9, 10, 15, 21, 30, 200)]
    got = lib.pnp_ransac_host(pn.pack(solvers))
    assert list(got["min_inliers"]) == [10, 10, 10, 10, 15, 100]
    assert list(got["hypotheses"]) == [0] + list(got["iterations"][1:])
    # epsilon = 10/15, then 0.5 (10/21 is below it): ceil(log(0.01) / log(1 - eps^3))
    assert list(got["iterations"]) == [1, 1, 14, 35, 35, 35]
    for s, f in enumerate(solvers):
        assert pn.ransac_parameters(len(f["p2d"]), 0.99, 10, 300, 0.5) == (got["min_inliers"][s], got["iterations"][s])


def test_planted_scene():
    rng = np.random.default_rng(33)
    f, truth = pn.random_solver(rng, 60, min_inliers=10, max_iterations=12, tail=5, seed=33, outlier_frac=0.3)
    problems = pn.pack([f])
    want = pn.table(problems)
    t = lib.pnp_table(want, 0)
    # conditions on the inputs, checked on the numpy table alone
    assert t["returns"].any()
    h = int(np.argmax(t["returns"]))
    assert np.array_equal(pn.unpack_mask(t["refined_mask"][t["best"][h]], 60), truth["inliers"])
    assert not pn.tables_equal(lib.pnp_ransac_host(problems), want)
    R = t["refined_R"][t["best"][h]].reshape(3, 3)
    assert np.allclose(R, truth["R"], atol=1e-4) and np.allclose(t["refined_t"][t["best"][h]], truth["t"], atol=1e-3)


def test_degenerate_scenes():
    scenes = pn.degenerate_solvers(np.random.default_rng(23))
    names = list(scenes)
    traces = []
    got, _ = _assert_same(pn.pack([scenes[k] for k in names]), traces)
    by = {k: [tr for s, _, tr in traces if names[s] == k] for k in names}
    # coplanar world points: PW0tPW0 has an exactly zero singular value (cv::RNG supplies the third left vector), the control
    # points' matrix a zero column, so cvInvert is a pseudo-inverse: a singular value under SVBkSb's threshold is dropped
    assert by["coplanar"] and all(tr.invert_dropped >= 1 for tr in by["coplanar"])
    for tr in by["coplanar"]:
        G = np.array(tr.svd_inputs[0])
        assert np.all(G[2] == 0) and np.all(G[:, 2] == 0)
    # four coincident points: rho == 0, L's first column is matched by a zero system, qr_solve returns early
    assert by["coincident"] and all(tr.qr_early >= 1 for tr in by["coincident"])
    assert all(tr.qr_early == 0 for tr in by["generic"])
    # NaN world points: a hypothesis that samples one is NaN, counts nothing and is never the best row
    s = names.index("nan")
    t = lib.pnp_table(got, s)
    nan_rows = np.isnan(t["R"]).any(1)
    assert nan_rows.any() and np.all(t["inliers"][nan_rows] == 0)
    assert not any(b >= 0 and nan_rows[b] for b in t["best"])
    assert np.all(t["R"].view(np.uint64)[np.isnan(t["R"])] == 0x7FF8000000000000)


def test_zero_depth_is_an_infinite_projection_and_no_inlier():
    """CheckInliers at Zc == 0: invZc is +inf, the projection infinite or NaN, and `error2 < max` fails"""
    R, t, K, p2d, Xw, me, kind = pn.zc_zero_case()
    depth = [R[6] * float(X[0]) + R[7] * float(X[1]) + R[8] * float(X[2]) + t[2] for X in Xw]
    assert all((d == 0.0) == (k != 0) for d, k in zip(depth, kind)) and set(kind) == {0, 1, 2}
    want = pn.check_inliers(R, t, K, p2d, Xw, me)
    assert np.array_equal(want, kind == 0)
    assert np.array_equal(lib.pnp_inliers(R, t, K, p2d, Xw, me), want)
    # and the host's test is the restatement's on a planted scene under a perturbed pose, where both answers occur
    f, truth = pn.random_solver(np.random.default_rng(41), 200, outlier_frac=0.3, noise=1.0)
    Rp = (truth["R"] @ pn.rot([0, 1, 0], 2e-4)).reshape(9).tolist()
    tp = truth["t"].tolist()
    me = (f["sigma2"] * np.float32(5.991)).astype(np.float32)
    want = pn.check_inliers(Rp, tp, K, f["p2d"], f["Xw"], me)
    assert 20 < want.sum() < 180 and np.array_equal(lib.pnp_inliers(Rp, tp, K, f["p2d"], f["Xw"], me), want)


CONDITION_SEEDS = (3, 5, 13)


def test_conditions_across_the_suite():
    """three refine jobs in one solver; a refine that does not return; a returning row whose best is an earlier row"""
    problems = pn.pack([pn.searched_solver(s) for s in CONDITION_SEEDS])
    got, _ = _assert_same(problems)
    tabs = [lib.pnp_table(got, s) for s in range(len(CONDITION_SEEDS))]
    rows = [(t, r) for t in tabs for r in range(len(t["inliers"]))]
    assert any(t["refines"] >= 3 for t in tabs)
    assert any(t["inliers"][r] >= t["min_inliers"] and t["refined_inliers"][t["best"][r]] <= t["min_inliers"] and not t["returns"][r]
               for t, r in rows)
    assert any(t["returns"][r] and t["best"][r] != r for t, r in rows)


def _schedule(w, calls):
    """calls: 'find' or an iteration count, then iterate(5) again and again; the results until bNoMore"""
    out = []
    for c in list(calls) + [5] * 40:
        res = w.find() if c == "find" else w.iterate(c)
        out.append(res)
        if res[2]:
            break
    return out


@pytest.mark.parametrize("seed", CONDITION_SEEDS)
@pytest.mark.parametrize("calls", ([5] * 8, ["find", 5, 5], [1, 2, 3, 4, 5, 5], [5, "find", 5]), ids=("i5", "find", "mixed", "i5find"))
def test_walker_equals_the_literal_loop(seed, calls):
    """every returned pose is rejected by the caller, who calls again; the schedules read rows past `iterations`"""
    f = dict(pn.searched_solver(seed), tail=100)
    problems = pn.pack([f])
    t = lib.pnp_table(lib.pnp_ransac_host(problems), 0)
    N = len(f["p2d"])
    got = _schedule(pn.TableWalker(t, N), calls)
    want = _schedule(pn.LiteralSolver(pn.solver_of(problems, 0)), calls)
    assert got == want and got[-1][2]


def test_walker_reads_past_iterations_and_runs_off_the_tail():
    f = pn.searched_solver(3)                          # no row of it returns
    N = len(f["p2d"])
    t = lib.pnp_table(lib.pnp_ransac_host(pn.pack([dict(f, tail=5)])), 0)
    assert not t["returns"].any() and t["iterations"] == 10 and len(t["inliers"]) == 15
    # the `||`: a call that starts below mRansacMaxIts runs to it whatever nIterations is
    w = pn.TableWalker(t, N)
    assert w.iterate(1) == ("best", 6, True) and w.done == 10
    # and one that starts at it runs nIterations more rows, past `iterations`
    assert w.iterate(5) == ("best", 6, True) and w.done == 15
    with pytest.raises(pn.OffTheTail):
        w.iterate(5)
    # the refill with a larger tail continues where the first table ended: the seed fixes every row
    t2 = lib.pnp_table(lib.pnp_ransac_host(pn.pack([dict(f, tail=10)])), 0)
    for k in ("sample", "R", "inliers", "best", "returns"):
        assert np.array_equal(t2[k][:15], t[k], equal_nan=True)
    w2 = pn.TableWalker(t2, N)
    w2.done = 15
    lit = pn.LiteralSolver(pn.solver_of(pn.pack([f]), 0))
    assert [lit.iterate(1), lit.iterate(5), lit.iterate(5)][2] == w2.iterate(5)
    # too few correspondences: no rows, bNoMore at once
    f0 = pn.random_solver(np.random.default_rng(1), 7, min_inliers=10, tail=5)[0]
    t0 = lib.pnp_table(lib.pnp_ransac_host(pn.pack([f0])), 0)
    assert len(t0["inliers"]) == 0 and pn.TableWalker(t0, 7).iterate(5) == (None, -1, True)
    assert pn.LiteralSolver(pn.solver_of(pn.pack([f0]), 0)).iterate(5) == (None, -1, True)


def _refused(problems):
    with pytest.raises(lib.DrfeError):
        lib.pnp_ransac_host(problems)


def test_refusals():
    rng = np.random.default_rng(17)
    ok = pn.random_solver(rng, 20, max_iterations=3, tail=1)[0]
    lib.pnp_ransac_host(pn.pack([ok]))
    _refused(pn.pack([pn.random_solver(rng, pn.MAX_CORR + 1, max_iterations=1, tail=0)[0]]))
    _refused(pn.pack([dict(ok, max_iterations=pn.MAX_ITERATIONS + 1)]))
    _refused(pn.pack([dict(ok, tail=pn.MAX_TAIL + 1)]))
    _refused(pn.pack([dict(ok, tail=-1)]))
    _refused(pn.pack([ok, dict(ok, min_inliers=-1)]))
    for bad in (np.inf, np.nan):
        sig = ok["sigma2"].copy()
        sig[7] = bad
        _refused(pn.pack([dict(ok, sigma2=sig)]))
    _refused(pn.pack([dict(ok, th2=3e38)]))             # sigma2 * th2 overflows float
    p = pn.pack([ok, ok])
    p["offsets"] = np.array([0, 30, 20], np.int32)
    p["p2d"], p["Xw"], p["sigma2"] = p["p2d"][:30], p["Xw"][:30], p["sigma2"][:30]
    _refused(p)
    # 65 536 solvers in one call
    n = 65536
    big = dict(K=np.tile(pn.K_DEFAULT, (n, 1)), probability=np.full(n, 0.99), min_inliers=np.full(n, 10, np.int32),
               max_iterations=np.ones(n, np.int32), epsilon=np.full(n, 0.5, np.float32), th2=np.full(n, 5.991, np.float32),
               tail=np.zeros(n, np.int32), seed=np.zeros(n, np.uint32), offsets=np.zeros(n + 1, np.int32),
               p2d=np.zeros((0, 2), np.float32), Xw=np.zeros((0, 3), np.float32), sigma2=np.zeros(0, np.float32))
    _refused(big)
    for k in big:
        big[k] = big[k][:-1] if k not in ("p2d", "Xw", "sigma2") else big[k]
    assert lib.pnp_ransac_host(big)["hypotheses"].sum() == 0
    # the totals of a call: 1 800 empty solvers of 600 rows are more than 2^20 rows; 300 solvers of 4 096 correspondences and 600
    # rows are 11.5 M mask words, still below 2^24, 500 of them are above
    n = 1800
    rows = {k: v[:n] for k, v in big.items() if k not in ("p2d", "Xw", "sigma2", "offsets")}
    rows.update(max_iterations=np.full(n, 300, np.int32), tail=np.full(n, 300, np.int32), offsets=np.zeros(n + 1, np.int32),
                p2d=big["p2d"], Xw=big["Xw"], sigma2=big["sigma2"])
    _refused(rows)
    n, N = 500, pn.MAX_CORR
    words = {k: v[:n] for k, v in rows.items() if k not in ("p2d", "Xw", "sigma2", "offsets")}
    words.update(min_inliers=np.full(n, 5000, np.int32), offsets=(np.arange(n + 1) * N).astype(np.int32),
                 p2d=np.zeros((n * N, 2), np.float32), Xw=np.zeros((n * N, 3), np.float32), sigma2=np.ones(n * N, np.float32))
    assert n * 600 <= 2 ** 20 < 1800 * 600 and n * 600 * 64 > 2 ** 24
    _refused(words)


def _suite_matrices():
    traces = []
    solvers = [pn.searched_solver(s) for s in CONDITION_SEEDS] + [pn.degenerate_solvers(np.random.default_rng(23))["generic"]]
    pn.table(pn.pack(solvers), traces)
    mats = [np.array(A) for _, _, tr in traces for A in tr.svd_inputs]
    return [A for A in mats if np.isfinite(A).all() and np.abs(A).max() > 0]


def test_double_jacobi_svd_is_an_svd():
    """the 12x12, 3x3 and 6xk matrices of the suite: singular values against numpy.linalg.svd, relative to the largest one.  The
    bit-level claim is host against numpy (the tables above); this catches a wrong rotation or sort."""
    mats = _suite_matrices()
    shapes = set(A.shape for A in mats)
    assert {(12, 12), (3, 3), (6, 4), (6, 3), (6, 5)} <= shapes
    worst_np = worst_host = 0.0
    for A in mats:
        ref = np.linalg.svd(A, compute_uv=False)
        w_np = np.array(pn.jacobi_svd(A.tolist())[0])
        w, ut, vt = lib.pnp_svd(A)
        assert np.array_equal(w, w_np)                 # the host's is the restatement's, bit for bit
        worst_np = max(worst_np, float(np.abs(w_np - ref).max() / ref[0]))
        worst_host = max(worst_host, float(np.abs(w - ref).max() / ref[0]))
        assert np.all(np.diff(w) <= 0)
        # U^T diag(w) Vt rebuilds A where the singular value is not negligible
        rebuilt = (ut.T * w) @ vt
        assert np.abs(rebuilt - A).max() <= 1e-12 * max(ref[0], 1.0)
    print(f"jacobi_svd vs numpy.linalg.svd over {len(mats)} matrices: numpy restatement {worst_np:.3e}, host {worst_host:.3e}")
    assert worst_host <= SVD_BOUND


@pytest.mark.parametrize("verdicts", ((0, 0, 1), (0,) * 40), ids=("third", "none"))
def test_native_candidate_loop_on_the_host_entry(tmp_path, verdicts):
    """tests/native/pnp_caller.cpp in its host mode (every solver fills its own table on first use, and refills it with a larger
    tail when a walk runs off it) against the walk over the ctypes host tables"""
    import os
    import subprocess
    import native_build
    exe = native_build.caller("pnp_caller")          # built here if the tests directory holds no build products
    blob, problems, indices, n_keys = pn.caller_scene(np.random.default_rng(61), verdicts)
    (tmp_path / "in.bin").write_bytes(blob)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "host"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "pnp_caller ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    problems["tail"][:] = pn.MAX_TAIL
    r = lib.pnp_ransac_host(problems)
    want, handed, past = pn.caller_expected([lib.pnp_table(r, s) for s in range(3)], indices, n_keys, verdicts)
    assert handed >= 3 and (tmp_path / "out.bin").read_bytes() == want
    if not any(verdicts):
        assert past and " 0 refills" not in p.stdout    # rejected poses send the cursor past mRansacMaxIts and off a tail of 5
