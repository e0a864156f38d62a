"""CPU tests of the Levenberg optimisers' host entries on the hand-built degenerate systems of tests/lm_edge_scenarios.py (DESIGN.md
section 24): every scene takes the control path it is named for, counted on the restatement by paths(); the host entry equals the
restatement on every scene, byte for byte; the thresholds are where the scenes say they are; the LDLT keeps the sign of a zero
right-hand side.  These are the tests the mutants of lm_core.h listed in section 24 were run against."""
import math

import numpy as np
import pytest

import lm_edge_scenarios as L
from dr_slam_amd import lib

HOST = {"pose_opt": lib.pose_opt_host, "trans_opt": lib.trans_opt_host, "sim3_opt": lib.sim3_opt_host}
ALL = [(o, n) for o in L.OPTIMISERS for n in L.scenes(o)]
IDS = [f"{o}-{n}" for o, n in ALL]


@pytest.mark.parametrize("optimiser,name", ALL, ids=IDS)
def test_scene_takes_its_path(optimiser, name):
    sc = L.scenes(optimiser)[name]
    r = L.scene_paths(optimiser, name)
    assert L.unmet(r, sc["expect"]) == [], {k: r[k] for k in ("stops", "trials_per_iteration", "failed_solves", "accepted_after_failed",
                                                               "good_after_failed", "stale_x_across_calls", "uncertifiable",
                                                               "first_tr", "first_pivot_ratio", "max_theta")}
    o = r["out"]
    n_edges = 2 * len(sc["scene"]["index"]) if optimiser == "sim3_opt" else (
        o["point_outlier"].size + 2 * o["line_outlier"].size + int(np.sum(sc["scene"]["plane_mask"] != 0)))
    assert n_edges <= 300


@pytest.mark.parametrize("optimiser,name", ALL, ids=IDS)
def test_host_equals_the_restatement(optimiser, name):
    m = L.MODULE[optimiser]
    h = HOST[optimiser](m.pack([L.scenes(optimiser)[name]["scene"]]))
    assert m.tables_equal(h, L.expected_table(optimiser, [name])) == []


@pytest.mark.parametrize("optimiser", L.OPTIMISERS)
def test_host_equals_the_restatement_in_one_call(optimiser):
    """every scene of an optimiser in one host call, a plain scene between every two: each keeps the rows it has alone"""
    m = L.MODULE[optimiser]
    names = list(L.scenes(optimiser))
    items = L.interleaved(optimiser, names)
    h = HOST[optimiser](m.pack([s for _, s in items]))
    assert m.tables_equal(h, L.expected_table_of(optimiser, items)) == []


def test_every_listed_path_has_a_scene():
    """what the scenes reach, per optimiser, and the paths no scene reaches (DESIGN.md section 24 lists the same)"""
    for o in L.OPTIMISERS:
        rs = [L.scene_paths(o, n) for n in L.scenes(o)]
        assert sum(r["failed_solves"] for r in rs) > 100
        assert any(r["accepted_after_failed"] for r in rs) and any(r["good_after_failed"] for r in rs)
        assert any(r["rho0_first_then_more"] for r in rs) and any(r["qmax_stops"] for r in rs)
        assert any(r["stale_x_across_calls"] for r in rs)
        assert any(u[:2] == ("cube", "range") and u[3] == "levenberg" for r in rs for u in r["uncertifiable"])
        assert {len(t) for r in rs for t in r["trials_per_iteration"]} >= {0, 1, 10} or o == "sim3_opt"
        # not reached by any scene: an x left over an empty round, and a tie of the cube
        assert not any(r["stale_x_after_empty"] for r in rs)
        assert not any(u[1] == "tie" for r in rs for u in r["uncertifiable"])
    assert any(u[0] == "sincos" for n in L.scenes("pose_opt") for u in L.scene_paths("pose_opt", n)["uncertifiable"])
    assert L.scene_paths("trans_opt", "negative_mono")["max_theta"] == 0.0      # translation only: omega is zero, always
    assert any(L.scene_paths("sim3_opt", n)["sigma_nonzero"] for n in L.scenes("sim3_opt"))


def test_thresholds_are_where_the_scenes_put_them():
    """the chi2 of the threshold scenes recomputed from their fields alone"""
    F, D = np.float32, np.float64
    for o in ("pose_opt", "trans_opt"):
        fr = L.scenes(o)["chi2_at_thresholds"]["scene"]
        e0 = fr["obs"][:, 0].astype(D) - D(F(L.EXACT_K[2]))
        chi2 = (e0 * (fr["inv_sigma2"].astype(D) * e0)).astype(F)
        th = np.where(fr["u_right"] < 0, L.TH_MONO, L.TH_STEREO)
        assert (np.abs(e0) == 2).all() and (fr["obs"][:, 1] == F(L.EXACT_K[3])).all()
        want = np.concatenate([np.repeat(L._near(t), 2) for t in (L.TH_MONO, L.TH_STEREO)])
        assert chi2.tobytes() == want.astype(F).tobytes()
        assert [int(v) for v in chi2 > th] == L.scenes(o)["chi2_at_thresholds"]["expect"]["flags"]["point_outlier"]
        e = fr["line_fn"][:, 2]                                      # 3 cx - 4 cy is zero: the error is the offset
        assert ((e * e).astype(F).tobytes() == np.repeat(L._near(L.TH_LINE), 2).astype(F).tobytes())
        hub = L.scenes(o)["huber_at_delta"]["scene"]
        assert [float(v) for v in hub["inv_sigma2"][:6:2]] == [float(v) for v in L._near(L._delta_sq(5.991))]
        assert [float(v) for v in hub["inv_sigma2"][1:6:2]] == [float(v) for v in L._near(L._delta_sq(7.815))]
    pr = L.scenes("sim3_opt")["chi2_at_th2"]["scene"]
    for key, wkey, rows in (("obs1", "inv_sigma2_1", slice(0, 6)), ("obs2", "inv_sigma2_2", slice(6, 12))):
        e0 = pr[key][rows, 0].astype(D) - D(F(L.sn.CAM1[2]))
        chi2 = e0 * (pr[wkey][rows].astype(D) * e0)
        assert [c > 10.0 for c in chi2] == [False, False, False, False, True, True] and chi2[2] == 10.0 == chi2[3]
        assert chi2[0] == 4 * D(np.nextafter(F(2.5), F(0))) and chi2[4] == 4 * D(np.nextafter(F(2.5), F(3)))
    lo, hi = (L.scene_paths("pose_opt", n)["thetas"][0] for n in ("theta_below_1e-5", "theta_at_1e-5"))
    assert lo < 1e-5 <= hi and hi - lo < 64 * math.ulp(1e-5)
    lo, hi = (L.scene_paths("sim3_opt", n)["thetas"][0] for n in ("theta_below_1e-5", "theta_at_1e-5"))
    assert lo < 1e-5 <= hi and hi - lo < 2e-13


def test_certificate_ranges_agree_with_the_library():
    """paths() counts hand-backs from the documented ranges; the library's own certificate says the same at their ends"""
    x = np.array([2.0 ** 300, np.nextafter(2.0 ** 300, 0), 2.0 ** -300, np.nextafter(2.0 ** -300, 1), 7.0e298, 208065.0, 208067.0,
                  3.0, -1.5e90, 0.0])
    _, ok = lib.cr_cube(x)
    assert [L.cube_uncertifiable(v) is None for v in x] == [bool(v) for v in ok]
    assert L.cube_uncertifiable(208065.0) == "tie" and L.cube_uncertifiable(7.0e298) == "range"
    assert L.sincos_uncertifiable(64.0) == "range" and L.sincos_uncertifiable(np.nextafter(64.0, 0)) is None


@pytest.mark.parametrize("n", (6, 7))
def test_ldlt_keeps_the_sign_of_a_zero_right_hand_side(n):
    """triangular_solve_vector skips a zero element of the right-hand side: a -0 further down is not turned into +0 by
    subtracting 0 * L.  No optimisation produces a -0 in b, so the hook is the only way to it."""
    solve = (lib.pose_opt_ldlt, L.pn.ldlt_solve) if n == 6 else (lib.sim3_opt_ldlt, L.sn.ldlt_solve7)
    A = np.diag(np.arange(n, 0, -1).astype(np.float64)) * 4
    for i in range(n):
        for j in range(i):
            A[i, j] = A[j, i] = -0.25 * (1 + (i + j) % 3)
    for zero in range(n - 1):
        b = np.zeros(n)
        b[zero + 1:] = -0.0                                          # +0 up to `zero`, -0 below it
        ok, x = solve[0](A, b)
        ok2, x2 = solve[1]([[float(v) for v in row] for row in A], [float(v) for v in b])
        assert ok and ok2 and np.asarray(x, np.float64).tobytes() == np.asarray(x2, np.float64).tobytes(), (zero, x, x2)
        assert [bool(v) for v in np.signbit(x)] == [False] * (zero + 1) + [True] * (n - zero - 1) and not np.any(x)
