"""CPU (-m "not gpu") tests of OptimizeSim3's host entry (drfe_sim3_opt_host): every output byte for byte
against the numpy restatement (tests/sim3_opt_numpy.py) on behaviour scenes, match counts and random problems; that the behaviour
scenes take the paths they are named after (through the entry's diagnostics); the stale-error classification and the x[6] side
effect, each shown to decide something; the refusals and caps; the 7x7 LDLT and the four branches of the step on their own; the
planted Sim3; Scw; the native caller; the exported symbols and the struct layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sim3_opt_numpy as sn
from dr_slam_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64


def _host(problems):
    return lib.sim3_opt_host(sn.pack(problems))


def _diag(h, i):
    return dict(zip(lib.SIM3_OPT_DIAG, h["diag"][i][:7].tolist()))


def test_new_symbols_are_exported_as_declared():
    L = lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drfe.h")).read(), flags=re.S)
    header = " ".join(header.split())
    for decl in ("int drfe_sim3_opt_host(const drfe_sim3_opt_problems* problems, drfe_sim3_opt_out* out);",
                 "int drfe_sim3_opt_batch(drfe_ctx* ctx, const drfe_sim3_opt_problems* problems, drfe_sim3_opt_out* out, void* stream);",
                 "int drfe_sim3_opt_stats(drfe_ctx* ctx, int64_t* stats );"):
        assert decl in header, decl
    for name, nargs in (("drfe_sim3_opt_host", 2), ("drfe_sim3_opt_batch", 4), ("drfe_sim3_opt_stats", 2),
                        ("drfe_debug_sim3_opt_hand_back", 2), ("drfe_debug_sim3_opt_ldlt", 4), ("drfe_debug_sim3_opt_step", 6)):
        assert name in lib.SYMBOLS and len(getattr(L, name).argtypes) == nargs
    # the structs as the header lays them out on LP64: 2 int32 and 17 pointers; 9 pointers
    assert C.sizeof(lib.Sim3OptProblems) == 8 + 17 * 8 and C.sizeof(lib.Sim3OptOut) == 9 * 8
    for struct, cls in (("drfe_sim3_opt_problems", lib.Sim3OptProblems), ("drfe_sim3_opt_out", lib.Sim3OptOut)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header)
        fields = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", m.group(1))
        assert fields == [f[0] for f in cls._fields_], fields
    for name, value in (("DRFE_SIM3_OPT_MAX_PROBLEMS", lib.SIM3_OPT_MAX_PROBLEMS), ("DRFE_SIM3_OPT_MAX_MATCHES", lib.SIM3_OPT_MAX_MATCHES),
                        ("DRFE_SIM3OPT_DEVICE_FROM", lib.SIM3OPT_DEVICE_FROM)):
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
    # what needs no device: the refusal of a call without a context
    P, out, _, _keep = lib._sim3_opt_pack(sn.pack([sn.problem(np.random.default_rng(0), 12)]))
    assert L.drfe_sim3_opt_batch(None, C.byref(P), C.byref(out), None) == -1
    assert L.drfe_sim3_opt_stats(None, None) == -1


def test_ldlt_7x7_matches_the_restatement_and_solves():
    rng = np.random.default_rng(4)
    for trial in range(40):
        A = rng.normal(size=(9, 7))
        H = A.T @ A * 10.0 ** rng.integers(-3, 6)
        if trial % 4 == 1:
            H[:, 6] = 0
            H[6, :] = 0                              # the fixed scale's row and column: positive semi-definite
        if trial % 4 == 2:
            H[3, 3] = -H[3, 3]                       # indefinite
        b = rng.normal(size=7)
        pos, x = lib.sim3_opt_ldlt(H, b)
        want_pos, want_x = sn.ldlt_solve7(H.tolist(), b.tolist())
        assert pos == want_pos == (trial % 4 != 2)
        if pos:
            assert np.array_equal(x.view(U64), np.array(want_x).view(U64))
            if trial % 4 in (0, 3):
                assert np.allclose(H @ x, b, rtol=1e-6, atol=1e-6 * np.abs(b).max())
    pos, x = lib.sim3_opt_ldlt(np.zeros((7, 7)), rng.normal(size=7))     # isPositive() of a zero matrix, x = 0
    assert pos and not x.any()
    want_pos, want_x = sn.ldlt_solve7(np.zeros((7, 7)).tolist(), [1.0] * 7)
    assert want_pos and not any(want_x)


def test_step_takes_the_four_branches_of_the_exponential():
    """Sim3(x) * estimate with theta and |sigma| on either side of 1e-5, against the restatement; the scale moves only when free"""
    rng = np.random.default_rng(6)
    S = sn.problem(rng, 12)["S12"]
    S[7] = 1.1
    for theta in (3e-6, 0.02):
        for sigma in (4e-6, -0.03):
            w = rng.normal(size=3)
            x = np.concatenate([w / np.linalg.norm(w) * theta, rng.normal(size=3) * 0.1, [sigma]])
            for fix in (0, 1):
                got, _ = lib.sim3_opt_step(S, x, np.zeros(7), 0.0, fix)
                (q, t, s), small = sn.oplus(sn.s12_tuple(S), list(x), fix)
                assert small == (theta < 1e-5)
                assert np.array_equal(got.view(U64), np.array(q + t + [s]).view(U64)), (theta, sigma, fix)
                assert (got[7] == S[7]) == bool(fix)


def test_fixed_scale_zeroes_x6_before_compute_scale_reads_it():
    """oplusImpl writes update[6] = 0 through the solver's own x, so Levenberg's computeScale, which runs after update(), reads a
    zero there.  In a call's own flow x[6] is a zero already (column 6 of every Jacobian is +0.0, so H's row 6 and b[6] are); the
    step hook shows the order of the two reads on an x[6] that is not."""
    rng = np.random.default_rng(7)
    S = sn.problem(rng, 12)["S12"]
    x, b, lam = rng.normal(size=7) * 0.01, rng.normal(size=7), 0.37
    _, after = lib.sim3_opt_step(S, x, b, lam, 1)
    _, before = lib.sim3_opt_step(S, x, b, lam, 1, read_before=True)
    xs = list(x)
    sn.oplus(sn.s12_tuple(S), xs, True)
    assert xs[6] == 0.0 and after == sn.compute_scale(xs, b, lam)
    assert before == sn.compute_scale(list(x), b, lam)
    assert before != after                           # the order of the reads decides the scale
    _, free = lib.sim3_opt_step(S, x, b, lam, 0)
    assert free == before                            # a free scale leaves x[6] alone


def test_behaviour_scenes_take_their_paths_and_equal_the_restatement():
    B = sn.behaviour_problems()
    names = list(B)
    probs = [B[k] for k in names]
    h = _host(probs)
    off = sn.pack(probs)["match_offsets"]
    d = {k: _diag(h, i) for i, k in enumerate(names)}
    it = {k: h["iterations"][i].tolist() for i, k in enumerate(names)}
    nbad = {k: int(h["n_bad"][i]) for i, k in enumerate(names)}
    # no outlier: the second optimize() stops at 5 iterations; planted outliers: it goes on to 10
    assert nbad["five_more"] == 0 and it["five_more"] == [5, 5] and d["five_more"]["nbad_stops"] == 0
    assert nbad["ten_more"] > 0 and it["ten_more"] == [5, 10]
    assert nbad["clean"] == 0 and it["clean"][1] <= 5 and nbad["outliers"] == 16
    # fewer than 10 pairs left: 0, the estimate's bits untouched, the nulled matches reported
    i = names.index("too_few")
    assert h["returns"][i] == 0 and d["too_few"]["early_return"] == 1 and it["too_few"][1] == 0
    assert np.array_equal(h["S12"][i].view(U64), B["too_few"]["S12"].view(U64))
    assert h["outlier"][off[i]:off[i + 1]].sum() == nbad["too_few"] > 14 - 10
    assert sum(v["early_return"] for v in d.values()) == 1
    assert d["clean"]["rejected"] > 0 and d["clean"]["last_rejected"] >= 1
    assert d["nbad_stop"]["nbad_stops"] == 2                     # both optimize() calls stopped by _nBad >= 3
    for k in ("clean", "far_start", "free_big"):
        assert d[k]["small_theta"] > 0 and d[k]["big_theta"] > 0
    # z == 0 after the map: the errors are not finite from the first pass on, every trial is rejected, the estimate stays, and
    # the errors the last (rejected) trial left are NaN, which is no outlier: the planted outliers pass, whom a recompute rejects
    for k in ("z0_e12", "z0_e21"):
        i = names.index(k)
        assert d[k]["rejected"] == h["trials"][i].sum() > 0 and d[k]["last_rejected"] == 2
        assert np.array_equal(h["S12"][i].view(U64), B[k]["S12"].view(U64))
        assert not h["outlier"][off[i]:off[i + 1]].any() and h["returns"][i] == 40
        assert d[k]["stale_decided"] >= 3
    for k in ("zneg_e12", "zneg_e21"):
        i = names.index(k)
        assert np.isfinite(h["S12"][i]).all() and h["outlier"][off[i] + 3]
    assert sn.tables_equal(h, sn.numpy_table("behaviour", probs)) == []


def test_stale_errors_decide_classifications_that_a_recompute_decides_otherwise():
    """After a call whose last trial was rejected the reference classifies on the errors at the rejected estimate.  Recomputing
    them at the kept estimate, as PoseOptimization's computeError() would, gives another verdict for the matches the diagnostic
    counts; the restatement run with a recompute returns other flags than the entry."""
    pr = sn.behaviour_problems()["z0_e12"]
    h = _host([pr])
    assert _diag(h, 0)["last_rejected"] == 2 and _diag(h, 0)["stale_decided"] > 0

    class Recompute(sn.Optimizer):
        def classify(self, S):
            act, stale, fresh = super().classify(S)
            return act, fresh, fresh
    r = Recompute(pr).run()
    assert r["outlier"].sum() > 0 and not h["outlier"].any()
    assert r["n_bad"] != h["n_bad"][0]


def test_free_scale_steps_see_sigma_on_both_sides_of_the_threshold(monkeypatch):
    sigmas = []
    real = sn.sim3_exp

    def spy(u):
        sigmas.append(abs(u[6]))
        return real(u)
    monkeypatch.setattr(sn, "sim3_exp", spy)
    B = sn.behaviour_problems()
    r = sn.table([B["free_big"], B["free_small"]])
    steps = [s for s in sigmas if s != 1e-9 and s != 0.0]        # the numeric Jacobian's own perturbations aside
    assert any(s >= 1e-5 for s in steps) and any(0 < s < 1e-5 for s in steps)
    h = _host([B["free_big"], B["free_small"]])
    assert sn.tables_equal(h, r) == []
    assert abs(h["S12"][0][7] - 1.3) < 0.02 and abs(h["S12"][1][7] - 1.0) < 0.02


def test_match_counts_equal_the_restatement():
    probs = sn.size_problems()
    h = _host(probs)
    assert sn.tables_equal(h, sn.numpy_table("size", probs)) == []
    r = dict(zip(sn.SIZES, zip(h["returns"].tolist(), h["diag"][:, 5].tolist(), h["iterations"][:, 0].tolist())))
    assert r[0] == (0, 1, 0)                         # no match: no iteration, the return before the second optimize()
    assert r[9][:2] == (0, 1) and r[9][2] > 0        # nine pairs are optimised once and then found too few
    assert r[10][1] == 0 and r[10][0] == 10
    for n in sn.SIZES[3:]:
        assert r[n][1] == 0 and 0.7 * n <= r[n][0] <= n


def test_unequal_intrinsics_are_kept_apart():
    pr = sn.behaviour_problems()["unequal_k"]
    a = _host([pr])
    b = _host([dict(pr, K2=pr["K1"])])
    assert a["returns"][0] >= 40 and b["returns"][0] < a["returns"][0]


def test_random_problems_equal_the_restatement_and_recover_the_planted_sim3():
    """20 problems, a quarter with a free scale; 15 % of the matches moved by 15 .. 60 px, pixel noise 0.7 px times the level's
    sigma.  The tolerances are the noise's: with 40 or more matches at 1.5 .. 6 m and f = 517 px, 0.7 px is 0.7 / 517 rad = 1.4e-3
    rad a match and 1.4e-3 x 6 m = 8 mm a match at most; 0.01 rad, 0.05 m and 2 % of scale allow for the octave's sigma (up to 3.6)
    and the few matches of the smallest problem."""
    probs = sn.random_problems()
    assert max(len(p["index"]) for p in probs) <= 150
    h = _host(probs)
    assert sn.tables_equal(h, sn.numpy_table("random", probs)) == []
    for i, pr in enumerate(probs):
        R12, t12, s12 = pr["planted"]
        q, t, s = sn.s12_tuple(h["S12"][i])
        R = np.array(sn.pon.quat_matrix(q))
        ang = np.arccos(np.clip((np.trace(R.T @ R12) - 1) / 2, -1, 1))
        assert ang < 0.01 and np.abs(np.array(t) - t12).max() < 0.05 and abs(s - s12) < 0.02 * s12, (i, ang, t, t12, s, s12)
        assert h["returns"][i] >= 0.7 * len(pr["index"])


def test_scw_is_the_restated_product():
    probs = sn.random_problems()[:6]
    h = _host(probs)
    for i, pr in enumerate(probs):
        S = sn.s12_tuple(h["S12"][i])
        assert np.array_equal(h["Scw"][i].view(np.uint32), sn.scw(pr, S).view(np.uint32))
        assert np.array_equal(h["T12"][i].view(np.uint32), sn.to_cvmat(S).view(np.uint32))
        # and what it is for: a world point through key frame 2's pose and then S12
        Smw = np.eye(4)
        Smw[:3, :3], Smw[:3, 3] = pr["R2w"].reshape(3, 3), pr["t2w"]
        assert np.allclose(h["Scw"][i].reshape(4, 4), h["T12"][i].reshape(4, 4).astype(np.float64) @ Smw, atol=1e-5)


@pytest.mark.parametrize("n", (0, 1, 2, 63, 64, 65, 300))
def test_problems_per_call(n):
    probs = sn.mix_problems(n, seed=n, n=12)
    h = _host(probs)
    assert h["S12"].shape == (n, 8) and len(h["outlier"]) == sum(len(p["index"]) for p in probs)
    if n:
        # a problem's outputs do not depend on its neighbours in the call
        one = _host(probs[-1:])
        assert np.array_equal(one["S12"][0].view(U64), h["S12"][-1].view(U64)) and one["returns"][0] == h["returns"][-1]
        assert (h["iterations"][:, 0] > 0).all()


def test_caps_run_and_one_above_is_refused():
    rng = np.random.default_rng(9)
    big = sn.problem(rng, lib.SIM3_OPT_MAX_MATCHES, outlier_frac=0.1)
    h = _host([big])
    assert h["returns"][0] > 0.8 * lib.SIM3_OPT_MAX_MATCHES and np.isfinite(h["S12"]).all()
    with pytest.raises(lib.DrfeError):
        _host([sn.problem(rng, lib.SIM3_OPT_MAX_MATCHES + 1)])
    small = sn.problem(rng, 3)
    with pytest.raises(lib.DrfeError):
        _host([small] * (lib.SIM3_OPT_MAX_PROBLEMS + 1))
    assert len(_host([small] * lib.SIM3_OPT_MAX_PROBLEMS)["returns"]) == lib.SIM3_OPT_MAX_PROBLEMS
    bad = sn.pack([sn.problem(rng, 5), sn.problem(rng, 5)])
    bad["match_offsets"] = np.array([0, 7, 5], np.int32)
    with pytest.raises(lib.DrfeError):
        lib.sim3_opt_host(bad)
    bad = sn.pack([sn.problem(rng, 5)])
    bad["index"] = bad["index"][::-1].copy()
    with pytest.raises(lib.DrfeError):
        lib.sim3_opt_host(bad)


def test_cap_refusals_name_the_enum():
    """the message of a refused call names the cap: read from the source, since the host entry has no context to keep it in"""
    src = open(os.path.join(ROOT, "dr_slam_amd", "csrc", "sim3_opt.cpp")).read()
    assert "more than DRFE_SIM3_OPT_MAX_PROBLEMS problems" in src and "more than DRFE_SIM3_OPT_MAX_MATCHES matches" in src


@pytest.mark.parametrize("mode", ("host", "auto"))
def test_native_caller_on_the_host_entry(tmp_path, mode):
    """tests/native/sim3_opt_caller.cpp: Planar_SLAM::Optimizer::OptimizeSim3 candidate by candidate until one is accepted, then
    drfe::Sim3OptBatch over all of them, forced to the host entry or left at DRFE_SIM3OPT_DEVICE_FROM (these four go to the host
    entry), against the ctypes path"""
    import subprocess
    import native_build
    exe = native_build.caller("sim3_opt_caller")          # built here if the tests directory holds no build products
    blob, probs = sn.caller_scene()
    (tmp_path / "in.bin").write_bytes(blob)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "sim3_opt_caller ok" in p.stdout and "match 2 / 2" in p.stdout, (p.returncode, p.stdout, p.stderr)
    assert "batch device calls 0," in p.stdout
    h = _host(probs)
    assert h["returns"][0] < 20 and h["returns"][1] == 0 and h["returns"][2] >= 20
    assert (tmp_path / "out.bin").read_bytes() == sn.caller_expected(h, probs)
