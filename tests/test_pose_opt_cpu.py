"""CPU (-m "not gpu") tests of PoseOptimization's host entry (drfe_pose_opt_host): every output byte for byte
against the numpy restatement (tests/pose_opt_numpy.py) on behaviour scenes, edge-count and edge-kind mixes and random frames; that
the behaviour scenes take the paths they are named after (through the entry's diagnostics); the refusals and caps; the correctly
rounded cube and the restated LDLT on their own; the planted pose and outliers; the exported symbols and the struct layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_opt_numpy as pn
from dr_slam_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = {k: i for i, k in enumerate(lib.POSE_OPT_DIAG)}


def _host(frames):
    return lib.pose_opt_host(pn.pack(frames))


def test_new_symbols_are_exported_as_declared():
    L = lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drfe.h")).read(), flags=re.S)
    header = " ".join(header.split())
    for decl in ("int drfe_pose_opt_host(const drfe_pose_opt_problems* problems, drfe_pose_opt_out* out);",
                 "int drfe_pose_opt_batch(drfe_ctx* ctx, const drfe_pose_opt_problems* problems, drfe_pose_opt_out* out, void* stream);",
                 "int drfe_pose_opt_stats(drfe_ctx* ctx, int64_t* stats );"):
        assert decl in header, decl
    for name, nargs in (("drfe_pose_opt_host", 2), ("drfe_pose_opt_batch", 4), ("drfe_pose_opt_stats", 2)):
        assert name in lib.SYMBOLS and len(getattr(L, name).argtypes) == nargs
    # the structs as the header lays them out on LP64: 2 int32, 16 pointers, 7 doubles; 11 pointers
    assert C.sizeof(lib.PoseOptProblems) == 8 + 16 * 8 + 7 * 8 and lib.PoseOptProblems.plane_settings.offset == 136
    assert C.sizeof(lib.PoseOptOut) == 11 * 8
    for struct, cls in (("drfe_pose_opt_problems", lib.PoseOptProblems), ("drfe_pose_opt_out", lib.PoseOptOut)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header)
        fields = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", m.group(1))
        assert fields == [f[0] for f in cls._fields_], fields
    for name, value in (("DRFE_POSE_OPT_MAX_FRAMES", lib.POSE_OPT_MAX_FRAMES), ("DRFE_POSE_OPT_MAX_POINTS", lib.POSE_OPT_MAX_POINTS),
                        ("DRFE_POSE_OPT_MAX_LINES", lib.POSE_OPT_MAX_LINES), ("DRFE_POSE_OPT_MAX_PLANES", lib.POSE_OPT_MAX_PLANES),
                        ("DRFE_POSEOPT_DEVICE_FROM", lib.POSEOPT_DEVICE_FROM)):
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
    # what needs no device: the refusal of a call without a context
    P, out, _, _keep = lib._pose_opt_pack(pn.pack([pn.frame(np.random.default_rng(0), 5)]))
    assert L.drfe_pose_opt_batch(None, C.byref(P), C.byref(out), None) == -1
    assert L.drfe_pose_opt_stats(None, None) == -1


def test_cube_is_correctly_rounded_or_not_certified():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(size=2000), rng.normal(size=500) * 1e-5, np.exp(rng.uniform(-200, 200, 500)),
                        [0.0, -0.0, 1.0, -1.0, 3.0, 1e-5, 0.5, 2.0 ** -400, 2.0 ** 400, np.inf, np.nan,
                         262143.0, 208063.0]])      # 262143^3 has 54 bits (a tie); 208063^3 fits 53
    got, ok = lib.cr_cube(x)
    want = np.array([pn.cr_cube(v) for v in x])
    assert ok[:3000].all()                           # every ordinary argument is certified
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))
    assert not ok[list(x).index(262143.0)] and ok[list(x).index(208063.0)]
    assert not ok[-3] and not ok[-4] and not ok[-5] and not ok[-6]      # NaN, inf, 2^400, 2^-400: left to the caller


def test_ldlt_matches_the_restatement_and_solves():
    rng = np.random.default_rng(4)
    for trial in range(40):
        A = rng.normal(size=(8, 6))
        H = A.T @ A * 10.0 ** rng.integers(-3, 6)
        if trial % 4 == 1:
            H[:, 2] = 0
            H[2, :] = 0                              # a zero pivot in the middle: positive semi-definite
        if trial % 4 == 2:
            H[3, 3] = -H[3, 3]                       # indefinite
        b = rng.normal(size=6)
        pos, x = lib.pose_opt_ldlt(H, b)
        want_pos, want_x = pn.ldlt_solve(H.tolist(), b.tolist())
        assert pos == want_pos
        if pos:
            assert np.array_equal(x.view(np.uint64), np.array(want_x).view(np.uint64))
            if trial % 4 in (0, 3):
                assert np.allclose(H @ x, b, rtol=1e-6, atol=1e-6 * np.abs(b).max())
        assert pos == (trial % 4 != 2)
    pos, x = lib.pose_opt_ldlt(np.zeros((6, 6)), rng.normal(size=6))     # isPositive() of a zero matrix, x = 0
    assert pos and not x.any()


def test_plane_error_takes_both_sign_flips_and_the_negative_dot():
    """Converter::toPlane3D negates a measured plane with d < 0; Plane3D's operator* negates the transformed map plane when its d
    comes out below zero; ominus_par negates the normal when the dot product is negative.  Each case against the restatement."""
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(60):
        fr = pn.frame(rng, 0, 0, planes=(7,))
        meas, world, Tcw = fr["plane_meas"][0], fr["plane_world"][0], fr["Tcw"]
        q, t = pn.to_se3quat(Tcw)
        for kind in (3, 4, 5):
            w = world[4 * (kind - 3):4 * (kind - 3) + 4].copy()
            if rng.random() < 0.5:
                w[3] = 0.05                          # a map plane near the world origin: its d may flip under the pose
            e = lib.pose_opt_plane_error(kind, meas, w, Tcw)
            want = pn.plane_error(kind, pn.to_plane3d(meas), pn.to_plane3d(w), q, t)
            assert np.array_equal(e.view(np.uint64), np.array(want).view(np.uint64)), (kind, e, want)
            X = pn.to_plane3d(w)
            R = np.array(pn.quat_matrix(q))
            l = R @ X[:3]
            d_local = X[3] - np.dot(t, l)
            seen.add(("meas_flip", bool(meas[3] < 0)))
            seen.add(("local_flip", bool(d_local < 0)))
            if kind == 4:
                lp = l if d_local >= 0 else -l
                seen.add(("par_negative_dot", bool(np.dot(pn.to_plane3d(meas)[:3], lp) < 0)))
    assert seen == {(k, v) for k in ("meas_flip", "local_flip", "par_negative_dot") for v in (False, True)}


def test_behaviour_scenes_take_their_paths_and_equal_the_restatement():
    B = pn.behaviour_frames()
    names = list(B)
    h = _host([B[k] for k in names])
    d = {k: dict(zip(lib.POSE_OPT_DIAG, h["diag"][i][:6].tolist())) for i, k in enumerate(names)}
    i = names.index("all_outliers")
    assert d["all_outliers"]["empty_rounds"] == 3 and h["rounds"][i] == 4 and h["returns"][i] == 0
    assert h["point_outlier"][pn.pack([B[k] for k in names])["point_offsets"][i]:][:12].all()
    assert d["points"]["rejected"] > 0 and d["points"]["nbad_stops"] >= 1            # rejected trials, the _nBad >= 3 stop
    assert d["points"]["last_rejected"] >= 1                                         # the stale-error quirk's precondition
    assert d["points"]["small_theta"] > 0 and d["points"]["big_theta"] > 0
    # Zc == 0: the errors are not finite from the first pass on, every trial is rejected, the pose comes back as it went in
    i = names.index("zc_zero")
    assert d["zc_zero"]["rejected"] == h["trials"][i] > 0 and np.array_equal(h["Tcw"][i], B["zc_zero"]["Tcw"])
    assert not h["point_outlier"][pn.pack([B[k] for k in names])["point_offsets"][i]]     # chi2 > th is false for a NaN: an inlier
    i = names.index("zc_negative")
    assert np.isfinite(h["Tcw"][i]).all() and h["point_outlier"][pn.pack([B[k] for k in names])["point_offsets"][i] + 1]
    assert pn.tables_equal(h, pn.numpy_table("behaviour", [B[k] for k in names])) == []


@pytest.mark.parametrize("which", ("size", "mix"))
def test_sizes_and_mixes_equal_the_restatement(which):
    S = pn.size_frames() if which == "size" else pn.mix_frames()
    names = list(S)
    h = _host([S[k] for k in names])
    assert pn.tables_equal(h, pn.numpy_table(which, [S[k] for k in names])) == []
    r = dict(zip(names, zip(h["returns"].tolist(), h["rounds"].tolist())))
    if which == "size":
        for k in ("0", "2"):                         # fewer than 3 correspondences: 0, no round, the pose untouched
            assert r[k] == (0, 0) and np.array_equal(h["Tcw"][names.index(k)], S[k]["Tcw"])
        assert r["2_lines_as_4_edges"] == (0, 0)     # two lines are two correspondences, however many edges
        assert r["3"][1] == 1 and r["9"][1] == 1 and r["9_lines"][1] == 1            # edges().size() < 10 ends the loop
        assert r["10"][1] == 4 and r["10_lines"][1] == 4
    else:
        for name in ("m", "p", "v", "mpv", "3slots"):
            # bStruct off ignores the parallel and vertical map planes: the same outputs as with only the matched bit set
            f = dict(S[f"planes_{name}_struct0"])
            g = dict(f, plane_mask=f["plane_mask"] & pn.MATCHED, plane_world=f["plane_world"] * np.repeat([1, 0, 0], 4).astype(np.float32) + np.repeat([0, 1, 1], 4).astype(np.float32))
            a, b = _host([f]), _host([g])
            assert pn.tables_equal(a, b) == [] and not a["par_plane_outlier"].any() and not a["ver_plane_outlier"].any()


def test_random_frames_equal_the_restatement():
    frames = pn.random_frames()
    assert max(len(f["u_right"]) + 2 * len(f["line_fn"]) + 3 * len(f["plane_mask"]) for f in frames) <= 200
    assert pn.tables_equal(_host(frames), pn.numpy_table("random", frames)) == []


@pytest.mark.parametrize("n", (0, 1, 2, 63, 64, 65, 300))
def test_frames_per_call(n):
    rng = np.random.default_rng(n)
    frames = [pn.frame(rng, 12, 1) for _ in range(n)]
    h = _host(frames)
    assert h["Tcw"].shape == (n, 16) and len(h["point_outlier"]) == 12 * n
    if n:
        # a frame's outputs do not depend on its neighbours in the call
        one = _host(frames[-1:])
        assert np.array_equal(one["Tcw"][0], h["Tcw"][-1]) and one["returns"][0] == h["returns"][-1]
        assert (h["rounds"] == 4).all()


def test_caps_run_and_one_above_is_refused():
    rng = np.random.default_rng(9)
    big = pn.frame(rng, lib.POSE_OPT_MAX_POINTS, lib.POSE_OPT_MAX_LINES, planes=(7,) * lib.POSE_OPT_MAX_PLANES, b_struct=1)
    h = _host([big])
    assert h["rounds"][0] == 4 and np.isfinite(h["Tcw"]).all()
    assert np.abs(h["Tcw"][0] - big["true_Tcw"].reshape(16)).max() < 0.01
    h = _host([pn.frame(rng, 1000, outlier_frac=0.1)])
    assert h["rounds"][0] == 4
    for kw in (dict(n_points=lib.POSE_OPT_MAX_POINTS + 1), dict(n_points=3, n_lines=lib.POSE_OPT_MAX_LINES + 1),
               dict(n_points=3, planes=(1,) * (lib.POSE_OPT_MAX_PLANES + 1))):
        with pytest.raises(lib.DrfeError):
            _host([pn.frame(rng, **kw)])
    P = pn.pack([pn.frame(rng, 3)] * (lib.POSE_OPT_MAX_FRAMES + 1))
    with pytest.raises(lib.DrfeError):
        lib.pose_opt_host(P)
    assert len(lib.pose_opt_host(pn.pack([pn.frame(rng, 3)] * lib.POSE_OPT_MAX_FRAMES))["returns"]) == lib.POSE_OPT_MAX_FRAMES
    bad = pn.pack([pn.frame(rng, 5), pn.frame(rng, 5)])
    bad["point_offsets"] = np.array([0, 7, 5], np.int32)
    with pytest.raises(lib.DrfeError):
        lib.pose_opt_host(bad)


# Planted check (sanity, not parity).  Seed 31: 150 points, 20 % of them moved by 25 .. 80 px, pixel noise 0.7 px per level sigma,
# a start 0.02 rad and ~5 cm off.  On the numpy restatement alone the recovered pose differs from the planted one by at most
# 9.5e-4 in any element of the 4x4 (measured here, on the CPU: the test prints it); the tolerance that passes there, 1e-3, is the
# assertion's tolerance for the host entry as well.
PLANTED_SEED = 31
PLANTED_TOL = 1e-3


def test_planted_pose_and_outliers():
    fr = pn.frame(np.random.default_rng(PLANTED_SEED), 150, 6, outlier_frac=0.2)
    n = pn.pose_optimization(fr)
    err_numpy = np.abs(n["Tcw"] - fr["true_Tcw"].reshape(16)).max()
    print("planted: numpy restatement max |Tcw - planted| =", err_numpy)
    assert err_numpy < PLANTED_TOL
    h = _host([fr])
    assert np.abs(h["Tcw"][0] - fr["true_Tcw"].reshape(16)).max() < PLANTED_TOL
    planted = fr["planted_outlier"]
    assert planted.sum() >= 20
    assert h["point_outlier"][planted].all()                     # every planted outlier is flagged
    assert h["point_outlier"][~planted].mean() < 0.1             # and few of the others (5 % expected from the chi2 test itself)
    assert h["returns"][0] == 150 + 6 - h["point_outlier"].sum() - h["line_outlier"].sum()


@pytest.mark.parametrize("mode", ("host", "auto"))
def test_native_caller_on_the_host_entry(tmp_path, mode):
    """tests/native/pose_opt_caller.cpp: Planar_SLAM::Optimizer::PoseOptimization frame by frame, then drfe::PoseOptBatch over all
    frames, forced to the host entry or left at DRFE_POSEOPT_DEVICE_FROM (64 frames: these four go to the host entry), against the ctypes path"""
    import subprocess
    import native_build
    exe = native_build.caller("pose_opt_caller")          # built here if the tests directory holds no build products
    frames = pn.caller_frames()
    (tmp_path / "in.bin").write_bytes(pn.caller_blob(frames))
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "pose_opt_caller ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    h = _host(frames)
    assert h["returns"][2] == 0 and np.array_equal(h["Tcw"][2], frames[2]["Tcw"])     # fewer than 3: SetPose is not called
    assert (tmp_path / "out.bin").read_bytes() == pn.caller_expected(h, frames)
