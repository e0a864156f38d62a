"""CPU (-m "not gpu") tests of TranslationOptimization's host entry (drfe_trans_opt_host): every output byte
for byte against the numpy restatement (tests/trans_opt_numpy.py) on behaviour scenes, the counting rules, edge-count and edge-kind
mixes and random frames; that the scenes take the paths they are named after (through the entry's diagnostics); the zero-rotation
property; the refusals and caps; the three translation-only plane errors on their own; the planted translation and outliers; the
exported symbols; the native caller."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_opt_numpy as pn
import trans_opt_numpy as tn
from dr_slam_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = {k: i for i, k in enumerate(lib.POSE_OPT_DIAG)}


def _host(frames):
    return lib.trans_opt_host(tn.pack(frames))


def _diag(h, i):
    return dict(zip(lib.POSE_OPT_DIAG, h["diag"][i][:6].tolist()))


def test_new_symbols_are_exported_as_declared():
    L = lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drfe.h")).read(), flags=re.S)
    header = " ".join(header.split())
    debug = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drfe_debug.h")).read(), flags=re.S)
    debug = " ".join(debug.split())
    for decl in ("int drfe_trans_opt_host(const drfe_pose_opt_problems* problems, drfe_pose_opt_out* out);",
                 "int drfe_trans_opt_batch(drfe_ctx* ctx, const drfe_pose_opt_problems* problems, drfe_pose_opt_out* out, void* stream);",
                 "int drfe_trans_opt_stats(drfe_ctx* ctx, int64_t* stats );"):
        assert decl in header, decl
    for decl in ("int drfe_debug_trans_opt_plane_error(int kind, const float* meas, const float* world, const float* Tcw, double* e);",
                 "int drfe_debug_trans_opt_hand_back(drfe_ctx* ctx, int every);"):
        assert decl in debug, decl
    for name, nargs in (("drfe_trans_opt_host", 2), ("drfe_trans_opt_batch", 4), ("drfe_trans_opt_stats", 2),
                        ("drfe_debug_trans_opt_plane_error", 5), ("drfe_debug_trans_opt_hand_back", 2)):
        assert name in lib.SYMBOLS and len(getattr(L, name).argtypes) == nargs
    assert re.search(r"\bDRFE_TRANSOPT_DEVICE_FROM = %d\b" % lib.TRANSOPT_DEVICE_FROM, header)
    # the kernel's boundaries the size scenes are built around
    internal = open(os.path.join(ROOT, "dr_slam_amd", "csrc", "trans_opt_internal.h")).read()
    for name, value in (("TO_THREADS", tn.TO_THREADS), ("TO_PLANE_GROUP", tn.TO_PLANE_GROUP), ("TO_WAVE", tn.TO_WAVE)):
        assert re.search(r"#define %s %d\b" % (name, value), internal), name
    # what needs no device: the refusal of a call without a context
    P, out, _, _keep = lib._pose_opt_pack(tn.pack([tn.tframe(np.random.default_rng(0), 5)]))
    assert L.drfe_trans_opt_batch(None, C.byref(P), C.byref(out), None) == -1
    assert L.drfe_trans_opt_stats(None, None) == -1
    assert L.drfe_debug_trans_opt_hand_back(None, 2) == -1


def test_float_rotation_is_gemm_s_small_matrix_path():
    """R_cw * Xw in the restatement is a float dot left to right: on some of these points it is not the double product rounded
    once, and it is always a float widened"""
    rng = np.random.default_rng(11)
    R = pn.rot(rng.normal(size=3), 0.7).astype(np.float32)
    X = rng.uniform(-3, 3, (2000, 3)).astype(np.float32)
    got = tn.gemm_rotate(R, X)
    once = (X.astype(np.float64) @ R.astype(np.float64).T).astype(np.float32).astype(np.float64)
    assert (got != once).any() and np.abs(got - once).max() < 1e-5
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))          # floats widened


def test_plane_errors_with_the_sign_flip_against_the_restatement():
    """The three translation-only plane edges through the debug hook: toPlane3D of both planes, rotateNormal by the float R_cw,
    localPlane = w2n + Xc with the whole vector negated when d - t . n < 0, ominus / ominus_par / ominus_ver"""
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(60):
        fr = tn.tframe(rng, 0, 0, planes=(7,))
        meas, world, Tcw = fr["plane_meas"][0], fr["plane_world"][0], fr["Tcw"]
        R = np.asarray(Tcw, np.float32).reshape(4, 4)[:3, :3]
        _, t = pn.to_se3quat(Tcw)
        for kind in (3, 4, 5):
            w = world[4 * (kind - 3):4 * (kind - 3) + 4].copy()
            if rng.random() < 0.5:
                w[3] = 0.05                          # a map plane near the world origin: d - t . n may come out below zero
            e = lib.trans_opt_plane_error(kind, meas, w, Tcw)
            Xc = tn.rotate_normal(R, pn.to_plane3d(w))
            want = tn.plane_error(kind, pn.to_plane3d(meas), Xc, t)
            assert np.array_equal(e.view(np.uint64), np.array(want).view(np.uint64)), (kind, e, want)
            d_local = Xc[3] - np.dot(t, Xc[:3])
            seen.add(("meas_flip", bool(meas[3] < 0)))
            seen.add(("local_flip", bool(d_local < 0)))
            if kind == 4:
                lp = np.array(Xc[:3]) * (1 if d_local >= 0 else -1)
                seen.add(("par_negative_dot", bool(np.dot(pn.to_plane3d(meas)[:3], lp) < 0)))
    assert seen == {(k, v) for k in ("meas_flip", "local_flip", "par_negative_dot") for v in (False, True)}
    # under the planted rotation the rotated map plane is the measured one: the matched edge's error is noise
    fr = tn.tframe(np.random.default_rng(6), 0, 0, planes=(1,), start_trans=0.0)
    e = lib.trans_opt_plane_error(3, fr["plane_meas"][0], fr["plane_world"][0][:4], fr["Tcw"])
    assert np.abs(e).max() < 0.02


def test_behaviour_scenes_take_their_paths_and_equal_the_restatement():
    B = tn.behaviour_frames()
    names = list(B)
    frames = [B[k] for k in names]
    h = _host(frames)
    po = tn.pack(frames)["point_offsets"]
    d = {k: _diag(h, i) for i, k in enumerate(names)}
    i = names.index("all_outliers")                  # every point an outlier after round one
    assert d["all_outliers"]["empty_rounds"] == 3 and h["rounds"][i] == 4 and h["returns"][i] == 0
    assert h["point_outlier"][po[i]:po[i + 1]].all()
    assert d["points"]["rejected"] > 0 and d["points"]["nbad_stops"] >= 1            # rejected trials, the _nBad >= 3 stop
    assert d["points"]["last_rejected"] >= 1                                         # a round whose last trial is rejected
    i = names.index("zc_negative")                   # a negative depth: finite everywhere, the point is flagged
    assert np.isfinite(h["Tcw"][i]).all() and h["point_outlier"][po[i] + 1]
    # the zero-rotation property: no update ever has theta at or above 1e-5 on a finite scene
    assert all(d[k]["big_theta"] == 0 and d[k]["small_theta"] == h["trials"][j] > 0 for j, k in enumerate(names))
    # a wrong start rotation stays: the rotation block of the result is the input's up to the float rounding of a unit quaternion
    i = names.index("wrong_rotation")
    Tin, Tout = B["wrong_rotation"]["Tcw"].reshape(4, 4), h["Tcw"][i].reshape(4, 4)
    assert np.abs(Tout[:3, :3] - Tin[:3, :3]).max() < 5e-7 and np.abs(Tout[:3, 3] - Tin[:3, 3]).max() > 1e-3
    assert np.abs(Tin[:3, :3] - B["wrong_rotation"]["true_Tcw"][:3, :3]).max() > 5e-3
    assert tn.tables_equal(h, tn.numpy_table("behaviour", frames)) == []


def test_nonfinite_scenes_flow_through_the_full_form():
    """Zc + t_z == 0 on a mono and on a stereo edge: the error is not finite, 0 * inf reaches the rotation rows of H and b, every
    solve is NaN (theta is not below 1e-5), every trial is rejected and the pose comes back as it went in"""
    B = tn.nonfinite_frames()
    names = list(B)
    frames = [B[k] for k in names]
    h = _host(frames)
    po = tn.pack(frames)["point_offsets"]
    for i, k in enumerate(names):
        d = _diag(h, i)
        assert d["rejected"] == h["trials"][i] > 0 and d["big_theta"] == h["trials"][i] and d["small_theta"] == 0, (k, d)
        assert np.array_equal(h["Tcw"][i], B[k]["Tcw"])
        assert not h["point_outlier"][po[i]]         # chi2 > th is false for a NaN: an inlier
    assert tn.tables_equal(h, tn.numpy_table("nonfinite", frames)) == []


def test_counting_rules():
    S = tn.counting_frames()
    names = list(S)
    frames = [S[k] for k in names]
    h = _host(frames)
    assert tn.tables_equal(h, tn.numpy_table("counting", frames)) == []
    P = tn.pack(frames)
    r = dict(zip(names, zip(h["returns"].tolist(), h["rounds"].tolist())))
    for k in ("0", "2", "2_points_5_lines_3_planes"):   # fewer than 3 points: 0, no round, the pose untouched, nothing flagged
        i = names.index(k)
        assert r[k] == (0, 0) and np.array_equal(h["Tcw"][i], S[k]["Tcw"]) and h["iterations"][i] == 0
    assert r["3"][1] == 1
    assert r["3_points_3_lines"][1] == 1 and r["4_points_3_lines"][1] == 4           # 9 edges: one round; 10 edges: four
    # three inlier points, four plane edges that are outliers: nInitialCorrespondences - nBad is negative and returned as it is
    i = names.index("negative_return")
    so = P["plane_offsets"]
    flagged = sum(int(h[k][so[i]:so[i + 1]].sum()) for k in ("plane_outlier", "par_plane_outlier", "ver_plane_outlier"))
    assert flagged == 4 and not h["point_outlier"][P["point_offsets"][i]:P["point_offsets"][i + 1]].any() and r["negative_return"][0] == -1
    # line outliers go to nLineBad, which is not returned
    i, j = names.index("lines_all_outliers"), names.index("lines_removed")
    lo = P["line_offsets"]
    assert lo[i + 1] - lo[i] == 4 and h["line_outlier"][lo[i]:lo[i + 1]].all()
    assert r["lines_all_outliers"][0] == r["lines_removed"][0] == 30 - h["point_outlier"][P["point_offsets"][i]:P["point_offsets"][i + 1]].sum()


@pytest.mark.parametrize("which", ("size", "mix"))
def test_sizes_and_mixes_equal_the_restatement(which):
    S = tn.size_frames() if which == "size" else tn.mix_frames()
    names = list(S)
    h = _host([S[k] for k in names])
    assert tn.tables_equal(h, tn.numpy_table(which, [S[k] for k in names])) == []
    assert (h["diag"][:, DIAG["big_theta"]] == 0).all()                              # the zero-rotation property
    if which == "size":
        r = dict(zip(names, h["rounds"].tolist()))
        assert r["9"] == 1 and r["10"] == 4
        edges = {k: len(S[k]["u_right"]) + 2 * len(S[k]["line_fn"]) for k in names}
        for n in (tn.TO_WAVE, tn.TO_THREADS):        # one below, at and one above a wavefront and a pass's chunk
            assert [edges[str(n + o)] for o in (-1, 0, 1)] == [n - 1, n, n + 1]
        assert edges["250+2x4"] == tn.TO_THREADS + 2                                 # lines across the chunk's end
        for n in (tn.TO_PLANE_GROUP - 1, tn.TO_PLANE_GROUP, tn.TO_PLANE_GROUP + 1):   # plane edges of a pass
            f = S[f"{n}_planes"]
            assert sum(bin(int(m)).count("1") for m in f["plane_mask"]) == n and f["b_struct"]
    else:
        for name in ("m", "p", "v", "mpv", "3slots"):
            # bStruct off ignores the parallel and vertical map planes: the same outputs as with only the matched bit set
            f = dict(S[f"planes_{name}_struct0"])
            g = dict(f, plane_mask=f["plane_mask"] & tn.MATCHED, plane_world=f["plane_world"] * np.repeat([1, 0, 0], 4).astype(np.float32) + np.repeat([0, 1, 1], 4).astype(np.float32))
            a, b = _host([f]), _host([g])
            assert tn.tables_equal(a, b) == [] and not a["par_plane_outlier"].any() and not a["ver_plane_outlier"].any()


def test_random_frames_equal_the_restatement():
    frames = tn.random_frames()
    assert len(frames) == 20 and max(len(f["u_right"]) + 2 * len(f["line_fn"]) + 3 * len(f["plane_mask"]) for f in frames) <= 200
    h = _host(frames)
    assert tn.tables_equal(h, tn.numpy_table("random", frames)) == []
    assert (h["diag"][:, DIAG["big_theta"]] == 0).all()


@pytest.mark.parametrize("n", (0, 1, 2, 63, 64, 65, 300))
def test_frames_per_call(n):
    rng = np.random.default_rng(n)
    frames = [tn.tframe(rng, 12, 1) for _ in range(n)]
    h = _host(frames)
    assert h["Tcw"].shape == (n, 16) and len(h["point_outlier"]) == 12 * n
    if n:
        # a frame's outputs do not depend on its neighbours in the call
        one = _host(frames[-1:])
        assert np.array_equal(one["Tcw"][0], h["Tcw"][-1]) and one["returns"][0] == h["returns"][-1]
        assert (h["rounds"] == 4).all()


def test_caps_run_and_one_above_is_refused():
    rng = np.random.default_rng(9)
    big = tn.tframe(rng, lib.POSE_OPT_MAX_POINTS, lib.POSE_OPT_MAX_LINES, planes=(7,) * lib.POSE_OPT_MAX_PLANES, b_struct=1)
    h = _host([big])
    assert h["rounds"][0] == 4 and np.isfinite(h["Tcw"]).all()
    assert np.abs(h["Tcw"][0] - big["true_Tcw"].reshape(16)).max() < 0.01
    # the refusals' messages are the context's: tests/test_gpu_trans_opt.py reads them from the batch entry
    for kw in (dict(n_points=lib.POSE_OPT_MAX_POINTS + 1), dict(n_points=3, n_lines=lib.POSE_OPT_MAX_LINES + 1),
               dict(n_points=3, planes=(1,) * (lib.POSE_OPT_MAX_PLANES + 1))):
        with pytest.raises(lib.DrfeError):
            _host([tn.tframe(rng, **kw)])
    with pytest.raises(lib.DrfeError):
        lib.trans_opt_host(tn.pack([tn.tframe(rng, 3)] * (lib.POSE_OPT_MAX_FRAMES + 1)))
    assert len(lib.trans_opt_host(tn.pack([tn.tframe(rng, 3)] * lib.POSE_OPT_MAX_FRAMES))["returns"]) == lib.POSE_OPT_MAX_FRAMES
    bad = tn.pack([tn.tframe(rng, 5), tn.tframe(rng, 5)])
    bad["point_offsets"] = np.array([0, 7, 5], np.int32)
    with pytest.raises(lib.DrfeError):
        lib.trans_opt_host(bad)


# Planted check (sanity, not parity).  tn.planted_frame(): 150 points, 6 lines, 20 % of the points moved by 25 .. 80 px, pixel noise
# 0.7 px per level sigma, the start rotation the planted one and the start translation ~5 cm off.  On the numpy restatement alone
# the recovered pose differs from the planted one by PLANTED_NUMPY_ERR in its worst element (measured on the CPU: the test prints
# it); four times that is the tolerance, for the restatement, the host and the device entry alike.
PLANTED_NUMPY_ERR = 1.64e-3
PLANTED_TOL = 4 * PLANTED_NUMPY_ERR


def test_planted_translation_and_outliers():
    fr = tn.planted_frame()
    n = tn.translation_optimization(fr)
    err_numpy = np.abs(n["Tcw"] - fr["true_Tcw"].reshape(16)).max()
    print("planted: numpy restatement max |Tcw - planted| =", err_numpy)
    assert err_numpy < PLANTED_TOL
    h = _host([fr])
    assert np.abs(h["Tcw"][0] - fr["true_Tcw"].reshape(16)).max() < PLANTED_TOL
    planted = fr["planted_outlier"]
    assert planted.sum() >= 20
    assert h["point_outlier"][planted].all()                     # every planted outlier is flagged
    assert h["point_outlier"][~planted].mean() < 0.1             # and few of the others (5 % expected from the chi2 test itself)
    assert h["returns"][0] == 150 - h["point_outlier"].sum()     # lines neither add nor take


@pytest.mark.parametrize("mode", ("host", "auto"))
def test_native_caller_on_the_host_entry(tmp_path, mode):
    """tests/native/trans_opt_caller.cpp: Planar_SLAM::Optimizer::TranslationOptimization frame by frame, then drfe::TransOptBatch
    over all frames, forced to the host entry or left at DRFE_TRANSOPT_DEVICE_FROM (these four frames go to the host entry),
    against the ctypes path"""
    import subprocess
    import native_build
    exe = native_build.caller("trans_opt_caller")          # built here if the tests directory holds no build products
    frames = tn.caller_frames()
    assert len(frames) < lib.TRANSOPT_DEVICE_FROM
    (tmp_path / "in.bin").write_bytes(pn.caller_blob(frames))
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "trans_opt_caller ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
    h = _host(frames)
    # two points with four lines and a plane: fewer than 3 points, SetPose is not called
    assert h["returns"][2] == 0 and np.array_equal(h["Tcw"][2], frames[2]["Tcw"])
    assert (tmp_path / "out.bin").read_bytes() == pn.caller_expected(h, frames)
