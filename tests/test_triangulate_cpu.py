"""Host tests of map-point and map-line triangulation: drfe_triangulate_points_host and
drfe_triangulate_lines_host equal the numpy restatement (tests/triangulate_numpy.py) bit for bit on random scenes that reach
every branch and reject code, and on hand-built cases - each threshold one float step on either side of where its decision
flips (5.991 / 7.8 sigma^2, 0.9998, cosParallaxRays > 0, the two ratio tests), equal stereo cosines, z == 0, w == 0,
dist == 0, a rank-deficient A, KF2's residual with KF1's mbf, UnprojectStereo on the distorted keys, the line idx2 quirk in and
out of range, the baseline skip at equality; the canonical atan2f / cosf of include/drfe_math.h are correctly rounded (mpmath)
on the depths and baselines that occur; bad arguments are rejected; and a C++ caller of the adaptor on stand-in types."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulate_numpy as TN  # noqa: E402
import triangulate_scenarios as TS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, F = np.float32, np.float32
KEYS = ("status", "branch", "x3d", "pair_skipped", "accepted")


def _host(scene, line=False):
    from dr_slam_amd import lib
    return (lib.triangulate_lines_host if line else lib.triangulate_points_host)(scene)


def _check(scene, line=False):
    """host == numpy; returns the host's outputs"""
    h = _host(scene, line)
    n = TN.triangulate(scene, line)
    for k in KEYS:
        assert h[k].tobytes() == n[k].tobytes(), k
    return h


@pytest.mark.parametrize("line", [False, True])
def test_host_equals_numpy_on_random_scenes(line):
    seen, branches = set(), set()
    for seed in range(5):
        s = TN.random_scene(np.random.default_rng(100 * line + seed), line=line)
        h = _check(s, line)
        seen |= set((h["status"] & 0x7F).tolist())
        branches |= set(h["branch"].tolist())
        if line:
            seen |= {"past"} if (h["status"] & 0x80).any() else set()
    codes = TN.L_CODES if line else TN.P_CODES
    # w == 0 and a zero distance have measure zero in a random scene, and a line end behind KF2 alone is rare: hand-built below
    rare = {"dist", "z_sp2", "z_ep2"} if line else {"w_zero", "dist"}
    assert {codes[c] for c in codes if c not in rare} <= seen
    assert branches == ({0, 2, 3} if line else {0, 1, 2, 3})
    if line:
        assert "past" in seen


# --- hand-built scenes (tests/triangulate_scenarios.py) ------------------------------------------------------------------------

_pt_scene, _proj, _two, _line_scene = TS.pt_scene, TS.proj, TS.two, TS.line_scene


def _bits_search(name):
    """the gate's flip (the least float32 at which the decision differs from the one at the low end, found with numpy alone);
    the cases at v - 1 ulp, v, v + 1 ulp are checked host == numpy and returned"""
    make, b, d0 = TS.flip_of(name)
    decide = TS.GATES[name]()[3]
    out = []
    for bits in (b - 1, b, b + 1):
        out.append(_check(make(TS.float_of(bits))))
    assert decide(out[0]["status"][0]) == d0 and decide(out[1]["status"][0]) != d0
    return out


@pytest.mark.parametrize("stereo", [False, True])
def test_reprojection_threshold_steps(stereo):
    """5.991 sigma^2 (mono) / 7.8 sigma^2 (stereo), compared in double: KF1's level sigma^2 one step either side"""
    out = _bits_search("reproj_stereo" if stereo else "reproj_mono")
    assert out[0]["status"][0] == TN.P_CODES["reproj1"] and out[1]["status"][0] != TN.P_CODES["reproj1"]


def test_parallax_09998_steps():
    """cosParallaxRays < 0.9998 (a double) for two monocular keypoints: KF2 moved along x one float step at a time"""
    out = _bits_search("parallax_09998")
    assert out[0]["branch"][0] == 0 and out[1]["branch"][0] == 1


def test_cos_rays_positive_steps():
    """cosParallaxRays > 0: KF2 looks along world x, so KF1's keypoint at cx gives perpendicular rays (cos == 0 exactly)"""
    res = [_check(s)["branch"][0] for s in TS.cos_rays_scenes()]
    assert res[1] == 0                                 # cos == 0: not > 0
    assert sorted({res[0], res[2]}) != [0]             # one side is positive


def test_ratio_tests_steps_and_equality():
    make, k1, k2 = TS.ratio_make()
    h = TN.triangulate(make(F(1.2)))
    assert h["status"][0] == 0
    # ratioDist * ratioFactor < ratioOctave flips as KF1's scale grows; ratioDist > ratioOctave * ratioFactor as it shrinks
    _bits_search("ratio_above")
    lo = _bits_search("ratio_below")
    assert lo[1]["status"][0] == TN.P_CODES["scale"]
    # equality of the first test: ratioOctave == ratioDist * ratioFactor exactly is kept (strict <)
    eq, X = TS.ratio_equality_scene()
    h = TN.triangulate(eq)
    _check(eq)
    if h["x3d"][0].tolist() == X.tolist() or h["status"][0] in (0, TN.P_CODES["scale"]):
        assert h["status"][0] in (0, TN.P_CODES["scale"])


def test_equal_stereo_cosines():
    """cosParallaxStereo1 == cosParallaxStereo2 (= cosParallaxRays + 1, rays just past perpendicular): neither stereo
    branch is taken; one depth step nearer, stereo 1 is"""
    out = _bits_search("equal_stereo_cosines")
    assert out[1]["status"][0] == TN.P_CODES["no_parallax"] and out[0]["branch"][0] == 2


def test_z_zero_w_zero_dist_zero_rank_deficient():
    # z1 == 0: the stereo point lands on KF1's plane (Twc and Tcw are independent inputs); low parallax: stereo 1
    h = _check(TS.z_zero_scene())
    assert h["status"][0] == TN.P_CODES["z1"] and h["branch"][0] == 2
    # w == 0: keypoints at the principal point, A's third column zero and its fourth orthogonal to the rest
    h = _check(TS.w_zero_scene())
    assert h["status"][0] == TN.P_CODES["w_zero"] and h["branch"][0] == 1
    # rank-deficient A with w != 0: KF2's first two rows equal KF1's (rows 2, 3 of A repeat rows 0, 1)
    h = _check(TS.rank_deficient_scene())
    assert h["branch"][0] == 1 and h["status"][0] != TN.P_CODES["w_zero"]
    # dist == 0: KF1's centre (GetCameraCenter, an input of its own) on the unprojected point
    h = _check(TS.dist_zero_scene())
    assert h["status"][0] == TN.P_CODES["dist"] and h["branch"][0] == 2


def test_kf2_residual_uses_kf1_mbf():
    s_ok, s_off = TS.kf2_residual_scenes()
    ok = _check(s_ok)
    assert ok["status"][0] == 0
    h = _check(s_off)                                   # KF1's mbf 80, KF2's own stays 40: its residual is now off by 40 / z
    assert h["status"][0] == TN.P_CODES["reproj2"]


def test_unproject_reads_the_distorted_keys():
    k1, p1, s, s2 = TS.distorted_keys_scenes()          # low parallax: stereo 1
    h = _check(s)
    assert h["branch"][0] == 2
    z = F(p1["depth"])
    want = TN._twc(k1["Twc"], [F(F((F(p1["raw"][0]) - k1["cx"]) * z) * k1["invfx"]), F(F((F(p1["raw"][1]) - k1["cy"]) * z) * k1["invfy"]), z])
    if h["status"][0] == 0:
        assert h["x3d"][0].tolist() == [float(v) for v in want]
        assert _check(s2)["x3d"][0].tolist() != h["x3d"][0].tolist()


def test_line_idx2_quirk():
    q = TS.line_idx2_scenes()
    # in range: KF1's line idx2 has depth, KF2's has none: bStereo2 is read from KF1, so stereo 2 is taken
    h = _check(q[0], True)
    assert h["branch"][0] == 3 and h["status"][0] == 0
    # KF1's line idx2 without depth, KF2's with: no line
    h = _check(q[1], True)
    assert h["status"][0] == TN.L_CODES["no_stereo"]
    # idx2 past KF1's lines: bStereo2 false, flagged
    h = _check(q[2], True)
    assert h["status"][0] == TN.L_CODES["no_stereo"] | TN.PAST_KF1
    h = _check(q[3], True)
    assert h["status"][0] == TN.PAST_KF1 and h["branch"][0] == 2 and h["accepted"][0] == 1


def test_line_gates_hand_built():
    g = TS.line_gate_scenes()
    assert _check(g[0], True)["status"][0] == TN.L_CODES["z_sp2"]         # KF2 looks back: sp behind it
    assert _check(g[1], True)["status"][0] == TN.L_CODES["z_ep2"]         # sp in front of KF2, ep behind it
    assert _check(g[2], True)["status"][0] == TN.L_CODES["dist"]


def test_baseline_skip_at_equality():
    eq, above = TS.baseline_scenes()
    h = _check(eq)
    assert h["pair_skipped"][0] == 0
    h = _check(above)
    assert h["pair_skipped"][0] == 1 and h["status"][0] == 1


def test_every_case_holds_on_the_host():
    """every case of the scenario module, as the device tests run them: host == numpy and the case's own expectation"""
    for name, scene, line, expect in TS.cases():
        TS.holds(expect, _check(scene, line))


def test_bad_arguments_are_rejected():
    from dr_slam_amd import lib
    k1, k2, p1, p2 = _two(st1=True)
    s = _pt_scene([k1, k2], [p1], [p2])
    with pytest.raises(lib.DrfeError):
        lib.triangulate_points_host(s, monocular=1)
    for key, val in (("matches", np.int32([[1, 0]])), ("kf2", np.int32([2])), ("octave", np.int32([8, 0]))):
        with pytest.raises(lib.DrfeError):
            lib.triangulate_points_host(dict(s, **{key: val}))
    with pytest.raises(lib.DrfeError):
        lib.triangulate_points_host(dict(s, depth=np.float32([0.0, -1.0])))      # stereo keypoint without depth
    assert lib.triangulate_points_host(dict(s, kf1=s["kf1"][:0], kf2=s["kf2"][:0], match_offsets=np.int32([0]),
                                            matches=s["matches"][:0]))["status"].size == 0


# --- canonical atan2f / cosf ----------------------------------------------------------------------------------------------

def _cr(vals, fn):
    """the correctly rounded float32 of fn (mpmath, 120 bits) at each input tuple"""
    import mpmath
    mpmath.mp.prec = 120
    out = np.empty(len(vals), f32)
    for i, v in enumerate(vals):
        x = fn(*[mpmath.mpf(float(a)) for a in v])
        c = F(float(x))
        best = min((c, np.nextafter(c, F(np.inf)), np.nextafter(c, F(-np.inf))), key=lambda q: abs(mpmath.mpf(float(q)) - x))
        out[i] = best
    return out


def test_canonical_atan2f_cosf_are_correctly_rounded():
    import mpmath
    from dr_slam_amd import lib, synth
    rng = np.random.default_rng(9)
    depth = (np.arange(1, 65536, dtype=np.float32) * (F(1) / F(5000)))            # every 16-bit raw depth, DepthMapFactor 5000
    ys = []
    for cam in (synth.TUM1, synth.TUM2, synth.TUM3):
        ys.append(F(F(cam.bf) / F(cam.fx)) / F(2))
    y = np.concatenate([np.full(len(depth), v, f32) for v in ys] + [np.exp(rng.uniform(-12, 5, 100000)).astype(f32)])
    x = np.concatenate([depth] * len(ys) + [np.exp(rng.uniform(-12, 5, 100000)).astype(f32)])
    got = lib.triangulate_math(0, y, x)
    want = _cr(list(zip(y, x)), mpmath.atan2)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(np.array([TN.atan2f(a, b) for a, b in zip(y[:2000], x[:2000])], f32).view(np.int32),
                          want[:2000].view(np.int32))
    # cosf on [0, pi]: the doubled angles that occur, and random floats of the domain
    ang = np.concatenate([F(2) * got, rng.uniform(0, np.pi, 100000).astype(f32), np.float32([0, np.pi, np.pi / 2])])
    ang = ang[ang <= F(np.pi)]
    gc = lib.triangulate_math(1, ang)
    wc = _cr([(a,) for a in ang], mpmath.cos)
    assert np.array_equal(gc.view(np.int32), wc.view(np.int32))
    assert np.array_equal(lib.triangulate_math(2, F(2) * y, x).view(np.int32), lib.triangulate_math(1, F(2) * got).view(np.int32))
    # the host libm's float functions (what the reference calls) for comparison: printed, not asserted
    m = C.CDLL("libm.so.6")
    m.atan2f.restype = m.cosf.restype = C.c_float
    m.atan2f.argtypes = [C.c_float, C.c_float]
    m.cosf.argtypes = [C.c_float]
    da = sum(1 for a, b, w in zip(y, x, want) if F(m.atan2f(float(a), float(b))) != w)
    dc = sum(1 for a, w in zip(ang, wc) if F(m.cosf(float(a))) != w)
    print(f"libm atan2f differs on {da} of {len(y)}, cosf on {dc} of {len(ang)}")
    assert math.isfinite(da)


ADAPTOR_CALLER = r"""
#include "drfe_adaptor.hpp"
#include <cstdio>
using drfe_cv::Mat;
struct Vec6 { double v[6]; double operator()(int k) const { return v[k]; } };
struct KeyFrame {
    float Tcw[16], Twc[16], Ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf, mfScaleFactor = 1.2f;
    int mnScaleLevels = 8;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvuRight, mvDepth, mvDepthLine;
    std::vector<drfe_cv::KeyPoint> mvKeysUn, mvKeys;
    std::vector<drfe_cv::KeyLine> mvKeyLines;
    std::vector<Vec6> mvLines3D;
    Mat GetPose() const { Mat m(4, 4, 4); std::memcpy(m.data, Tcw, 64); return m; }
    Mat GetPoseInverse() const { Mat m(4, 4, 4); std::memcpy(m.data, Twc, 64); return m; }
    Mat GetCameraCenter() const { Mat m(3, 1, 4); std::memcpy(m.data, Ow, 12); return m; }
};
int main(int, char** argv)
{
    FILE* f = fopen(argv[1], "rb");
    auto rd = [&](void* p, size_t n) { if (fread(p, 1, n, f) != n) exit(2); };
    KeyFrame kf[2];
    for (KeyFrame& k : kf) {
        rd(k.Tcw, 64); rd(k.Twc, 64); rd(k.Ow, 12); rd(&k.fx, 4 * 8);
        k.mvScaleFactors.resize(8); k.mvLevelSigma2.resize(8); rd(k.mvScaleFactors.data(), 32); rd(k.mvLevelSigma2.data(), 32);
        int n; rd(&n, 4);
        k.mvKeysUn.resize(n); k.mvKeys.resize(n); k.mvuRight.resize(n); k.mvDepth.resize(n);
        for (int i = 0; i < n; i++) {
            rd(&k.mvKeysUn[i].pt, 8); rd(&k.mvKeys[i].pt, 8); rd(&k.mvKeysUn[i].octave, 4); k.mvKeys[i].octave = k.mvKeysUn[i].octave;
            rd(&k.mvuRight[i], 4); rd(&k.mvDepth[i], 4);
        }
        rd(&n, 4);
        k.mvKeyLines.resize(n); k.mvDepthLine.resize(n); k.mvLines3D.resize(n);
        for (int i = 0; i < n; i++) {
            rd(&k.mvKeyLines[i].startPointX, 16); rd(&k.mvKeyLines[i].octave, 4); rd(&k.mvDepthLine[i], 4); rd(k.mvLines3D[i].v, 48);
        }
    }
    int np, nl; rd(&np, 4);
    std::vector<std::pair<size_t, size_t>> mp(np), ml;
    for (auto& m : mp) { int a[2]; rd(a, 8); m = {(size_t)a[0], (size_t)a[1]}; }
    rd(&nl, 4); ml.resize(nl);
    for (auto& m : ml) { int a[2]; rd(a, 8); m = {(size_t)a[0], (size_t)a[1]}; }
    for (const auto& r : drfe::TriangulateNewMapPoints(&kf[0], &kf[1], mp))
        printf("P %zu %zu %08x %08x %08x\n", r.idx1, r.idx2, *(const unsigned*)&r.x3D[0], *(const unsigned*)&r.x3D[1], *(const unsigned*)&r.x3D[2]);
    for (const auto& r : drfe::TriangulateNewMapLines(&kf[0], &kf[1], ml)) {
        printf("L %zu %zu", r.idx1, r.idx2);
        for (int k = 0; k < 3; k++) printf(" %08x", *(const unsigned*)&r.sp[k]);
        for (int k = 0; k < 3; k++) printf(" %08x", *(const unsigned*)&r.ep[k]);
        printf("\n");
    }
    /* the device batch form compiles against the same types (it needs a GPU to run) */
    (void)&drfe::Triangulation::Points<KeyFrame, std::vector<std::pair<size_t, size_t>>>;
    (void)&drfe::Triangulation::Lines<KeyFrame, std::vector<std::pair<size_t, size_t>>>;
    return 0;
}
"""


def test_adaptor_caller(tmp_path):
    """drfe::TriangulateNewMapPoints / TriangulateNewMapLines on stand-in KeyFrame types return the accepted matches in order
    with the numpy restatement's points and endpoints"""
    from dr_slam_amd import lib
    # one seed for both: the two scenes share their keyframes
    sp = TN.random_scene(np.random.default_rng(17), n_kf=2, n_feat=120, n_pairs=1, per_pair=(60, 61))
    sl = TN.random_scene(np.random.default_rng(17), n_kf=2, n_feat=120, n_pairs=1, line=True, per_pair=(60, 61))
    assert sp["kf"].tobytes() == sl["kf"].tobytes() and sp["kf1"].tolist() == [0] and sp["kf2"].tolist() == [1]
    blob = b""
    for k in range(2):
        r = sp["kf"][k]
        T = np.concatenate([r["Tcw"], np.float32([0, 0, 0, 1])])
        W = np.concatenate([r["Twc"], np.float32([0, 0, 0, 1])])
        blob += T.tobytes() + W.tobytes() + r["Ow"].tobytes()
        blob += np.float32([r[f] for f in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")]).tobytes()
        blob += sp["scale_factors"][k].tobytes() + sp["level_sigma2"][k].tobytes()
        a, b = sp["offsets"][k], sp["offsets"][k + 1]
        blob += np.int32([b - a]).tobytes()
        for i in range(a, b):
            blob += sp["un"][i].tobytes() + sp["raw"][i].tobytes() + sp["octave"][i:i + 1].tobytes() + \
                sp["u_right"][i:i + 1].tobytes() + sp["depth"][i:i + 1].tobytes()
        a, b = sl["offsets"][k], sl["offsets"][k + 1]
        blob += np.int32([b - a]).tobytes()
        for i in range(a, b):
            blob += sl["ends"][i].tobytes() + sl["octave"][i:i + 1].tobytes() + sl["depth"][i:i + 1].tobytes() + sl["lines3d"][i].tobytes()
    blob += np.int32([len(sp["matches"])]).tobytes() + sp["matches"].astype(np.int32).tobytes()
    blob += np.int32([len(sl["matches"])]).tobytes() + sl["matches"].astype(np.int32).tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    exe, src = tmp_path / "caller", tmp_path / "caller.cpp"
    src.write_text(ADAPTOR_CALLER)
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-ldrfe", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe), str(tmp_path / "in.bin")], check=True, capture_output=True, text=True).stdout.split("\n")
    got_p = [ln.split()[1:] for ln in out if ln.startswith("P ")]
    got_l = [ln.split()[1:] for ln in out if ln.startswith("L ")]
    for s, got, line in ((sp, got_p, False), (sl, got_l, True)):
        want = TN.triangulate(s, line)
        ok = np.nonzero((want["status"] & 0x7F) == 0)[0]
        assert len(ok) > 3 and len(got) == len(ok)
        for g, m in zip(got, ok):
            assert [int(g[0]), int(g[1])] == s["matches"][m].tolist()
            assert [int(v, 16) for v in g[2:]] == want["x3d"][m].view(np.uint32).tolist()
