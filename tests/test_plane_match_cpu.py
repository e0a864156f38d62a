"""CPU tests of plane association: the host entries drfe_plane_match_host / drfe_plane_flag_points_host /
drfe_plane_match_status_host equal an independent numpy restatement of the reference (tests/plane_match_numpy.py) bit for bit
on randomised scenes and on hand-built cases that reach every branch; a C++ caller of the adaptor's PlaneMatcher and
drfe::FlagMatchedPlanePoints fills the frame's pointer vectors and the map points' flags as the reference does."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_match_numpy as PN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
I4 = np.eye(4, dtype=f32)


def _check(Tcw, coefs, map_coefs, bad, clouds, priors=(None, None, None), params=PN.DEFAULTS):
    from dr_slam_amd import lib
    got = lib.plane_match_host(Tcw, coefs, map_coefs, bad, clouds, *priors, params=np.array(params, f32))
    want = PN.search_map_by_coefficients(Tcw, coefs, map_coefs, bad, clouds, *priors, params=params)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w), (got, want)
    assert got[3] == want[3]
    return got


@pytest.mark.parametrize("seed", range(12))
def test_host_equals_numpy_on_random_scenes(seed):
    from dr_slam_amd import lib
    Tcw, coefs, mc, bad, clouds, pts = PN.random_scene(seed)
    rng = np.random.default_rng(100 + seed)
    P = len(coefs)
    priors = tuple(np.where(rng.random(P) < 0.5, rng.integers(0, len(mc), P), -1).astype(np.int32) for _ in range(3))
    mi, pi, vi, n = _check(Tcw, coefs, mc, bad, clouds, priors)
    _check(Tcw, coefs, mc, bad, clouds)
    prior_flags = (rng.random(len(pts)) < 0.1).astype(np.uint8)
    fl, npair = lib.plane_flag_points_host(Tcw, coefs, mi, pts, prior_flags)
    wfl, wn = PN.flag_matched_plane_points(Tcw, coefs, mi, pts, prior_flags)
    assert np.array_equal(fl, wfl) and npair == wn
    assert np.all(fl >= prior_flags)


def test_random_scenes_reach_every_outcome():
    """the randomised scenes are not vacuous: matches, parallel and vertical assignments, and flags all occur"""
    from dr_slam_amd import lib
    seen = np.zeros(4, int)
    for seed in range(12):
        Tcw, coefs, mc, bad, clouds, pts = PN.random_scene(seed)
        mi, pi, vi, n = lib.plane_match_host(Tcw, coefs, mc, bad, clouds)
        fl, npair = lib.plane_flag_points_host(Tcw, coefs, mi, pts)
        seen += [n, (pi >= 0).sum(), (vi >= 0).sum(), npair]
    assert np.all(seen > 0), seen


def _flat(z, n=8, extra=()):
    """n points of the plane z = const (x, y spread), then `extra` rows"""
    g = np.stack([np.linspace(-1, 1, n), np.linspace(1, -1, n), np.full(n, z)], 1)
    return np.vstack([g] + [np.asarray(e, np.float64).reshape(1, 3) for e in extra]).astype(f32)


Z = np.array([0, 0, 1, -1], f32)            # camera plane z = 1 (identity pose: world plane z = 1)


def test_bad_plane_is_skipped():
    mc = np.array([[0, 0, 1, -1], [0, 0, 1, -1]], f32)
    mi, pi, vi, n = _check(I4, [Z], mc, [1, 0], [_flat(1.0), _flat(1.02)])
    assert list(mi) == [1] and n == 1 and pi[0] == -1


def test_gated_but_far_falls_through_to_parallel():
    mc = np.array([[0, 0, 1, -1]], f32)
    mi, pi, vi, n = _check(I4, [Z], mc, [0], [_flat(1.2)])
    assert mi[0] == -1 and pi[0] == 0 and n == 0


def test_later_plane_replaces_only_with_strictly_smaller_distance():
    mc = np.array([[0, 0, 1, -1]] * 3, f32)
    mi, pi, vi, n = _check(I4, [Z], mc, [0, 0, 0], [_flat(1.05), _flat(1.03), _flat(1.03)])
    assert mi[0] == 1 and pi[0] == 2 and n == 1         # the equal third falls through to the parallel test
    mi, pi, vi, n = _check(I4, [Z], mc[:2], [0, 0], [_flat(1.05), _flat(1.05)])
    assert mi[0] == 0 and pi[0] == 1


def test_priors_are_kept_where_nothing_is_written():
    mc = np.array([[0.6, 0.0, 0.8, 0.0]], f32)          # angle 0.8: no gate, not parallel, not vertical
    mi, pi, vi, n = _check(I4, [Z, Z], mc, [0], [_flat(1.0)], ([7, -1], [3, 4], [-1, 5]))
    assert list(mi) == [7, -1] and list(pi) == [3, 4] and list(vi) == [-1, 5] and n == 0
    mi, pi, vi, n = _check(I4, [Z], np.zeros((0, 4), f32), [], [], ([2], [3], [4]))
    assert (mi[0], pi[0], vi[0], n) == (2, 3, 4, 0)


def test_negative_angles():
    mc = np.array([[0, 0, -1, 1], [0, 0, -1, 5], [0.01, 0.9999, 0.0, 0]], f32)
    mi, pi, vi, n = _check(I4, [Z], mc, [0, 0, 0], [_flat(1.01), _flat(5.0), _flat(0.0)])
    assert mi[0] == 0 and pi[0] == 1 and vi[0] == 2
    mc2 = np.array([[0, -0.02, -0.9998, 0]], f32)
    mi, pi, vi, n = _check(I4, [np.array([0, 1, 0, 0], f32)], mc2, [0], [_flat(9.0)])
    assert vi[0] == 0


def test_parallel_and_vertical_thresholds_tighten():
    def unit(a):                                        # normal with n . (0, 0, 1) = a
        return [np.sqrt(1 - a * a), 0, a, -50]
    mc = np.array([unit(0.997), unit(0.999), unit(0.998), unit(0.05), unit(0.02), unit(0.03), unit(-0.01)], f32)
    mi, pi, vi, n = _check(I4, [Z], mc, [0] * 7, [_flat(50.0)] * 7)
    assert pi[0] == 1 and vi[0] == 6 and mi[0] == -1
    mc = mc[:6]
    mi, pi, vi, n = _check(I4, [Z], mc, [0] * 6, [_flat(50.0)] * 6)
    assert vi[0] == 4
    mi, pi, vi, n = _check(I4, [Z], mc, [0] * 6, [_flat(50.0)] * 6, params=(0.1, 0.86, 0.01, 0.9999))
    assert pi[0] == -1 and vi[0] == -1


def test_zero_negative_zero_and_nan_points():
    mc = np.array([[0, 0, 1, 0]], f32)
    coef = np.array([0, 0, 1, 0], f32)                  # z = 0: the z == 0 points would be at distance 0
    cl = np.array([[1, 1, 0.0], [2, 2, -0.0], [0, 0, np.nan], [np.nan, 0, 0.5], [0, 0, 0.06]], f32)
    mi, pi, vi, n = _check(I4, [coef], mc, [0], [cl])
    assert mi[0] == 0
    assert PN.point_distance_from_plane(PN.world_coef(I4, coef), cl) == float(f32(0.06))
    only_skipped = cl[:3]
    assert PN.point_distance_from_plane(PN.world_coef(I4, coef), only_skipped) == 100.0
    mi, pi, vi, n = _check(I4, [coef], mc, [0], [only_skipped])
    assert mi[0] == -1 and pi[0] == 0


def test_empty_cloud_gives_no_match():
    mc = np.array([[0, 0, 1, -1]], f32)
    mi, pi, vi, n = _check(I4, [Z], mc, [0], [np.zeros((0, 3), f32)])
    assert mi[0] == -1 and pi[0] == 0
    mi, pi, vi, n = _check(I4, [Z], mc, [0], [np.zeros((0, 3), f32)], params=(200.0, 0.86, 0.08716, 0.9962))
    assert mi[0] == 0                                   # 100 < dTh: the empty cloud matches


def test_flags_at_the_half_boundary_and_without_match():
    from dr_slam_amd import lib
    below = np.nextafter(f32(0.5), f32(0))
    pts = np.array([[0, 0, 0.5], [0, 0, below], [0, 0, -0.5], [0, 0, -below], [0, 0, np.nan], [3, 3, 0.0]], f32)
    coef = np.array([0, 0, 1, 0], f32)
    fl, n = lib.plane_flag_points_host(I4, [coef], [0], pts)
    assert list(fl) == [0, 1, 0, 1, 0, 1] and n == 3
    assert (PN.flag_matched_plane_points(I4, [coef], [0], pts)[1]) == 3
    fl, n = lib.plane_flag_points_host(I4, [coef, coef], [-1, 4], pts)        # only non-null planes; the index is not read
    assert list(fl) == [0, 1, 0, 1, 0, 1] and n == 3
    fl, n = lib.plane_flag_points_host(I4, [coef, coef], [2, 2], pts)
    assert n == 6
    fl, n = lib.plane_flag_points_host(I4, [coef], [-1], pts, np.array([1, 0, 0, 0, 0, 0], np.uint8))
    assert list(fl) == [1, 0, 0, 0, 0, 0] and n == 0                          # sticky, never cleared


def test_match_status_both_ways():
    from dr_slam_amd import lib
    c = np.array([[0, 0, 1, -1], [1, 0, 0, -2]], f32)
    matched = np.array([[0, 0.05, 0.99875, -1], [1, 0, 0, -2]], f32)
    ang = PN.angle_of(PN.world_coef(I4, c[0]), matched[0])
    th = np.radians(2.0)
    Rmf = np.array([[1, 0, 0], [0, np.cos(th), np.sin(th)], [0, -np.sin(th), np.cos(th)]], f32)
    ang_mf = PN.angle_of(PN.world_coef(I4, c[0], Rmf), matched[0])
    assert abs(ang_mf) - 0.05 < abs(ang) < abs(ang_mf) - 0.0005
    for mf, R, want in ((True, Rmf, False), (False, None, True), (True, np.eye(3), True)):
        assert lib.plane_match_status_host(I4, c, matched, [1, 1], mf, R) == want
        assert PN.match_status(I4, c, matched, [1, 1], mf, R) == want
    assert lib.plane_match_status_host(I4, c, matched, [0, 1], True, Rmf)        # null / bad: skipped
    assert lib.plane_match_status_host(I4, c[:1], matched[:1], [1], True, Rmf)   # fewer than two planes


@pytest.mark.parametrize("seed", range(4))
def test_match_status_random(seed):
    from dr_slam_amd import lib
    Tcw, coefs, mc, bad, clouds, pts = PN.random_scene(seed)
    rng = np.random.default_rng(seed)
    matched = mc[rng.integers(0, len(mc), len(coefs))]
    m = (rng.random(len(coefs)) < 0.7).astype(np.uint8)
    R = (Tcw[:3, :3].T.astype(np.float64) @ np.array([[1, 0, 0], [0, np.cos(0.01), -np.sin(0.01)], [0, np.sin(0.01), np.cos(0.01)]]))
    for mf in (True, False):
        assert lib.plane_match_status_host(Tcw, coefs, matched, m, mf, R) == PN.match_status(Tcw, coefs, matched, m, mf, R)


ADAPTOR_CALLER = r"""
#include "drfe_adaptor.hpp"
#include <cstdio>
#include <set>
struct Pt { float x, y, z, rgb; };
struct Cloud { std::vector<Pt> points; };
drfe_cv::Mat fmat(int r, int c, const float* v) { drfe_cv::Mat m(r, c, 4); m.step = (size_t)c * 4; std::memcpy(m.data, v, (size_t)r * c * 4); return m; }
struct MapPlane {
    drfe_cv::Mat pos; bool bad = false; Cloud* mvPlanePoints = nullptr; int id = 0;
    bool isBad() const { return bad; }
    drfe_cv::Mat GetWorldPos() const { return pos; }
};
struct MapPoint {
    drfe_cv::Mat pos; bool flag = false; int id = 0;
    drfe_cv::Mat GetWorldPos() const { return pos; }
    void SetAssociatedWithPlaneFlag(bool f) { flag = f; }
};
struct Frame {
    int mnPlaneNum = 0; drfe_cv::Mat mTcw; std::vector<drfe_cv::Mat> mvPlaneCoefficients;
    std::vector<MapPlane*> mvpMapPlanes, mvpParallelPlanes, mvpVerticalPlanes; bool mbNewPlane = true;
};
static float rdf(FILE* f) { float v; if (fread(&v, 4, 1, f) != 1) exit(2); return v; }
static int rdi(FILE* f) { int v; if (fread(&v, 4, 1, f) != 1) exit(2); return v; }
int main(int, char** argv)
{
    FILE* f = fopen(argv[1], "rb");
    Frame F;
    float T[16]; for (float& t : T) t = rdf(f);
    F.mTcw = fmat(4, 4, T);
    F.mnPlaneNum = rdi(f);
    for (int i = 0; i < F.mnPlaneNum; i++) { float c[4]; for (float& v : c) v = rdf(f); F.mvPlaneCoefficients.push_back(fmat(4, 1, c)); }
    const int M = rdi(f);
    std::vector<MapPlane> planes(M); std::vector<Cloud> clouds(M);
    std::vector<MapPlane*> vp;
    for (int j = 0; j < M; j++) {
        float c[4]; for (float& v : c) v = rdf(f);
        planes[j].pos = fmat(4, 1, c); planes[j].bad = rdi(f) != 0; planes[j].id = j;
        const int n = rdi(f);
        for (int k = 0; k < n; k++) { Pt p; p.x = rdf(f); p.y = rdf(f); p.z = rdf(f); p.rgb = 0; clouds[j].points.push_back(p); }
        planes[j].mvPlanePoints = &clouds[j];
        vp.push_back(&planes[j]);
    }
    const int N = rdi(f);
    std::vector<MapPoint> mps(N);
    std::set<MapPoint*> mspMapPoints;
    for (int p = 0; p < N; p++) { float v[3]; for (float& x : v) x = rdf(f); mps[p].pos = fmat(3, 1, v); mps[p].id = p; mspMapPoints.insert(&mps[p]); }
    MapPlane sentinel; sentinel.id = 999;
    F.mvpMapPlanes.assign(F.mnPlaneNum, nullptr); F.mvpParallelPlanes.assign(F.mnPlaneNum, &sentinel); F.mvpVerticalPlanes.assign(F.mnPlaneNum, nullptr);
    Planar_SLAM::PlaneMatcher pm;
    drfe_cv::Mat R;
    const int n = pm.SearchMapByCoefficients(F, vp, R);
    printf("%d %d\n", n, F.mbNewPlane ? 1 : 0);
    for (int i = 0; i < F.mnPlaneNum; i++)
        printf("%d %d %d\n", F.mvpMapPlanes[i] ? F.mvpMapPlanes[i]->id : -1, F.mvpParallelPlanes[i] ? F.mvpParallelPlanes[i]->id : -1,
               F.mvpVerticalPlanes[i] ? F.mvpVerticalPlanes[i]->id : -1);
    const int pairs = drfe::FlagMatchedPlanePoints(F, mspMapPoints, 0.1f);
    std::vector<int> first(N); for (int p = 0; p < N; p++) first[p] = mps[p].flag;
    for (auto& m : mps) m.flag = false;
    const int pairs2 = drfe::FlagMatchedPlanePoints(F, mspMapPoints, 1000.0f);    /* dTh is not read */
    int same = pairs == pairs2;
    for (int p = 0; p < N; p++) same &= first[p] == (int)mps[p].flag;
    printf("%d %d\n", pairs, same);
    for (int p = 0; p < N; p++) printf("%d", first[p]);
    printf("\n");
    const float Rv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    printf("%d %d\n", pm.bMatchStatus(F, vp, false, R) ? 1 : 0, pm.bMatchStatus(F, vp, true, fmat(3, 3, Rv)) ? 1 : 0);
    return 0;
}
"""


def test_adaptor_fills_pointer_vectors_and_flags(tmp_path):
    """A C++ caller of Planar_SLAM::PlaneMatcher and drfe::FlagMatchedPlanePoints (include/drfe_adaptor.hpp) on stand-in Frame /
    MapPlane / MapPoint types: the pointer vectors are written where the reference writes them (a prior non-null parallel
    pointer survives where nothing is assigned), mbNewPlane is cleared, and the map points' flags follow the host entry."""
    from dr_slam_amd import lib
    Tcw, coefs, mc, bad, clouds, pts = PN.random_scene(5)
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        f.write(Tcw.tobytes() + np.int32([len(coefs)]).tobytes() + coefs.tobytes() + np.int32([len(mc)]).tobytes())
        for j in range(len(mc)):
            f.write(mc[j].tobytes() + np.int32([bad[j], len(clouds[j])]).tobytes() + clouds[j].tobytes())
        f.write(np.int32([len(pts)]).tobytes() + pts.tobytes())
    exe, src = tmp_path / "caller", tmp_path / "caller.cpp"
    src.write_text(ADAPTOR_CALLER)
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-ldrfe", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe), str(blob)], check=True, capture_output=True, text=True).stdout.split("\n")
    P = len(coefs)
    mi, pi, vi, n = PN.search_map_by_coefficients(Tcw, coefs, mc, bad, clouds, None, np.full(P, 999), None)
    assert out[0].split() == [str(n), "0"] and n > 0
    rows = [tuple(map(int, ln.split())) for ln in out[1:1 + P]]
    assert rows == [(int(mi[i]), int(pi[i]), int(vi[i])) for i in range(P)]
    fl, npair = PN.flag_matched_plane_points(Tcw, coefs, mi, pts)
    assert out[1 + P].split() == [str(npair), "1"] and npair > 0
    assert out[2 + P] == "".join(str(int(v)) for v in fl)
    mcoef = np.array([mc[m] if m >= 0 else np.zeros(4, f32) for m in mi], f32)
    mm = np.array([m >= 0 and not bad[m] for m in mi], np.uint8)
    want = [PN.match_status(Tcw, coefs, mcoef, mm, False), PN.match_status(Tcw, coefs, mcoef, mm, True, np.eye(3))]
    assert out[3 + P].split() == [str(int(w)) for w in want]
