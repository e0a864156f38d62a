"""Host tests of map-point and map-line upkeep: drfe_map_point_upkeep_host and drfe_map_line_upkeep_host
equal the numpy restatement (tests/map_upkeep_numpy.py) bit for bit on random scenes with 1 to 300 observations per item and
on hand-built cases - median ties, even and odd N, bad keyframes interleaved, all keyframes bad, no observations, a bad
keyframe that still counts in the normal, the zero-length viewing ray, the line's full matrix - plus a C++ caller of the
adaptor's drfe::UpkeepMapPoint / drfe::UpkeepMapLine on stand-in types, the observations[pRefKF] quirk included."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_upkeep_numpy as MU  # noqa: E402
import map_upkeep_scenarios as MS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
KEYS = ("best_obs", "desc", "normal", "max_distance", "min_distance", "status", "frustum")


def _host(scene, line=False, what=3):
    from dr_slam_amd import lib
    return (lib.map_line_upkeep_host if line else lib.map_point_upkeep_host)(scene, what)


def _assert_same(got, want):
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k


_flip, _scene, BASE = MS.flip, MS.scene, MS.BASE          # the hand-built items: tests/map_upkeep_scenarios.py


@pytest.mark.parametrize("line", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_host_equals_numpy_on_random_scenes(line, seed):
    rng = np.random.default_rng(1000 * line + seed)
    counts = np.concatenate([rng.integers(0, 11, 150), rng.integers(11, 70, 12), [1, 2, 3, 4, 5, 16, 17, 64, 65],
                             rng.integers(100, 301, 2)])
    rng.shuffle(counts)
    scene = MU.random_scene(rng, counts, line=line, flips=(0, 6 if seed % 2 else 30))
    got = _host(scene, line)
    _assert_same(got, MU.upkeep(scene, line=line))
    assert (got["status"] & 1).sum() > 100 and (got["status"] & 2).sum() > 100


@pytest.mark.parametrize("what", [1, 2])
def test_halves_are_independent(what):
    rng = np.random.default_rng(5)
    scene = MU.random_scene(rng, rng.integers(0, 12, 80))
    got, both = _host(scene, what=what), _host(scene)
    _assert_same(got, MU.upkeep(scene, what=what))
    if what == 1:
        assert np.array_equal(got["best_obs"], both["best_obs"]) and not got["normal"].any() and not (got["status"] & 2).any()
    else:
        assert np.array_equal(got["normal"].view(np.uint32), both["normal"].view(np.uint32)) and (got["best_obs"] == -1).all()


def test_median_tie_first_row_wins():
    """a far row first, then three rows 8 apart: medians 40, 8, 8, 8 - the first of the tied rows (1) wins"""
    rows = MS.tie_rows()
    for line in (False, True):
        s = _scene(rows, line=line)
        got = _host(s, line)
        assert got["best_obs"][0] == 1 and got["desc"][0].tobytes() == rows[1].tobytes()
        _assert_same(got, MU.upkeep(s, line=line))


@pytest.mark.parametrize("N,expect", [(1, 0), (2, 0), (3, 1), (4, 0)])
def test_small_and_even_n(N, expect):
    """N = 1 and 2: the median index is 0, so row 0 wins.  N = 3: a far row, then B and B^{30,31}: medians 30, 2, 2, so
    row 1.  N = 4: B, B^{0,1}, B^{0..9}, B^{200..249}: the lower median (index 1) ties rows 0 and 1 at 2, so row 0; the
    upper median would have picked row 1 (8 against 10)."""
    rows, win = MS.small_n_rows(N)
    assert win == expect
    s = _scene(rows)
    got = _host(s)
    assert got["best_obs"][0] == expect
    _assert_same(got, MU.upkeep(s))


def test_bad_keyframes_interleaved():
    """observations of keyframes [bad, good, bad, good, good]: the rows are the three good ones (far, then two 6 apart), the
    first of the two close rows wins and best_obs points into the caller's list (3).  The bad keyframe's row B would have
    won (3 from both close rows) had it counted."""
    rows = MS.interleaved_rows()
    s = _scene(rows, kf_bad=[1, 0, 1, 0, 0])
    got = _host(s)
    assert got["best_obs"][0] == 3 and got["desc"][0].tobytes() == rows[3].tobytes()
    _assert_same(got, MU.upkeep(s))
    assert _host(_scene(rows, kf_bad=[1, 0, 0, 0, 0]))["best_obs"][0] == 2


def test_all_keyframes_bad_and_no_observations():
    """every keyframe bad: the descriptor is unchanged, the normal is still computed; no observations, or a bad item:
    nothing changes"""
    rows = [BASE, _flip(BASE, [1, 2])]
    s = _scene(rows, kf_bad=[1, 1])
    got = _host(s)
    assert got["best_obs"][0] == -1 and not got["desc"].any() and got["status"][0] == 2
    _assert_same(got, MU.upkeep(s))
    for s in (_scene(np.zeros((0, 32), np.uint8)), _scene(rows, bad=1)):
        got = _host(s)
        assert got["status"][0] == 0 and got["best_obs"][0] == -1 and not got["normal"].any() and got["max_distance"][0] == 0
        assert not got["frustum"]["world"].any()
        _assert_same(got, MU.upkeep(s))


def test_bad_keyframe_still_counts_in_the_normal():
    """keyframe 1 bad: the normal equals the one with keyframe 1 good, and differs from the one without its observation"""
    rows = [BASE, _flip(BASE, [1]), _flip(BASE, [2])]
    a, b = _host(_scene(rows, kf_bad=[0, 1, 0])), _host(_scene(rows))
    assert a["status"][0] == 3 and a["normal"].tobytes() == b["normal"].tobytes()
    c = _host(_scene([rows[0], rows[2]], obs_kf=[0, 2]))
    assert a["normal"].tobytes() != c["normal"].tobytes()


@pytest.mark.parametrize("line", [False, True])
def test_zero_length_viewing_ray(line):
    """a keyframe centre at the point (the line's middle): norm 0, and the normal becomes NaN as in the reference"""
    s = MS.zero_ray_scene(line)
    got = _host(s, line)
    assert np.isnan(got["normal"]).all() and got["status"][0] == 3
    _assert_same(got, MU.upkeep(s, line=line))


@pytest.mark.parametrize("line", [False, True])
def test_every_case_holds_on_the_host(line):
    """every case of the scenario module, as the device tests run them: host == numpy and the case's own expectation"""
    for name, s, expect in MS.cases(line):
        for what in (1, 2, 3):
            got = _host(s, line, what)
            _assert_same(got, MU.upkeep(s, what=what, line=line))
            MS.holds(expect, got, what=what)


def test_bucket_items_are_what_they_claim():
    """the items built for the device's kernels win where their construction says (numpy, up to 65 rows here)"""
    for nr in MS.BUCKET_ROWS:
        for name, rows, win in MS.bucket_items(nr):
            if nr <= 65 and win is not None:
                assert MU.distinctive(np.array(rows)) == win, (nr, name)
    s = MS.with_bad_keyframes(70, 4)
    got = _host(s)
    assert s["kf_bad"][got["best_obs"][0]] == 0
    _assert_same(got, MU.upkeep(s))
    m = MS.merge([s, _scene(MS.tie_rows()), MS.zero_ray_scene(False)])
    got = _host(m)
    _assert_same(got, MU.upkeep(m))
    assert got["best_obs"][1] == 1 and np.isnan(got["normal"][2]).all()


def test_line_full_matrix_gives_the_point_answer():
    """the line form fills the full N x N matrix, the point form the triangle and its mirror: same distances, same winner"""
    rng = np.random.default_rng(9)
    for _ in range(20):
        n = int(rng.integers(1, 40))
        rows = [_flip(BASE, rng.choice(256, int(rng.integers(0, 20)), replace=False)) for _ in range(n)]
        p, l = _host(_scene(rows)), _host(_scene(rows, line=True), line=True)
        assert p["best_obs"][0] == l["best_obs"][0] == MU.distinctive(np.array(rows), full_matrix=True)


def test_bad_arguments_are_rejected():
    from dr_slam_amd import lib
    L = lib.load()
    s = _scene([BASE, BASE])
    P = lib._p
    cen, sc, off, kf, desc, world = s["kf_center"], s["scale_factors"], s["obs_offsets"], s["obs_kf"], s["obs_desc"], s["world"]
    st = np.zeros(1, np.uint8)

    def call(what=3, off=off, kf=kf, ref=np.int32([0]), lvl=np.int32([0]), nk=len(cen), status=st):
        k = lib.UpkeepKeyframes(nk, len(sc), P(cen), None, P(sc))
        it = lib.UpkeepItems(1, 0, None, P(off), P(kf), P(desc), P(world), P(ref), P(lvl))
        o = lib.UpkeepOut(None, None, None, None, None, P(status), None)
        return L.drfe_map_point_upkeep_host(what, C.byref(k), C.byref(it), C.byref(o))
    assert call() == 0
    assert call(what=0) == -1 and call(what=4) == -1
    assert call(off=np.int32([1, 2])) == -1
    assert call(kf=np.int32([0, 5])) == -1
    assert call(ref=np.int32([9])) == -1
    assert call(lvl=np.int32([8])) == -1 and call(lvl=np.int32([-1])) == -1
    assert call(what=1, lvl=np.int32([8])) == 0           # the level is not read without the normal half
    assert call(status=None) == -1


ADAPTOR_CALLER = r"""
#include "drfe_adaptor.hpp"
#include <cstdio>
#include <map>
using drfe_cv::Mat;
struct Vec6 { double v[6]; double operator()(int k) const { return v[k]; } };
struct Vec3 { double v[3] = {0, 0, 0}; double& operator()(int k) { return v[k]; } };
struct KeyFrame {
    bool bad = false; float c[3];
    Mat mDescriptors = Mat(4, 32), mLineDescriptors = Mat(4, 32);
    std::vector<drfe_cv::KeyPoint> mvKeysUn = std::vector<drfe_cv::KeyPoint>(4);
    std::vector<drfe_cv::KeyLine> mvKeyLines = std::vector<drfe_cv::KeyLine>(4);
    std::vector<float> mvScaleFactors; int mnScaleLevels = 8;
    bool isBad() const { return bad; }
    Mat GetCameraCenter() const { Mat m(3, 1, 4); std::memcpy(m.data, c, 12); return m; }
};
struct MapPoint {
    bool bad = false; float X[3]; KeyFrame* ref = nullptr; std::map<KeyFrame*, size_t> obs;
    bool isBad() const { return bad; }
    std::map<KeyFrame*, size_t> GetObservations() const { return obs; }
    KeyFrame* GetReferenceKeyFrame() const { return ref; }
    Mat GetWorldPos() const { Mat m(3, 1, 4); std::memcpy(m.data, X, 12); return m; }
};
struct MapLine {
    bool bad = false; Vec6 P; KeyFrame* ref = nullptr; std::map<KeyFrame*, size_t> obs;
    Mat mLDescriptor; Vec3 mNormalVector; float mfMaxDistance = -1, mfMinDistance = -1; std::mutex mMutexPos, mMutexFeatures;
    bool isBad() const { return bad; }
    std::map<KeyFrame*, size_t> GetObservations() const { return obs; }
    KeyFrame* GetReferenceKeyFrame() const { return ref; }
    Vec6 GetWorldPos() const { return P; }
};
static void prp(const drfe::MapPointUpkeep& r)
{
    printf("%d %d", r.status, r.best_obs);
    for (int k = 0; k < 32; k++) printf(" %d", r.descriptor[k]);
    for (int k = 0; k < 3; k++) printf(" %08x", *(const unsigned*)&r.normal[k]);
    printf(" %08x %08x\n", *(const unsigned*)&r.max_distance, *(const unsigned*)&r.min_distance);
}
int main(int, char** argv)
{
    FILE* f = fopen(argv[1], "rb");
    auto rd = [&](void* p, size_t n) { if (fread(p, 1, n, f) != n) exit(2); };
    int K; rd(&K, 4);
    std::vector<KeyFrame> kfs(K);
    std::vector<float> scale(8); rd(scale.data(), 32);
    for (KeyFrame& k : kfs) {
        int b; rd(&b, 4); k.bad = b != 0; rd(k.c, 12);
        rd(k.mDescriptors.data, 128); rd(k.mLineDescriptors.data, 128);
        for (int q = 0; q < 4; q++) { int o; rd(&o, 4); k.mvKeysUn[q].octave = o; rd(&o, 4); k.mvKeyLines[q].octave = o; }
        k.mvScaleFactors = scale;
    }
    int nobs; rd(&nobs, 4);
    std::vector<int> ok(nobs), oi(nobs);
    for (int q = 0; q < nobs; q++) { rd(&ok[q], 4); rd(&oi[q], 4); }
    int refp, refl; rd(&refp, 4); rd(&refl, 4);
    MapPoint mp; rd(mp.X, 12); mp.ref = &kfs[refp];
    MapLine ml; rd(ml.P.v, 48); ml.ref = &kfs[refl];
    for (int q = 0; q < nobs; q++) { mp.obs[&kfs[ok[q]]] = oi[q]; ml.obs[&kfs[ok[q]]] = oi[q]; }
    /* the map's iteration order is pointer order: report it */
    for (const auto& o : mp.obs) printf("%d ", (int)(o.first - kfs.data()));
    printf("\n");
    prp(drfe::UpkeepMapPoint(mp));
    const drfe::MapLineUpkeep r = drfe::UpkeepMapLine(ml);
    printf("%d %d", r.status, r.best_obs);
    for (int k = 0; k < 32; k++) printf(" %d", ml.mLDescriptor.data[k]);
    for (int k = 0; k < 3; k++) printf(" %016llx", *(const unsigned long long*)&ml.mNormalVector.v[k]);
    printf(" %08x %08x\n", *(const unsigned*)&ml.mfMaxDistance, *(const unsigned*)&ml.mfMinDistance);
    mp.bad = true;
    prp(drfe::UpkeepMapPoint(mp));
    /* the device batch form compiles against the same types (it needs a GPU to run) */
    (void)&drfe::MapUpkeep::Points<MapPoint>;
    (void)&drfe::MapUpkeep::Lines<MapLine>;
    return 0;
}
"""


@pytest.mark.parametrize("ref_observed", [True, False])
def test_adaptor_caller(tmp_path, ref_observed):
    """drfe::UpkeepMapPoint and drfe::UpkeepMapLine on stand-in KeyFrame / MapPoint / MapLine types equal numpy; with the
    ref keyframe absent from the observations the level is keypoint 0's octave (operator[] on the copy inserts 0)"""
    from dr_slam_amd import lib
    rng = np.random.default_rng(31 + ref_observed)
    K = 6
    bad = np.array([0, 1, 0, 0, 0, 0], np.int32)
    cen = rng.normal(0, 2, (K, 3)).astype(f32)
    dk = [_flip(BASE, rng.choice(256, 8, replace=False)) for _ in range(4 * K)]
    dl = [_flip(BASE, rng.choice(256, 8, replace=False)) for _ in range(4 * K)]
    oct_p = rng.integers(0, 8, (K, 4)).astype(np.int32)
    oct_l = rng.integers(0, 8, (K, 4)).astype(np.int32)
    oct_p[5], oct_l[5] = [3, 7, 7, 7], [2, 6, 6, 6]   # keyframe 5's keypoint 0 is the only one at its octave
    obs = [(0, 2), (1, 1), (2, 3), (4, 0)]
    ref = 4 if ref_observed else 5                 # keyframe 5 is not among the observations
    X = np.array([0.3, -0.2, 3.0], f32)
    P = np.array([0.1, -0.4, 2.8, 0.6, 0.2, 3.3], f64)
    blob = np.int32([K]).tobytes() + MU.scale_factors().tobytes()
    for k in range(K):
        blob += np.int32([bad[k]]).tobytes() + cen[k].tobytes() + np.concatenate(dk[4 * k:4 * k + 4]).tobytes() + \
            np.concatenate(dl[4 * k:4 * k + 4]).tobytes() + np.stack([oct_p[k], oct_l[k]], 1).astype(np.int32).tobytes()
    blob += np.int32([len(obs)]).tobytes() + np.int32(obs).tobytes() + np.int32([ref, ref]).tobytes() + X.tobytes() + P.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    exe, src = tmp_path / "caller", tmp_path / "caller.cpp"
    src.write_text(ADAPTOR_CALLER)
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-ldrfe", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe), str(tmp_path / "in.bin")], check=True, capture_output=True, text=True).stdout.split("\n")
    order = [int(v) for v in out[0].split()]                 # GetObservations()'s order (pointer order = keyframe order)
    om = dict(obs)
    obs_kf = np.int32(order)
    obs_idx = [om[k] for k in order]
    pos = {k: order.index(k) for k in order}
    lvl_idx = om.get(ref, 0)
    for line, dsc, octs, w, row in ((False, dk, oct_p, X, 1), (True, dl, oct_l, P, 2)):
        scene = dict(kf_center=cen, kf_bad=bad.astype(np.uint8), scale_factors=MU.scale_factors(), bad=np.uint8([0]),
                     obs_offsets=np.int32([0, len(obs)]), obs_kf=obs_kf,
                     obs_desc=np.array([dsc[4 * k + i] for k, i in zip(order, obs_idx)], np.uint8),
                     world=w.reshape(1, -1), ref_kf=np.int32([ref]), ref_level=np.int32([octs[ref][lvl_idx]]))
        want = MU.upkeep(scene, line=line)
        v = out[row].split()
        assert int(v[0]) == 3 and int(v[1]) == want["best_obs"][0]
        assert bytes(int(x) for x in v[2:34]) == want["desc"][0].tobytes()
        nb = want["normal"][0].view(np.uint64 if line else np.uint32)
        assert [int(x, 16) for x in v[34:37]] == [int(x) for x in nb]
        assert [int(x, 16) for x in v[37:39]] == [int(want["max_distance"].view(np.uint32)[0]), int(want["min_distance"].view(np.uint32)[0])]
        assert pos[order[want["best_obs"][0]]] == want["best_obs"][0]
    assert out[3].split()[:2] == ["0", "-1"]               # a bad point is unchanged
