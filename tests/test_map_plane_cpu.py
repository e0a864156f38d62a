"""Host tests of MapPlane::UpdateCoefficientsAndPoints: drfe_map_plane_update_host and
drfe_map_plane_rebuild_host equal the numpy restatement (tests/map_plane_numpy.py) bit for bit on random scenes and on
hand-built cases - every branch of Eigen's matrix-to-quaternion step, the w < 0 flip, the quaternion round trip against the
plain transpose, the concatenation order, chained updates, empty clouds, the voxel grid's overflow exception and the
observation order - plus a C++ caller of the adaptor's drfe::UpdateCoefficientsAndPoints."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_plane_numpy as MN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _pose(R, t=(0.3, -0.2, 1.1)):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T.astype(f32)


@pytest.mark.parametrize("seed", range(6))
def test_update_host_equals_numpy_on_random_scenes(seed):
    from dr_slam_amd import lib
    rng = np.random.default_rng(seed)
    Tcw = MN.random_pose(rng)
    frame = MN.plane_cloud(rng, int(rng.integers(50, 3000)), center=rng.normal(0, 1, 3) + [0, 0, 2], normal=rng.normal(0, 1, 3))
    world = MN.transform(MN.pose_update(Tcw), frame)
    cur = MN.voxel(np.vstack([world, world + rng.normal(0, 0.02, world.shape).astype(f32)]))
    got = lib.map_plane_update_host(Tcw, frame, cur)
    assert len(got) > 0 and _same(got, MN.update(Tcw, frame, cur))


@pytest.mark.parametrize("seed", range(4))
def test_rebuild_host_equals_numpy_on_random_scenes(seed):
    from dr_slam_amd import lib
    rng = np.random.default_rng(100 + seed)
    k = int(rng.integers(1, 6))
    Twcs = [MN.random_pose(rng) for _ in range(k)]
    clouds = [MN.plane_cloud(rng, int(rng.integers(0, 2000)), normal=rng.normal(0, 1, 3)) for _ in range(k)]
    got = lib.map_plane_rebuild_host(Twcs, clouds)
    assert _same(got, MN.rebuild(Twcs, clouds))


# crafted rotations: (matrix, Eigen branch, w < 0 flip)
_CASES = [
    (MN.rotation([0.3, -0.5, 0.8], 0.7), "trace", False),
    (MN.rotation([1, 0.05, -0.02], np.deg2rad(170)), "i=0", False),
    (MN.rotation([0.02, 1, 0.05], np.deg2rad(175)), "i=1", False),
    (MN.rotation([-0.03, 0.02, 1], np.deg2rad(178)), "i=2", False),
    (MN.rotation([1, 0.05, -0.02], np.deg2rad(-170)), "i=0", True),
    (MN.rotation([0.05, 0.02, 1], np.deg2rad(-172)), "i=2", True),
]


@pytest.mark.parametrize("case", range(len(_CASES)))
def test_quaternion_branches(case):
    """each branch of quaternion_assign_impl<3, 3> and the w < 0 flip, on the float pose: the host entry equals numpy"""
    from dr_slam_amd import lib
    R, branch, flip = _CASES[case]
    Tcw = _pose(R)
    _, b, fl = MN.se3quat_rotation(Tcw[:3, :3].astype(f64))
    assert (b, fl) == (branch, flip)
    rng = np.random.default_rng(case)
    frame = (rng.uniform(-1, 1, (400, 3)) * [1, 1, 0.01] + [0, 0, 2]).astype(f32)
    got = lib.map_plane_update_host(Tcw, frame, np.zeros((0, 3), f32))
    assert _same(got, MN.update(Tcw, frame, np.zeros((0, 3), f32)))


def test_round_trip_is_not_the_plain_transpose():
    """the quaternion round trip renormalises the float rotation: its bits differ from R^T, and so do the moved points"""
    from dr_slam_amd import lib
    Tcw = _pose(MN.rotation([0.3, -0.5, 0.8], 0.7))
    T = MN.pose_update(Tcw)
    Rt = Tcw[:3, :3].astype(f64).T
    assert not np.array_equal(T[:3, :3], Rt)
    direct = np.eye(4)
    direct[:3, :3] = Rt
    t = Tcw[:3, 3].astype(f64)
    for r in range(3):
        direct[r, 3] = -((Rt[r, 0] * t[0] + Rt[r, 1] * t[1]) + Rt[r, 2] * t[2])
    g = np.arange(-10, 10, dtype=f64) * 0.11            # one point per leaf: the voxel grid returns the points themselves
    frame = np.stack(np.meshgrid(g, g, [2.0]), -1).reshape(-1, 3).astype(f32)
    got = lib.map_plane_update_host(Tcw, frame, np.zeros((0, 3), f32))
    assert _same(got, MN.voxel(MN.transform(T, frame)))
    assert not _same(got, MN.voxel(MN.transform(direct, frame)))


def test_concatenation_order_decides_the_centroids():
    """frame and map points share leaves: the frame's points come first, and the other order gives other bits"""
    from dr_slam_amd import lib
    rng = np.random.default_rng(5)
    Tcw = MN.random_pose(rng)
    frame = MN.plane_cloud(rng, 4000, extent=0.12, noise=0.001)
    world = MN.transform(MN.pose_update(Tcw), frame)
    cur = (world[::2] + rng.normal(0, 0.01, world[::2].shape)).astype(f32)
    got = lib.map_plane_update_host(Tcw, frame, cur)
    assert _same(got, MN.update(Tcw, frame, cur))
    assert len(got) < len(frame) // 10
    other = MN.voxel(np.vstack([cur, world]))
    assert got.shape == other.shape and not _same(got, other)


def test_two_updates_chain():
    from dr_slam_amd import lib
    rng = np.random.default_rng(9)
    T1, T2 = MN.random_pose(rng), MN.random_pose(rng)
    f1, f2 = MN.plane_cloud(rng, 1500, extent=0.4), MN.plane_cloud(rng, 1500, extent=0.4)
    m0 = MN.transform(MN.pose_update(T1), MN.plane_cloud(rng, 800, extent=0.4))
    c1 = lib.map_plane_update_host(T1, f1, m0)
    c2 = lib.map_plane_update_host(T2, f2, c1)
    assert _same(c2, MN.update(T2, f2, MN.update(T1, f1, m0)))
    assert not _same(c2, MN.update(T2, f2, m0))


def test_empty_clouds():
    from dr_slam_amd import lib
    rng = np.random.default_rng(3)
    Tcw = MN.random_pose(rng)
    frame = MN.plane_cloud(rng, 300)
    e = np.zeros((0, 3), f32)
    assert _same(lib.map_plane_update_host(Tcw, frame, e), MN.update(Tcw, frame, e))
    cur = MN.plane_cloud(rng, 300)
    assert _same(lib.map_plane_update_host(Tcw, e, cur), MN.voxel(cur))
    assert lib.map_plane_update_host(Tcw, e, e).shape == (0, 3)
    assert lib.map_plane_rebuild_host([], []).shape == (0, 3)
    assert lib.map_plane_rebuild_host([Tcw], [e]).shape == (0, 3)


def test_overflow_returns_the_concatenated_input():
    """a grid past 2^31 leaves: PCL's "leaf size too small" path returns the input cloud, frame points first"""
    from dr_slam_amd import lib
    rng = np.random.default_rng(4)
    Tcw = MN.random_pose(rng)
    frame = rng.uniform(-800, 800, (50, 3)).astype(f32)
    cur = rng.uniform(-800, 800, (30, 3)).astype(f32)
    got = lib.map_plane_update_host(Tcw, frame, cur)
    want = np.vstack([MN.transform(MN.pose_update(Tcw), frame), cur])
    assert _same(got, want) and _same(got, MN.update(Tcw, frame, cur))
    Twcs = [MN.random_pose(rng), MN.random_pose(rng)]
    got = lib.map_plane_rebuild_host(Twcs, [frame, cur])
    assert _same(got, np.vstack([MN.transform(MN.pose_rebuild(Twcs[0]), frame), MN.transform(MN.pose_rebuild(Twcs[1]), cur)]))


def test_observation_order_changes_the_bits():
    from dr_slam_amd import lib
    rng = np.random.default_rng(12)
    Twcs = [MN.random_pose(rng, 0.05) for _ in range(3)]
    base = MN.plane_cloud(rng, 3000, extent=0.15, noise=0.001)
    clouds = [MN.transform(np.linalg.inv(MN.pose_rebuild(T)), base[k::3]) for k, T in enumerate(Twcs)]
    a = lib.map_plane_rebuild_host(Twcs, clouds)
    b = lib.map_plane_rebuild_host(Twcs[::-1], clouds[::-1])
    assert _same(a, MN.rebuild(Twcs, clouds)) and _same(b, MN.rebuild(Twcs[::-1], clouds[::-1]))
    assert a.shape == b.shape and not _same(a, b)


def test_bad_arguments_are_rejected():
    import ctypes as C
    from dr_slam_amd import lib
    L = lib.load()
    T = np.eye(4, dtype=f32)
    p = np.zeros((4, 3), f32)
    n = C.c_int()
    P = lib._p
    assert L.drfe_map_plane_update_host(None, P(p), 4, P(p), 0, P(p), 4, C.byref(n)) != 0
    assert L.drfe_map_plane_update_host(P(T), None, 4, P(p), 0, P(p), 4, C.byref(n)) != 0
    assert L.drfe_map_plane_update_host(P(T), P(p), -1, P(p), 0, P(p), 4, C.byref(n)) != 0
    assert L.drfe_map_plane_update_host(P(T), P(p), 4, P(p), 0, P(p), 0, C.byref(n)) == -3     # capacity
    off = np.array([0, 4], np.int32)
    assert L.drfe_map_plane_rebuild_host(1, None, P(off), P(p), P(p), 4, C.byref(n)) != 0
    bad = np.array([3, 1], np.int32)
    assert L.drfe_map_plane_rebuild_host(1, P(T), P(bad), P(p), P(p), 4, C.byref(n)) != 0


ADAPTOR_CALLER = r"""
#include "drfe_adaptor.hpp"
#include <cstdio>
#include <map>
struct Pt { float x, y, z, rgb; };
struct Cloud { std::vector<Pt> points; unsigned width = 0, height = 0; bool is_dense = false; };
drfe_cv::Mat fmat(int r, int c, const float* v) { drfe_cv::Mat m(r, c, 4); m.step = (size_t)c * 4; std::memcpy(m.data, v, (size_t)r * c * 4); return m; }
struct KeyFrame { drfe_cv::Mat Twc; std::vector<Cloud> mvPlanePoints; drfe_cv::Mat GetPoseInverse() const { return Twc; } };
struct Frame { drfe_cv::Mat mTcw; std::vector<Cloud> mvPlanePoints; };
struct MapPlane {
    std::shared_ptr<Cloud> mvPlanePoints = std::make_shared<Cloud>();
    std::vector<std::pair<KeyFrame*, size_t>> obs;
    std::vector<std::pair<KeyFrame*, size_t>> GetObservations() const { return obs; }
};
struct RawPlane { Cloud* mvPlanePoints = nullptr; };
static float rdf(FILE* f) { float v; if (fread(&v, 4, 1, f) != 1) exit(2); return v; }
static int rdi(FILE* f) { int v; if (fread(&v, 4, 1, f) != 1) exit(2); return v; }
static Cloud rdc(FILE* f) { Cloud c; const int n = rdi(f); for (int k = 0; k < n; k++) { Pt p; p.x = rdf(f); p.y = rdf(f); p.z = rdf(f); p.rgb = 7; c.points.push_back(p); } return c; }
static void pr(const Cloud& c) { printf("%zu %u %u %d", c.points.size(), c.width, c.height, c.is_dense ? 1 : 0); for (const Pt& p : c.points) printf(" %08x %08x %08x", *(const unsigned*)&p.x, *(const unsigned*)&p.y, *(const unsigned*)&p.z); printf("\n"); }
int main(int, char** argv)
{
    FILE* f = fopen(argv[1], "rb");
    float T[16];
    Frame F;
    for (float& t : T) t = rdf(f);
    F.mTcw = fmat(4, 4, T);
    F.mvPlanePoints.push_back(Cloud());
    F.mvPlanePoints.push_back(rdc(f));
    MapPlane mp;
    *mp.mvPlanePoints = rdc(f);
    std::shared_ptr<Cloud> old = mp.mvPlanePoints;
    drfe::UpdateCoefficientsAndPoints(mp, F, 1);
    pr(*mp.mvPlanePoints);
    printf("%d\n", old.get() != mp.mvPlanePoints.get() && !old->points.empty() ? 1 : 0);
    const int K = rdi(f);
    std::vector<KeyFrame> kfs(K);
    for (int k = 0; k < K; k++) {
        for (float& t : T) t = rdf(f);
        kfs[k].Twc = fmat(4, 4, T);
        kfs[k].mvPlanePoints.push_back(Cloud());
        kfs[k].mvPlanePoints.push_back(rdc(f));
        mp.obs.push_back({&kfs[k], 1});
    }
    drfe::UpdateCoefficientsAndPoints(mp);
    pr(*mp.mvPlanePoints);
    Cloud raw;
    RawPlane rp; rp.mvPlanePoints = &raw;
    drfe::UpdateCoefficientsAndPoints(rp, F, 1);
    printf("%zu\n", raw.points.size());
    return 0;
}
"""


def test_adaptor_updates_the_plane_cloud(tmp_path):
    """A C++ caller of drfe::UpdateCoefficientsAndPoints (include/drfe_adaptor.hpp), both forms, on stand-in Frame / KeyFrame /
    MapPlane types: the new cloud equals numpy bit for bit, a shared_ptr cloud is reseated (the old one survives), the PCL shape
    fields are set, and a raw-pointer cloud is overwritten in place."""
    from dr_slam_amd import lib
    rng = np.random.default_rng(21)
    Tcw = MN.random_pose(rng)
    frame = MN.plane_cloud(rng, 700, extent=0.5)
    cur = MN.transform(MN.pose_update(Tcw), MN.plane_cloud(rng, 500, extent=0.5))
    Twcs = [MN.random_pose(rng) for _ in range(3)]
    kc = [MN.plane_cloud(rng, 400, extent=0.5) for _ in range(3)]

    def cl(c):
        return np.int32([len(c)]).tobytes() + np.ascontiguousarray(c, f32).tobytes()
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        f.write(Tcw.tobytes() + cl(frame) + cl(cur) + np.int32([3]).tobytes())
        for T, c in zip(Twcs, kc):
            f.write(np.ascontiguousarray(T, f32).tobytes() + cl(c))
    exe, src = tmp_path / "caller", tmp_path / "caller.cpp"
    src.write_text(ADAPTOR_CALLER)
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-ldrfe", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe), str(blob)], check=True, capture_output=True, text=True).stdout.split("\n")

    def parse(line):
        v = line.split()
        n = int(v[0])
        xyz = np.array([int(h, 16) for h in v[4:]], np.uint32).view(f32).reshape(n, 3)
        return xyz, tuple(int(x) for x in v[1:4])
    got, shape = parse(out[0])
    want = MN.update(Tcw, frame, cur)
    assert _same(got, want) and shape == (len(want), 1, 1)
    assert out[1] == "1"
    got, shape = parse(out[2])
    want = MN.rebuild(Twcs, kc)
    assert _same(got, want) and shape == (len(want), 1, 1)
    assert int(out[3]) == len(MN.update(Tcw, frame, np.zeros((0, 3), f32)))
