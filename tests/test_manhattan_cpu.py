"""CPU tests of the Manhattan-frame tracker: the host entry drfe_manhattan_track_host equals an independent
numpy restatement of the reference (tests/manhattan_numpy.py) bit for bit on synthetic scenes and on hand-built records that
reach every branch; the canonical asin / exp / tanf of include/drfe_math.h stay within 1 ulp of the host libm; the tracked
rotation follows the true camera rotation of a synthetic sequence."""
import collections
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manhattan_numpy as MN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(normals):
    from dr_slam_amd import lib
    n = np.asarray(normals, np.float32).reshape(-1, 3)
    r = np.zeros(len(n), lib.SURFACE_NORMAL_DTYPE)
    r["normal"] = n
    r["camera_position"] = np.arange(3 * len(n), dtype=np.float32).reshape(-1, 3)
    r["frame_x"] = np.arange(len(n)) * 3
    r["frame_y"] = np.arange(len(n)) % 7
    return r


def _scene_records(oracle_mod, kind, seed, k=0, cam=None):
    from dr_slam_amd import synth
    O = oracle_mod
    cam = cam or synth.TUM3
    _, d, T = next(synth.sequence(seed, 1, cam=cam, kind=kind, start=k))
    inv = np.float32(1.0) / np.float32(cam.depth_factor)
    cloud, nrm = O.post_surface_normals(O.depth_to_float(d, inv), np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float32), 9.0)
    on, oc, fx, fy = O.post_surface_normal_records(cloud, nrm)
    r = _records(on)
    r["camera_position"], r["frame_x"], r["frame_y"] = oc, fx, fy
    return r, np.linalg.inv(T)[:3, :3].astype(np.float32)


def _check(R, recs, dirs=None, n_calls=3, hits=None):
    from dr_slam_amd import lib
    Rc, ic, rbc, lbc = lib.manhattan_track_host(R, recs, dirs, n_calls)
    Rn, infos, rb, lb, hits = MN.track(R, recs["normal"], dirs, n_calls, hits)
    MN.assert_equal_to_product(Rn, infos, rb, lb, Rc, ic, rbc, lbc)
    return Rc, ic, rbc, lbc, hits


def _rot(ax, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][ax]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _around(axes, n, rng, noise=0.05, R=np.eye(3)):
    """n normals around each Manhattan axis in `axes` (columns of R), both signs, Gaussian tilt"""
    out = []
    for a in axes:
        v = R[:, a][None, :] * np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0) + rng.normal(0, noise, (n, 3))
        out.append(v / np.linalg.norm(v, axis=1, keepdims=True))
    return np.concatenate(out).astype(np.float32)


@pytest.mark.parametrize("kind,seed", [("room_boxes", 2), ("corridor", 4), ("living_room", 3)])
def test_host_entry_equals_numpy_restatement_on_scenes(oracle_mod, kind, seed):
    hits = collections.Counter()
    for k, tilt in ((0, 0.0), (5, 4.0)):
        recs, Rcw = _scene_records(oracle_mod, kind, seed, k)
        R0 = (Rcw.astype(np.float64) @ _rot(0, tilt)).astype(np.float32)
        _, info, rb, _, hits = _check(R0, recs, hits=hits)
        assert info["call"][0]["in_cone"].sum() > 500
        assert (rb & 0x1FF).any() and (rb & MN.INLINE).any()
    assert hits["nan_records"] > 0                         # PCL leaves NaN normals at borders and discontinuities


def test_host_entry_equals_numpy_restatement_hand_built():
    from dr_slam_amd import lib
    rng = np.random.default_rng(7)
    hits = collections.Counter()
    R1 = (_rot(1, 3.0) @ _rot(0, -2.0)).astype(np.float32)
    # no axis: every normal far from every cone -> the input comes back unchanged, no SVD
    far = np.tile(np.float32([1, 1, 1]) / np.float32(math.sqrt(3)), (400, 1)) + rng.normal(0, 0.01, (400, 3)).astype(np.float32)
    Rc, info, _, _, hits = _check(R1, _records(far), hits=hits)
    assert np.array_equal(Rc.view(np.uint32), R1.view(np.uint32)) and info["call"]["svd"][:3].sum() == 0
    # one axis: the reference still replaces that column (R_cm and R_cm_update share one buffer) and skips the SVD
    Rc, info, _, _, hits = _check(R1, _records(_around([2], 600, rng, R=R1)), hits=hits)
    assert info["call"][0]["found"] == 4 and info["call"][0]["svd"] == 0 and info["call"][0]["deficient"] == 1
    assert np.array_equal(Rc[:, :2].view(np.uint32), R1[:, :2].view(np.uint32))
    assert not np.array_equal(Rc[:, 2].view(np.uint32), R1[:, 2].view(np.uint32))
    # exactly two axes, every pair
    for pair, mask in (((0, 1), 3), ((1, 2), 6), ((0, 2), 5)):
        _, info, _, _, hits = _check(R1, _records(_around(pair, 700, rng, R=R1)), hits=hits)
        assert info["call"][0]["found"] == mask and info["call"][0]["svd"] == 1
    # an exactly axis-aligned normal under R = I (lambda == 0: 0 / 0, pushed but dropped) and NaN records.  Axis x: the
    # first of the mean-shift pass, which still sees the input R (later axes see the columns already replaced)
    nrm = np.concatenate([_around([0, 1, 2], 300, rng), [[1, 0, 0], [-1, 0, 0], [np.nan] * 3, [np.nan, 0, 1]]]).astype(np.float32)
    _, info, rb, _, hits = _check(np.eye(3, dtype=np.float32), _records(nrm), n_calls=1, hits=hits)
    assert rb[-4] & 1 and rb[-3] & 1                        # pushed to the x list ...
    assert info["call"][0]["n_selected"][0] == int((rb & 1).sum()) - 2   # ... but not selected
    assert rb[-2] == 0 and rb[-1] == 0                      # NaN: never in a cone
    # line directions: 0.05 rad off an axis is inside the line cone (0.1018), 0.15 rad is not (but would be for a normal)
    dirs = np.array([[math.sin(0.05), 0, math.cos(0.05)], [0, math.cos(0.05), math.sin(0.05)], [math.sin(0.15), 0, math.cos(0.15)],
                     [math.cos(0.15), math.sin(0.15), 0], [0.6, 0.0, 0.8]])
    _, _, _, lb, hits = _check(R1 @ np.eye(3, dtype=np.float32), _records(_around([0, 1, 2], 200, rng, R=R1)), dirs, hits=hits)
    _, _, _, lb, hits = _check(np.eye(3, dtype=np.float32), _records(_around([0, 1, 2], 200, rng)), dirs, hits=hits)
    assert list(lb & MN.INLINE != 0) == [True, True, False, False, False]
    assert (lb[:2] & 0x1FF).all() and not (lb[2:] & 0x1FF).any()
    for case in ("found_0", "found_1", "pair_3", "pair_6", "pair_5", "det_flip", "deficiency", "zero_lambda_dropped",
                 "nan_records", "lines_in_cone", "lines_outside_cone", "found_3"):
        assert hits[case] > 0, case
    with pytest.raises(lib.DrfeError):
        lib.manhattan_track_host(np.eye(3), _records(far), n_calls=6)


def _ulp_diff(a, b, dtype):
    it = np.int64 if dtype == np.float64 else np.int32
    return np.abs(np.asarray(a, dtype).view(it).astype(np.int64) - np.asarray(b, dtype).view(it).astype(np.int64))


def test_canonical_libm_within_one_ulp():
    from dr_slam_amd import lib
    rng = np.random.default_rng(3)
    x = np.concatenate([[0.0, 1e-300, 1e-9], rng.uniform(0, MN.SIN_MS, 150000)])
    a = lib.manhattan_math(0, x)
    assert _ulp_diff(a, [math.asin(v) for v in x], np.float64).max() <= 1
    assert np.array_equal(a.view(np.int64), MN.asin(x).view(np.int64))
    x = np.concatenate([[0.0, -2.0, -1e-12], rng.uniform(-2, 0, 150000)])
    e = lib.manhattan_math(1, x)
    assert _ulp_diff(e, [math.exp(v) for v in x], np.float64).max() <= 1
    assert np.array_equal(e.view(np.int64), MN.exp(x).view(np.int64))
    xf = np.concatenate([[0.0, 0.26], rng.uniform(0, 0.26, 150000)]).astype(np.float32)
    t = lib.manhattan_math(2, xf.astype(np.float64)).astype(np.float32)
    assert _ulp_diff(t, np.tan(xf), np.float32).max() <= 1
    assert np.array_equal(t.view(np.int32), MN.tanf(xf).view(np.int32))
    for c, h in ((0.2018, "0x1.9a7caf08cdfccp-3"), (0.1018, "0x1.a040c2f653a3cp-4"), (0.2518, "0x1.fe4118cace77ep-3")):
        assert float.fromhex(h) == math.sin(c)
    txt = open(os.path.join(ROOT, "include", "drfe_math.h")).read()
    for h in ("0x1.9a7caf08cdfccp-3", "0x1.a040c2f653a3cp-4", "0x1.fe4118cace77ep-3"):
        assert h in txt
    assert MN.SIN_NORMAL == math.sin(0.2018) and MN.SIN_LINE == math.sin(0.1018) and MN.SIN_MS == math.sin(0.2518)


def test_tracking_follows_the_true_rotation(oracle_mod):
    """room_boxes, 60 frames (the camera yaws 0.2 deg per frame): R_cm stays within 1 deg of R_cw up to axis order / sign"""
    from dr_slam_amd import lib
    R = None
    worst = 0.0
    for k in range(60):
        recs, Rcw = _scene_records(oracle_mod, "room_boxes", 2, k)
        R = Rcw if R is None else R
        R, info, _, _ = lib.manhattan_track_host(R, recs)
        P = Rcw.astype(np.float64).T @ R.astype(np.float64)     # a signed permutation when R_cm matches
        S = np.round(P)
        assert np.allclose(np.abs(S).sum(0), 1) and np.allclose(np.abs(S).sum(1), 1)
        Q = P @ S.T
        worst = max(worst, math.degrees(math.acos(min(1.0, (np.trace(Q) - 1) / 2))))
    assert worst < 1.0, worst


ADAPTOR_CALLER = r"""
#include <cstdio>
#include <vector>
#include "drfe_adaptor.hpp"
int main(int argc, char** argv)
{
    FILE* f = std::fopen(argv[1], "rb");
    int n = 0, nl = 0;
    float R[9];
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(&nl, 4, 1, f) != 1 || std::fread(R, 4, 9, f) != 9) return 2;
    std::vector<drfe::SurfaceNormal> sn(n);
    for (int i = 0; i < n; i++) {
        drfe_surface_normal r;
        if (std::fread(&r, sizeof(r), 1, f) != 1) return 2;
        sn[i].normal = drfe::Point3f{r.normal[0], r.normal[1], r.normal[2]};
        sn[i].cameraPosition = drfe::Point3f{r.camera_position[0], r.camera_position[1], r.camera_position[2]};
        sn[i].FramePosition = drfe::Point2i{r.frame_x, r.frame_y};
    }
    std::vector<drfe::FrameLine> lines(nl);
    for (int l = 0; l < nl; l++) {
        double d[3];
        if (std::fread(d, 8, 3, f) != 3) return 2;
        lines[l].direction = drfe::Point3d{d[0], d[1], d[2]};
    }
    std::fclose(f);
    drfe::Mat33f Rm;
    for (int i = 0; i < 9; i++) Rm.v[i] = R[i];
    drfe::ManhattanFrameOut out;
    std::vector<bool> inl;
    for (int k = 0; k < 3; k++) Rm = drfe::TrackManhattanFrame(Rm, sn, lines, out, inl);
    drfe::Mat33f R3 = drfe::rotation_make(R);
    for (int k = 0; k < 3; k++) R3 = drfe::TrackManhattanFrame(R3, sn, lines);
    for (int i = 0; i < 9; i++)
        if (R3.v[i] != Rm.v[i]) return 3;
    for (int i = 0; i < 9; i++) std::printf("%08x\n", *reinterpret_cast<unsigned*>(&Rm.v[i]));
    const std::vector<drfe::Point2i>* L[3] = {&out.vSurfaceNormalx, &out.vSurfaceNormaly, &out.vSurfaceNormalz};
    for (int a = 0; a < 3; a++) {
        std::printf("list %d %zu\n", a, L[a]->size());
        for (const auto& p : *L[a]) std::printf("%d %d\n", p.x, p.y);
    }
    size_t nin = 0;
    for (bool b : inl) nin += b;
    std::printf("inline %zu %zu\n", inl.size(), nin);
    std::printf("lines %zu %zu\n", out.vVanishingLinex.size() + out.vVanishingLiney.size() + out.vVanishingLinez.size(),
                out.vVanishingLinex.empty() ? 0 : out.vVanishingLinex[0].size());
    return 0;
}
"""


def test_adaptor_reproduces_surface_normal_lists(oracle_mod, tmp_path):
    """A C++ caller of drfe::TrackManhattanFrame (include/drfe_adaptor.hpp) over the host entry: three chained calls fill
    vSurfaceNormalx/y/z call-major, then in record order, as ProjectSN2MF pushes them."""
    from dr_slam_amd import lib
    recs, Rcw = _scene_records(oracle_mod, "living_room", 3, 2)
    dirs = np.array([[0.05, 0.0, 1.0], [0.3, 0.3, 0.9]])
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        f.write(np.int32([len(recs), len(dirs)]).tobytes() + Rcw.tobytes() + recs.tobytes() + dirs.tobytes())
    exe = tmp_path / "caller"
    src = tmp_path / "caller.cpp"
    src.write_text(ADAPTOR_CALLER)
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-ldrfe", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe), str(blob)], check=True, capture_output=True, text=True).stdout.split("\n")
    Rc, info, rb, lb = lib.manhattan_track_host(Rcw, recs, dirs, 3)
    assert [int(v, 16) for v in out[:9]] == list(Rc.reshape(-1).view(np.uint32))
    pos = 9
    for a in range(3):
        head = out[pos].split()
        cnt = int(head[2])
        got = [tuple(map(int, ln.split())) for ln in out[pos + 1:pos + 1 + cnt]]
        want = [(int(recs["frame_x"][i]), int(recs["frame_y"][i])) for k in range(3)
                for i in np.flatnonzero(rb & (1 << (3 * k + a)))]
        assert got == want and cnt > 0
        pos += 1 + cnt
    assert out[pos].split() == ["inline", str(len(recs)), str(int(((rb & MN.INLINE) != 0).sum()))]
    n_pairs = sum(bin(int(b) & 0x1FF).count("1") for b in lb)
    assert out[pos + 1].split()[1] == str(n_pairs)
