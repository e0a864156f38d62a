"""No-GPU tests around Frame::isLineGood's batch entry: the hand-built scene of line3d_scenarios.py is
deterministic and has the properties the GPU tests rely on; on it the host entry drfe_lines_is_good - the truth of the GPU tests -
agrees with the numpy oracle and, with its arithmetic moved into line3d_core.h, still writes the bytes recorded before the move
(tests/golden/line3d_host.npz); the new symbols are exported as include/drfe.h declares them."""
import ctypes as C
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line3d_scenarios as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (sc.K9, sc.CX, sc.CY, sc.INVFX, sc.INVFY)


def _host(seed, lines=None, **kw):
    from dr_slam_amd import lib
    kl = sc.key_lines(lib.KEYLINE_DTYPE) if lines is None else lines
    return lib.lines_is_good(kl, sc.depth_image(), *CAM, k_as_f64=True, seed=seed, **kw)


def test_scene_is_deterministic_and_as_described():
    from dr_slam_amd import lib
    a, b = sc.depth_image(), sc.depth_image()
    assert a.dtype == np.float32 and a.shape == (sc.H, sc.W) and a.tobytes() == b.tobytes()
    assert (a[95:111, 30:36] == 0).all() and (np.delete(a, np.s_[95:111], 0) > 1.9).all()
    assert ((np.round(a.astype(np.float64) * 5000) / 5000).astype(np.float32) == a).all()              # 1/5000 m steps
    assert 3.9 < np.median(a[:, 100:]) < 4.1 and 2.0 < np.median(a[:, :100]) < 2.2                  # the step
    clean = np.where(np.arange(sc.W) < 100, 2 + 0.002 * np.arange(sc.W), 4.0)[None, :]
    far = (a - clean > 0.15) & (a > 0)
    assert 0.10 < far.mean() < 0.20                                                                # the outliers
    kl = sc.key_lines(lib.KEYLINE_DTYPE)
    assert len(kl) == 12 and kl.tobytes() == sc.key_lines(lib.KEYLINE_DTYPE).tobytes()
    assert kl[0].tobytes()[8:] == kl[11].tobytes()[8:]                                             # one line twice (class_id apart)
    forty = sc.key_lines(lib.KEYLINE_DTYPE, count=40)
    assert forty["start_point_x"][12] == kl["start_point_x"][0] and forty["end_point_y"][39] == kl["end_point_y"][3]


def test_scene_shows_the_rand_chain():
    """n_good = 3 at every seed, eight seeds give eight outputs, the twice-listed line gets two results in one frame, and taking
    line 1 out changes the lines behind it"""
    from dr_slam_amd import lib
    res = {s: _host(s) for s in range(1, 9)}
    assert all(r[3] == 3 for r in res.values())
    assert len({r[0].tobytes() + r[1].tobytes() + r[2].tobytes() for r in res.values()}) == 8
    assert res[1][2][0] != res[1][2][11]
    assert (res[1][2][[3, 5]] == 0).all()                     # 9 samples, and a sub-pixel line: no RANSAC
    kl = sc.key_lines(lib.KEYLINE_DTYPE)
    without = _host(1, np.delete(kl, 1))
    assert without[1][1:].tobytes() != res[1][1][2:].tobytes()


def test_host_entry_matches_numpy_oracle_on_the_scene():
    """as tests/test_host_cpu.py compares them: inlier counts and depth exact, end points up to the A/B swap"""
    from dr_slam_amd import lib
    from oracle import line3d_oracle as L3
    kl, depth = sc.key_lines(lib.KEYLINE_DTYPE), sc.depth_image()
    for seed in (1, 8):
        dl, l3, ni, good = _host(seed)
        odl, ol3, oni = L3.is_line_good(kl, depth, sc.K9, True, sc.CX, sc.CY, sc.INVFX, sc.INVFY, seed=seed)
        assert np.array_equal(ni, oni), (ni, oni)
        assert np.array_equal(dl.view(np.uint32), odl.view(np.uint32))
        for a, b in zip(l3, ol3):
            assert np.allclose(a, b, atol=1e-9) or np.allclose(a, np.concatenate([b[3:], b[:3]]), atol=1e-9)
        assert good == int((dl >= 0).sum()) == 3


def test_host_entry_writes_the_bytes_recorded_before_line3d_core():
    g = np.load(os.path.join(ROOT, "tests", "golden", "line3d_host.npz"))
    for k, seed in enumerate((1, 8)):
        dl, l3, ni, good = _host(seed)
        assert dl.tobytes() == g[f"depth_line_{seed}"].tobytes()
        assert l3.tobytes() == g[f"lines3d_{seed}"].tobytes()
        assert ni.tobytes() == g[f"n_inliers_{seed}"].tobytes()
        assert good == g["n_good"][k]


def test_new_symbols_are_exported_as_declared():
    from dr_slam_amd import lib
    L = lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drfe.h")).read(), flags=re.S)
    header = " ".join(header.split())
    for decl in ("int drfe_lines_is_good_batch(drfe_ctx* ctx, const drfe_line3d_frames* in, drfe_line3d_out* out, void* stream);",
                 "int drfe_line3d_stats(drfe_ctx* ctx, int64_t* stats );",
                 "int drfe_line3d_chunk_frames(int cap);"):
        assert decl in header, decl
    for name, nargs in (("drfe_lines_is_good_batch", 4), ("drfe_line3d_stats", 2), ("drfe_line3d_chunk_frames", 1)):
        assert name in lib.SYMBOLS and len(getattr(L, name).argtypes) == nargs
    # the structs as the header lays them out on LP64: 2 int32, 3 pointers, 2 size_t, 4 int32, 13 floats, (pad), 1 pointer
    assert C.sizeof(lib.Line3dFrames) == 8 + 24 + 16 + 16 + 52 + 4 + 8 and lib.Line3dFrames.seeds.offset == 120
    assert lib.Line3dFrames.K.offset == 64 and lib.Line3dFrames.cx.offset == 100 and C.sizeof(lib.Line3dOut) == 32
    m = re.search(r"typedef struct drfe_line3d_frames \{(.*?)\} drfe_line3d_frames;", header)
    fields = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", m.group(1))
    assert fields == [f[0] for f in lib.Line3dFrames._fields_], fields
    # what needs no device: the chunk size, and the refusal of a call without a context
    assert lib.line3d_chunk_frames(40) >= 64 and lib.line3d_chunk_frames(40) * 40 == lib.line3d_chunk_frames(1)
    assert lib.line3d_chunk_frames(10 ** 6) == 1
    fr, out, _, _keep = lib.line3d_frames(sc.key_lines(lib.KEYLINE_DTYPE)[None], [12], sc.depth_image()[None], *CAM)
    assert fr.nframes == 1 and fr.cap == 12 and fr.w == sc.W and fr.h == sc.H and fr.stride == sc.W and fr.depth_on_device == 0
    assert L.drfe_lines_is_good_batch(None, C.byref(fr), C.byref(out), None) == -1
    assert L.drfe_line3d_stats(None, None) == -1
