"""Bounds of the in-place level 0 (dr_slam_amd/csrc/level0_view.h), on the host.

An out-of-range read of the caller's image cannot be shown on a device, so tests/native/level0_view.cpp replays every block and
thread of level 0's four readers - the blur's level-0 tiles, the FAST fills of level-0 cells, level 1's resize windows, the
descriptor's raw patches along the rim of where a keypoint can lie - through the address helpers the kernels call, and counts
the loads with a byte outside [frame, frame + (h - 1) * row_stride + w).

Geometries: 640x480 with row strides 640 and 704, 1280x960, 208x112 in rows of 256 bytes, 256x128, 48x48.
  - 256x128 runs two levels: with a third one the context refuses the geometry (the level's single FAST cell row is taller than
    the 60-px window limit).
  - 208x112 (three levels) is not eligible - its level-0 FAST cells need 14 rows per lane, k_fast_cells_cols holds 12 - but its
    width gives level 1 a window plan, so its loads are replayed all the same; 208x122 on two levels is its eligible neighbour.
  - 48x48 is smaller than one FAST cell: the context refuses it, nothing is read in place.
Eligibility is a pure function of geometry, pointer and strides: 641x479 and 333x250 are refused (width), 640x480 is refused 4 bytes
off a 16-byte boundary or in rows of 644 bytes.  752x480 meets every condition (752 = 47 x 16, every cell in k_fast_cells_cols,
level 1 on the tiled resize) and replays clean, so it is read in place.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def view_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("level0_view") / "level0_view")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-DDRFE_NO_ROCTX",
                    "-I/opt/rocm/include", os.path.join(ROOT, "tests", "native", "level0_view.cpp"),
                    os.path.join(ROOT, "dr_slam_amd", "csrc", "orb_geometry.cpp"), "-o", exe], check=True)
    return exe


def _view(exe, *args):
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    f = p.stdout.split()
    if p.returncode != 0:
        return dict(error=p.stdout.strip())
    assert f[0::2] == ["eligible", "loads", "outside", "padding", "plan", "reflect"], p.stdout
    return dict(zip(f[0::2], (int(v) for v in f[1::2])))


@pytest.mark.parametrize("w,h,stride,nlevels,eligible", [
    (640, 480, 640, 8, 1), (640, 480, 704, 8, 1), (1280, 960, 1280, 8, 1), (208, 112, 256, 3, 0), (208, 122, 256, 2, 1),
    (256, 128, 256, 2, 1), (752, 480, 752, 8, 1)])
def test_every_level0_load_lies_inside_the_frame(view_exe, w, h, stride, nlevels, eligible):
    r = _view(view_exe, w, h, stride, nlevels)
    assert "error" not in r, r
    assert r["eligible"] == eligible, r
    assert r["loads"] > 100000, r            # all four readers were replayed
    assert r["outside"] == 0, r
    assert r["padding"] == 0, r              # stronger than the frame's range: no load touches a row's padding either
    assert r["plan"] == 1 and r["reflect"] == 1, r


@pytest.mark.parametrize("args", [(641, 479, 656, 8), (333, 250, 336, 8), (640, 480, 640, 8, 4), (640, 480, 644, 8),
                                  (640, 480, 640, 1)])
def test_eligibility_refuses(view_exe, args):
    r = _view(view_exe, *args)
    assert "error" not in r, r
    assert r["eligible"] == 0, r


@pytest.mark.parametrize("args", [(48, 48, 48, 3), (256, 128, 256, 3)])
def test_geometries_the_context_refuses(view_exe, args):
    r = _view(view_exe, *args)
    assert "error" in r, r
