"""Host-side layout of the tiled pyramid resize (k_pyr_resize_tile), without a device.

tests/native/resize_plan.cpp builds a context's geometry through orb_geometry.cpp and replays, per level, the kernel's
mapping of items (4 x 4 pixels) to the bordered level: lane coverage, exactly-once stores (direct or mirrored), and that
every tap lies inside its block's LDS tile and every tile inside the source level.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resize_plan") / "resize_plan")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-DDRFE_NO_ROCTX",
                    "-I/opt/rocm/include", os.path.join(ROOT, "tests", "native", "resize_plan.cpp"),
                    os.path.join(ROOT, "dr_slam_amd", "csrc", "orb_geometry.cpp"), "-o", exe], check=True)
    return exe


def _plan(exe, w, h, scale, nlevels):
    out = subprocess.run([exe, str(w), str(h), str(scale), str(nlevels)], capture_output=True, text=True, check=True).stdout
    rows = []
    for line in out.split("\n"):
        if line:
            l, lw, lh, lds, fill, cover, exact, windows = line.split()
            rows.append(dict(level=int(l), w=int(lw), h=int(lh), lds=int(lds), fill=int(fill), cover=float(cover),
                             exact=int(exact), windows=int(windows)))
    assert len(rows) == nlevels - 1
    return rows


@pytest.mark.parametrize("w,h,scale,nlevels", [
    (640, 480, 1.2, 8), (1280, 960, 1.2, 8), (641, 479, 1.2, 8), (653, 487, 1.2, 8), (752, 480, 1.2, 8),
    (333, 250, 1.2, 8), (640, 480, 1.1, 12), (640, 480, 1.3, 6), (640, 480, 1.5, 5), (640, 480, 1.7, 4),
    (640, 480, 2.0, 3), (1280, 960, 2.0, 3), (1600, 1200, 2.0, 3)])
def test_every_bordered_pixel_once_and_dense_lanes(plan_exe, w, h, scale, nlevels):
    for r in _plan(plan_exe, w, h, scale, nlevels):
        assert r["exact"] == 1, r
        assert r["windows"] == 1, r
        assert r["cover"] >= 0.95, r


def test_default_geometries_take_the_tile_kernel(plan_exe):
    for w, h in ((640, 480), (1280, 960)):
        for r in _plan(plan_exe, w, h, 1.2, 8):
            assert r["lds"] == 1 and 1 <= r["fill"] <= 8, r


def test_oversized_windows_fall_back(plan_exe):
    """1600x1200 at scale 2: level 1's blocks need more than eight 16-byte loads per thread and run k_pyr_resize."""
    rows = _plan(plan_exe, 1600, 1200, 2.0, 3)
    assert rows[0]["lds"] == 0 and rows[1]["lds"] == 1


def test_scale_factor_limit_is_kept(plan_exe):
    p = subprocess.run([plan_exe, "640", "480", "3.0", "3"], capture_output=True, text=True)
    assert p.returncode == 1 and "up to 2.0" in p.stdout
