"""Host tests of LocalMapping::MapPlaneCulling: every hand-built scene takes the path it was built for
(on the numpy restatement alone), drfe_plane_map_cull_host equals the restatement bit for bit on every scene, refused
arguments, and the symbols, constants and dispatch threshold are held to include/drfe.h and profiles/plane_cull_timing.jsonl."""
import copy
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_cull_numpy as un  # noqa: E402
import plane_cull_scenarios as us  # noqa: E402
from dr_slam_amd import lib  # noqa: E402

SCENARIOS = us.all_scenarios()
_REF = {}


def reference(name):
    """the restatement's result of a scene, computed once"""
    if name not in _REF:
        _REF[name] = un.cull(SCENARIOS[name]["scene"])
    return _REF[name]


same = us.same


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_premise(name):
    """the scene takes the path it exists for: asserted on the restatement, not on the code under test"""
    sc = SCENARIOS[name]
    assert len(sc["scene"]["coefs"]) <= 24 and all(len(c) <= 2 * us.C + 1 for c in sc["scene"]["clouds"])
    assert sc["needs"](reference(name), sc["scene"]), sc["premise"]


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_host_equals_restatement(name):
    same(lib.plane_map_cull_host(SCENARIOS[name]["scene"]), reference(name))


def test_random_maps_meet_the_condition():
    for seed in us.RANDOM_SEEDS:
        r = reference(f"random_{seed}")
        assert len(r["events"]) >= 3 and r["counters"]["stale_columns"] >= 1 and all(n >= 1 for n in r["paths"]["verdicts"]), seed
        s = SCENARIOS[f"random_{seed}"]["scene"]
        assert len(s["coefs"]) == 24 and len(s["Twc"]) == 40 and all(200 <= len(c) <= 700 for c in s["clouds"])


def test_lazy_rebuild_equals_the_eager_one():
    """the restatement rebuilds inside Replace, the entries right before the next read: `rebuilds` counts clouds that were read or
    left, so two merges into one survivor with no read between count once"""
    r = reference("row_tiles")
    assert r["counters"]["rebuilds"] == 2 and len(r["events"]) == 2
    r = reference("rebuilt_twice_with_a_read_between")
    assert r["counters"]["rebuilds"] == r["counters"]["stale_columns"] == 2


def _refused(scene, **kw):
    with pytest.raises(lib.DrfeError) as e:
        lib.plane_map_cull_host(scene, **kw)
    return str(e.value)


def test_validation():
    base = SCENARIOS["shared_keyframe_chain"]["scene"]
    s = copy.deepcopy(base)
    s["obs"][0] = s["obs"][0][::-1]                              # not in key-frame order
    assert "(-1)" in _refused(s)
    s = copy.deepcopy(base)
    s["obs"][1] = [s["obs"][1][0], s["obs"][1][0]]               # one key frame twice
    assert "(-1)" in _refused(s)
    s = copy.deepcopy(base)
    s["recent"] = [3]
    assert "(-1)" in _refused(s)
    s = copy.deepcopy(base)
    s["recent"] = [-2]
    assert "(-1)" in _refused(s)
    assert "(-3)" in _refused(base, rebuilt_capacity=1)          # two clouds are rebuilt
    L = lib.load()
    assert L.drfe_plane_map_cull_host(None, None, None, None, None, None) == -1
    assert L.drfe_plane_map_cull_limits(None) == -1
    # a stride below three floats or off the float grid
    cin, cout, keep, o = lib._plane_cull_pack(base)
    coefs = np.ascontiguousarray(base["coefs"], np.float32)
    bad = np.ascontiguousarray(base["bad"], np.uint8)
    coff, xyz = lib._clouds_csr(list(base["clouds"]))
    for stride in (8, 18):
        cin.obs_cloud_stride = stride
        assert L.drfe_plane_map_cull_host(lib.C.byref(cin), lib._p(coefs), lib._p(bad), lib._p(coff), lib._p(xyz), lib.C.byref(cout)) == -1
    cin.obs_cloud_stride = lib.PLANE_CULL_CLOUD_STRIDE
    cin.n_kfs = 3                                                # observations name key frames 3, 4 and 5
    assert L.drfe_plane_map_cull_host(lib.C.byref(cin), lib._p(coefs), lib._p(bad), lib._p(coff), lib._p(xyz), lib.C.byref(cout)) == -1
    cin.n_kfs = 6
    assert L.drfe_plane_map_cull_host(lib.C.byref(cin), lib._p(coefs), lib._p(bad), lib._p(coff), lib._p(xyz), lib.C.byref(cout)) == 0
    coff[1] = coff[2] + 1                                        # decreasing cloud offsets
    assert L.drfe_plane_map_cull_host(lib.C.byref(cin), lib._p(coefs), lib._p(bad), lib._p(coff), lib._p(xyz), lib.C.byref(cout)) == -1


def test_only_xyz_of_a_strided_cloud_is_read():
    """the wrappers pack observation clouds at PointXYZ's 16 bytes with NaN in the pad: a read of the pad would poison a cloud"""
    r = lib.plane_map_cull_host(SCENARIOS["stale_column_grows"]["scene"])
    assert lib.PLANE_CULL_CLOUD_STRIDE == 16 and all(np.isfinite(c).all() for c in r["clouds"].values())


def _header():
    return open(os.path.join(lib._HERE, "..", "include", "drfe.h")).read()


def test_symbols_and_constants():
    L = lib.load()
    for s in lib.SYMBOLS:
        if "plane_map_cull" in s:
            assert hasattr(L, s), s
    assert sum("plane_map_cull" in s for s in lib.SYMBOLS) == 4
    text = _header()
    lim = lib.plane_map_cull_limits()
    assert int(re.search(r"DRFE_PLANE_CULL_DEVICE_FROM = (\d+)", text).group(1)) == lim["device_from"] == lib.PLANE_CULL_DEVICE_FROM
    assert int(re.search(r"DRFE_PLANE_CULL_MAX_PLANES = (\d+)", text).group(1)) == lim["max_planes"]
    assert (lim["chunk"], lim["row_tile"]) == (us.C, us.TILE) and lim["chunk"] % 256 == 0
    names = ("KEPT", "ERASED_BAD", "BAD_BY_RATIO", "BAD_BY_OBSERVATIONS", "ERASED_BY_AGE")
    for n in names:
        v = int(re.search(rf"DRFE_PLANE_CULL_{n} = (\d+)", text).group(1))
        assert v == getattr(lib, f"PLANE_CULL_{n}") == getattr(un, n)
    assert lib.PLANE_CULL_COUNTERS == tuple(un.cull(SCENARIOS["no_planes"]["scene"])["counters"])


def test_device_from_is_the_measured_crossover():
    """profiles/plane_cull_timing.jsonl (tools/plane_cull_timing.py): its last line is the constant, and the rows give it"""
    rows = [json.loads(x) for x in open(os.path.join(lib._HERE, "..", "profiles", "plane_cull_timing.jsonl"))]
    measured = rows[-1]["device_from"]
    lim = lib.plane_map_cull_limits()
    assert lim["device_from"] == (measured if measured is not None else lim["max_planes"] + 1)
    shapes = rows[:-1]
    assert {r["planes"] for r in shapes} == {16, 64, 256} and {r["cloud_points"] for r in shapes} == {500, 4000}
    assert {r["with_events"] for r in shapes} == {0, 1} and len(shapes) == 12
    assert all(r["equal"] and r["device_reps"] >= 5 and r["host_reps"] >= 5 for r in shapes)
    for r in shapes:
        assert r["device_wins"] == (r["host_ms"] - r["device_ms"] > max(r["host_iqr_ms"], r["device_iqr_ms"]))      # medians
        assert (r["events"] > 0) == bool(r["with_events"])
    sizes = sorted({r["planes"] for r in shapes})
    wins = {n: all(r["device_wins"] for r in shapes if r["planes"] == n) for n in sizes}
    want = None
    for n in reversed(sizes):                       # the smallest size from which the device wins at every other axis
        if not wins[n]:
            break
        want = n
    assert measured == want
