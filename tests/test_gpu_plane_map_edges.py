"""-m gpu tests of the resident plane map on hand-built scenarios (tests/plane_map_edge_scenarios.py; DESIGN.md sections 12
and 13): plane_map_upload + plane_match_batch + plane_match_download / plane_flags_download, and where a scenario changes the
clouds plane_map_update_batch / plane_map_rebuild_batch / plane_map_edit + plane_map_cloud_download / plane_map_update_stats,
against three things at once: the answer the builder states by hand, the numpy restatement and the host entries replayed on
host-held maps.  Indices, counts and flag bytes are equal, clouds are bit-equal, the stats are the stated ones (no job comes
back to the host); nothing here has a tolerance.  The scenarios aim at what only the device has: k_pm_gate's stride over more
than 256 map planes, the work list's chunks of 2048 points and its capacity from the host's mirror of the cloud sizes, the
wavefront min and the `k < start value` test before the atomicMin, k_pm_flags' block seams and wavefront count, and the
stride trips of k_mp_gather / k_mp_commit / k_mp_move past 65 536 elements.  tests/test_plane_map_edges_cpu.py proves on the
host that each construction reaches what it aims at.

All scenarios share one context and run in the builders' order, the larger uploads and calls first, and every scenario runs
twice in a row (a fresh upload each time), so accumulators, reused buffers and stale contents of grown ones are covered."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_map_edge_scenarios as S  # noqa: E402
from test_plane_map_edges_cpu import NAMES, HostImpl, NumpyImpl, bits_equal, check_against_hand  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    from dr_slam_amd import lib
    c = lib.Context()
    yield c
    c.close()


_REF = {}


def reference(name):
    """(scenario, host replay, numpy replay), computed once"""
    if not _REF:
        for sc in S.all_scenarios():
            _REF[sc["name"]] = (sc, S.HostMaps(sc["maps"], HostImpl).replay(sc["steps"]), S.HostMaps(sc["maps"], NumpyImpl).replay(sc["steps"]))
    return _REF[name]


def device_match(c, step, n_maps):
    """the step through plane_match_batch, in the shape HostMaps.match returns"""
    import torch
    from dr_slam_amd import lib
    frames = step["frames"]
    pri = [[None if fr["priors"] is None else fr["priors"][k] for fr in frames] for k in range(3)]
    c.plane_match_batch([fr["map"] for fr in frames], np.stack([fr["Tcw"] for fr in frames]), [fr["coefs"] for fr in frames], *pri,
                        flag_points=step["flag_points"], params=np.array(step["params"], f32),
                        stream=torch.cuda.current_stream().cuda_stream)
    res = [c.plane_match_download(f) for f in range(len(frames))]
    if step["flag_points"]:
        return res, [c.plane_flags_download(s) for s in range(n_maps)]
    with pytest.raises(lib.DrfeError):
        c.plane_flags_download(0)                  # no flags of a call that did not ask for them
    return res, None


def device_step(c, step, n_maps):
    if step["kind"] == "match":
        return device_match(c, step, n_maps)
    if step["kind"] == "update":
        c.plane_map_update_batch(step["frame_map"], step["Tcw"], step["clouds"], map_idx=step["map_idx"])
    elif step["kind"] == "rebuild":
        c.plane_map_rebuild_batch(step["jobs"])
    elif step["kind"] == "edit":
        c.plane_map_edit(step["map"], step["index"], coefs=step["coefs"], bad=step["bad"])
        return None
    assert c.plane_map_update_stats() == step["stats"], (c.plane_map_update_stats(), step["stats"])
    return {key: c.plane_map_cloud_download(*key) for key in step["clouds_after"]}


def same_step(step, got, ref, who):
    """device against one replay: everything equal, clouds bit for bit"""
    if step["kind"] == "match":
        for f, (g, r) in enumerate(zip(got[0], ref[0])):
            assert all(np.array_equal(g[k], r[k]) for k in range(3)) and g[3] == r[3] and g[4] == r[4], (who, f, g, r)
        if step["flag_points"]:
            for s, (g, r) in enumerate(zip(got[1], ref[1])):
                assert np.array_equal(g, r), (who, s)
    elif got is not None:
        for key in got:
            assert bits_equal(got[key], ref[key]), (who, key)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", NAMES)
def test_device_gives_the_hand_stated_answers(ctx, name):
    sc, host, nump = reference(name)
    for run in range(2):
        ctx.plane_map_upload(sc["maps"])
        for i, (st, h, n) in enumerate(zip(sc["steps"], host, nump)):
            got = device_step(ctx, st, len(sc["maps"]))
            if st["kind"] == "match" and not st["flag_points"]:
                got = (got[0], [])
            check_against_hand(st, got, f"device, run {run}, step {i}")
            same_step(st, got, h, f"host entry, run {run}, step {i}")
            same_step(st, got, n, f"numpy, run {run}, step {i}")
