"""The quadtree plan (drfe_quadtree_plan, orb_geometry.cpp) without a device: which k_quadtree instantiation every level runs
and how the levels are grouped into launches, through lib.quadtree_plan.

BENCH_COUNTS are the most FAST candidates per level the CPU oracle finds on six frames of the benchmark's two scenes
(sharding.render_sequence(10, 3, synth.TUM3, kind) for room_boxes and living_room) at 640x480 / 1000 / 1.2 / 8."""
import pytest

from dr_slam_amd import lib

BENCH_COUNTS = (7286, 4070, 2454, 1489, 947, 587, 363, 202)
# (threads, kpt) -> node-list capacities the library holds
INSTANCES = {(512, 16): (256, 1024), (256, 12): (256,), (64, 20): (128,)}
GEOMETRIES = [(640, 480, nf, 1.2, 8) for nf in (500, 1000, 2000)] + [(333, 250, 1000, 1.2, 8), (1280, 960, 1000, 1.2, 8),
                                                                     (640, 480, 1000, 2.0, 3), (640, 480, 1000, 1.1, 12)]


def _plan(w, h, nf, sf, nl, nframes=512, force=None):
    return lib.quadtree_plan(w, h, nfeatures=nf, scale_factor=sf, nlevels=nl, nframes=nframes, force=force)


def _invariants(plan):
    for r in plan:
        assert (r["threads"], r["kpt"]) in INSTANCES and r["maxn"] in INSTANCES[(r["threads"], r["kpt"])], r
        assert r["maxn"] >= r["kp_cap"], r
        assert 2 * r["threads"] >= r["maxn"], r
        if r["threads"] == 64:
            assert r["kp_cap"] <= 128, r
    # launches are runs of levels with one instantiation, numbered in level order
    assert plan[0]["launch"] == 0
    for a, b in zip(plan, plan[1:]):
        same = (a["threads"], a["kpt"], a["maxn"]) == (b["threads"], b["kpt"], b["maxn"])
        assert b["launch"] == a["launch"] + (0 if same else 1), (a, b)


def test_bench_geometry_keeps_every_level_in_registers():
    plan = _plan(640, 480, 1000, 1.2, 8)
    _invariants(plan)
    for r, n in zip(plan, BENCH_COUNTS):
        assert r["threads"] * r["kpt"] >= 1.1 * n, (r, n)
    # the heaviest launch comes first: register capacity never grows with the level
    caps = [r["threads"] * r["kpt"] for r in plan]
    assert caps == sorted(caps, reverse=True)


@pytest.mark.parametrize("w,h,nf,sf,nl", GEOMETRIES)
@pytest.mark.parametrize("nframes", [1, 64, 65, 512])
def test_invariants(w, h, nf, sf, nl, nframes):
    plan = _plan(w, h, nf, sf, nl, nframes)
    assert len(plan) == nl
    _invariants(plan)
    if nl * nframes <= 512:
        # a batch that is resident at once is one launch of the 512-thread kernel
        assert {r["launch"] for r in plan} == {0} and {r["threads"] for r in plan} == {512}


def test_large_nfeatures_keep_the_1024_node_instance():
    plan = _plan(640, 480, 2000, 1.2, 8)
    assert plan[0]["kp_cap"] > 256 and (plan[0]["threads"], plan[0]["maxn"]) == (512, 1024)
    for r in plan:
        assert (r["maxn"] == 1024) == (r["kp_cap"] > 256), r


@pytest.mark.parametrize("w,h,nf,sf,nl", GEOMETRIES + [(160, 120, 124, 1.2, 1), (160, 120, 125, 1.2, 1)])
@pytest.mark.parametrize("threads,kpt", sorted(INSTANCES))
@pytest.mark.parametrize("nframes", [1, 512])
def test_override_is_honoured_only_where_legal(w, h, nf, sf, nl, threads, kpt, nframes):
    own = _plan(w, h, nf, sf, nl, nframes)
    forced = _plan(w, h, nf, sf, nl, nframes, force=f"{threads},{kpt}")
    _invariants(forced)
    for o, f in zip(own, forced):
        if max(INSTANCES[(threads, kpt)]) >= o["kp_cap"]:
            assert (f["threads"], f["kpt"]) == (threads, kpt), (o, f)
            assert f["maxn"] == min(m for m in INSTANCES[(threads, kpt)] if m >= o["kp_cap"])
        else:
            assert (f["threads"], f["kpt"], f["maxn"]) == (o["threads"], o["kpt"], o["maxn"]), (o, f)


def test_override_per_level_and_malformed():
    own = _plan(640, 480, 1000, 1.2, 8)
    p = _plan(640, 480, 1000, 1.2, 8, force="512,16;256,12;64,20")
    assert [(r["threads"], r["kpt"]) for r in p[:2]] == [(512, 16), (256, 12)]
    # the last pair is repeated: levels whose node capacity exceeds 128 keep their own instantiation, the others take the wavefront
    assert own[2]["kp_cap"] > 128 and own[7]["kp_cap"] <= 128
    for o, r in zip(own[2:], p[2:]):
        assert (r["threads"], r["kpt"]) == ((64, 20) if o["kp_cap"] <= 128 else (o["threads"], o["kpt"])), (o, r)
    for bad in ("", "512", "512,", "3,5", "512,16,", "a,b", "512;16"):
        q = _plan(640, 480, 1000, 1.2, 8, force=bad)
        assert [(r["threads"], r["kpt"], r["maxn"]) for r in q] == [(r["threads"], r["kpt"], r["maxn"]) for r in own], bad


def test_wave_boundary_geometry():
    """nfeatures 124 gives kp_cap 128, 125 gives 129: the one-wavefront instance is legal for the first only."""
    a = _plan(160, 120, 124, 1.2, 1, 1, force="64,20")[0]
    b = _plan(160, 120, 125, 1.2, 1, 1, force="64,20")[0]
    assert (a["kp_cap"], a["threads"]) == (128, 64)
    assert b["kp_cap"] == 129 and b["threads"] != 64
