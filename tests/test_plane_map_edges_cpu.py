"""CPU tests of the hand-built plane-map scenarios (tests/plane_map_edge_scenarios.py; DESIGN.md sections 12 and 13): the host
entries (drfe_plane_match_host, drfe_plane_flag_points_host, drfe_map_plane_update_host, drfe_map_plane_rebuild_host) and the
numpy restatements (tests/plane_match_numpy.py, tests/map_plane_numpy.py) both give the answers the builders state by hand -
indices, counts, flag bytes, cloud bits - and each scenario's precondition holds: the angles and distances are exactly the
thresholds they claim, the minimum sits at the stated index, a cloud has the stated length and order after its update, no
voxel job would be handed back by the device, and without the point or plane a case rests on the answer differs.  The device
is held to the same scenarios in tests/test_gpu_plane_map_edges.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_plane_numpy as MN  # noqa: E402
import plane_map_edge_scenarios as S  # noqa: E402
import plane_match_numpy as PN  # noqa: E402
import post_scenarios as VS  # noqa: E402

f32 = np.float32


class NumpyImpl:
    @staticmethod
    def match(Tcw, coefs, mc, bad, clouds, priors, params):
        return PN.search_map_by_coefficients(Tcw, coefs, mc, bad, clouds, *(priors or (None,) * 3), params=params)

    @staticmethod
    def flag(Tcw, coefs, mi, points, flags):
        return PN.flag_matched_plane_points(Tcw, coefs, mi, points, flags)

    update = staticmethod(MN.update)
    rebuild = staticmethod(MN.rebuild)


class HostImpl:
    @staticmethod
    def match(Tcw, coefs, mc, bad, clouds, priors, params):
        from dr_slam_amd import lib
        return lib.plane_match_host(Tcw, coefs, mc, bad, clouds, *(priors or (None,) * 3), params=np.array(params, f32))

    @staticmethod
    def flag(Tcw, coefs, mi, points, flags):
        from dr_slam_amd import lib
        return lib.plane_flag_points_host(Tcw, coefs, mi, points, flags)

    @staticmethod
    def update(Tcw, frame_xyz, map_xyz):
        from dr_slam_amd import lib
        return lib.map_plane_update_host(Tcw, frame_xyz, map_xyz)

    @staticmethod
    def rebuild(Twcs, clouds):
        from dr_slam_amd import lib
        return lib.map_plane_rebuild_host(Twcs, clouds)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_against_hand(step, got, who):
    """one replayed step against the builder's hand-stated answer"""
    if step["kind"] == "match":
        res, flags = got
        for f, (g, w) in enumerate(zip(res, step["expect"])):
            for k in range(3):
                assert np.array_equal(g[k], w[k]), (who, f, k, g, w)
            assert g[3] == w[3] and g[4] == w[4], (who, f, g[3:], w[3:])
        if step["flag_points"]:
            for s, fl in enumerate(flags):
                assert np.array_equal(fl, step["flags"][s]), (who, s, np.flatnonzero(fl != step["flags"][s])[:8])
    elif step["kind"] in ("update", "rebuild"):
        for key, want in step["clouds_after"].items():
            assert bits_equal(got[key], want), (who, key, got[key].shape, want.shape)


_SC = {}


def scenario(name):
    if not _SC:
        _SC.update({sc["name"]: sc for sc in S.all_scenarios()})
    return _SC[name]


NAMES = ["long_segments", "minimum", "flags", "many_planes", "changed_clouds", "key_values", "thresholds", "degenerate"]


def test_scenario_names():
    assert [sc["name"] for sc in S.all_scenarios()] == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_host_and_numpy_give_the_hand_stated_answers(name):
    sc = scenario(name)
    host = S.HostMaps(sc["maps"], HostImpl).replay(sc["steps"])
    nump = S.HostMaps(sc["maps"], NumpyImpl).replay(sc["steps"])
    for st, h, n in zip(sc["steps"], host, nump):
        check_against_hand(st, h, "host")
        check_against_hand(st, n, "numpy")


@pytest.mark.parametrize("name", ["changed_clouds", "long_segments"])
def test_no_voxel_job_would_be_handed_back(name):
    """The stats the builders state have host_jobs == 0.  The device hands a voxel job back exactly when libstdc++'s introsort
    gives a range above 1024 records to its heap sort (tests/test_gpu_post_edges.py); the host predicate says none of the
    inputs does - and that the ascending order, unshuffled, would, which is why the builders shuffle."""
    from dr_slam_amd import lib
    sc = scenario(name)
    hm = S.HostMaps(sc["maps"], NumpyImpl)
    jobs = 0
    for st in sc["steps"]:
        if st["kind"] == "update":
            for f, s in enumerate(st["frame_map"]):
                for q, j in enumerate(st["map_idx"][f]):
                    inp = np.vstack([MN.transform(MN.pose_update(st["Tcw"][f]), st["clouds"][f][q]), hm.clouds[s][j]])
                    assert bits_equal(inp[:len(st["clouds"][f][q])], st["clouds"][f][q])        # the identity pose moves nothing
                    assert lib.debug_order_sort_heap_max(VS.records_of(inp), 1)[1] <= S.ORD_HEAP_MAX, (s, j)
                    hm.clouds[s][j] = MN.voxel(inp)
                    jobs += 1
        elif st["kind"] == "rebuild":
            for s, j, obs in st["jobs"]:
                inp = np.vstack([MN.transform(MN.pose_rebuild(T), c) for T, c in obs])
                assert lib.debug_order_sort_heap_max(VS.records_of(inp), 1)[1] <= S.ORD_HEAP_MAX, (s, j)
                hm.clouds[s][j] = MN.voxel(inp)
                jobs += 1
        elif st["kind"] == "edit":
            hm.apply(st)
        if "stats" in st:
            assert st["stats"]["device_jobs"] == jobs and st["stats"]["host_jobs"] == 0
    if name == "long_segments":
        asc = np.vstack([S.lattice(np.arange(S.N_RESIDENT - S.N_SHARED, S.N_AFTER), 0.25), sc["maps"][0]["clouds"][0]])
        assert lib.debug_order_sort_heap_max(VS.records_of(asc), 1)[1] > S.ORD_HEAP_MAX


# --- preconditions, case by case ---------------------------------------------------------------------------------------------

def _angles(fp, m):
    pM = PN.world_coef(S.I4, fp)
    return [PN.angle_of(pM, c) for c in m["coefs"]]


def _dist(fp, cloud, Tcw=S.I4):
    return PN.point_distance_from_plane(PN.world_coef(Tcw, fp), cloud)


def _match(m, fp, params=S.DEFAULTS, Tcw=S.I4, priors=None):
    return NumpyImpl.match(Tcw, np.asarray(fp, f32).reshape(-1, 4), m["coefs"], m["bad"], m["clouds"], priors, params)


def test_thresholds_are_met_exactly():
    dTh, aTh, verTh, parTh = S.DEFAULTS
    maps = scenario("thresholds")["maps"]
    a = _angles(S.Z0, maps[0])
    assert a[0] == aTh and a[2] == -aTh and a[1] == np.nextafter(aTh, f32(1)) and a[3] == -a[1]
    assert [_dist(S.Z0, c) for c in maps[0]["clouds"]] == [1 / 64, 1 / 16, 1 / 64, 1 / 32]
    # one ulp of slack in the gate and the exactly-met planes, which carry the nearest clouds, would win
    assert _match(maps[0], S.Z0, params=(dTh, np.nextafter(aTh, f32(0)), verTh, parTh))[0][0] == 0
    assert _dist(S.Z0, maps[1]["clouds"][0]) == float(dTh) and _dist(S.Z0, maps[2]["clouds"][1]) == float(np.nextafter(dTh, f32(0)))
    assert _match(maps[1], S.Z0, params=(np.nextafter(dTh, f32(1)), aTh, verTh, parTh))[0][0] == 0
    for m in maps[3:6]:
        d = [_dist(S.Z0, c) for c in m["clouds"]]
        assert d[-1] == d[-2] == 1 / 16
    a = _angles(S.Z0, maps[6])
    assert a[0] == parTh and a[1] == a[2] == np.nextafter(parTh, f32(1)) and a[3] == verTh and a[4] == -a[5] == np.nextafter(verTh, f32(0))
    assert all(_dist(S.Z0, c) == 50.0 for c in maps[6]["clouds"])
    # PERM turns the frame plane into Z0 without rounding; the bad plane holds the nearest cloud
    fr = scenario("thresholds")["steps"][0]["frames"][8]
    assert np.array_equal(PN.world_coef(fr["Tcw"], fr["coefs"][0]), S.Z0)
    assert [_dist(S.Z0, c) for c in maps[8]["clouds"]] == [1 / 16, 1 / 64, 1 / 32] and list(maps[8]["bad"]) == [0, 1, 0]
    good = dict(maps[8], bad=np.zeros(3, np.uint8))
    assert _match(good, S.Z0)[0][0] == 1
    # NaN angles; a prior index past the plane count
    assert np.isnan(_angles(S.Z0, maps[9])[0]) and np.all(np.isnan(PN.world_coef(S.I4, [0, 0, np.nan, 0])))
    pri = scenario("thresholds")["steps"][0]["frames"][10]["priors"]
    assert pri[0][0] >= len(maps[10]["coefs"]) and _angles(S.Z0, maps[10]) == [f32(0.8)]


def test_many_planes_answers_rest_on_the_planes_past_256():
    sc = scenario("many_planes")
    for m, fr in zip(sc["maps"], sc["steps"][0]["frames"]):
        assert len(m["coefs"]) > 256 and all(1 <= len(c) <= 4 for c in m["clouds"])
        cut = dict(coefs=m["coefs"][:256], bad=m["bad"][:256], clouds=m["clouds"][:256])
        mi, pi, vi, n = _match(cut, fr["coefs"])
        assert (mi[0], pi[1], vi[2]) == (10, 10, 10)         # one trip of the gate loop: the decoy everywhere
    e = sc["steps"][0]["expect"]
    assert e[0][0][0] == 256 and e[0][1][1] == 256 and e[0][2][2] == 256
    assert e[1][0][0] == 599 and e[1][1][1] >= 256 and e[1][2][2] >= 256


def test_minimum_sits_where_stated():
    sc = scenario("minimum")
    m, fr = sc["maps"][0], sc["steps"][0]["frames"][0]
    cfg = S.min_configs()
    assert len(cfg) == 66 and {c[0] for c in cfg} == set(S.MIN_SIZES)
    for spot in S.MIN_SPOTS + (4096, 2112, 62, 0):
        assert any(at == spot for _, at, _ in cfg)
    assert any(n - at == 1 and n % S.PM_CHUNK == 1 for n, at, _ in cfg)       # a last chunk that holds the near point only
    for c, (n, at, near) in enumerate(cfg):
        pM = PN.world_coef(S.I4, fr["coefs"][c])
        cl = m["clouds"][2 * c]
        d = np.abs(cl[:, 2] + pM[3])
        assert len(cl) == n and int(np.argmin(d)) == at and d[at] == near and np.all(np.delete(d, at) == 0.5)
        assert _dist(fr["coefs"][c], m["clouds"][2 * c + 1]) == 1 / 16
        others = [_dist(fr["coefs"][c], m["clouds"][j]) for j in (2 * c - 1, 2 * c + 2) if 0 <= j < len(m["clouds"])]
        assert all(o >= 7 for o in others)
    # without the near points every frame plane takes its one-point plane
    blind = dict(m, clouds=[cl.copy() for cl in m["clouds"]])
    for c in range(len(cfg)):
        blind["clouds"][2 * c][:, 2] = 8.0 * (c + 1) + 0.5
    mi = _match(blind, fr["coefs"])[0]
    assert list(mi) == [2 * c + 1 for c in range(len(cfg))]


def test_key_values_are_what_they_claim():
    sc = scenario("key_values")
    cl = [m["clouds"] for m in sc["maps"]]
    pX = PN.world_coef(S.I4, S.X0)
    x, y, z = cl[0][0][0]
    prod = pX[0] * x
    assert prod == 0 and np.signbit(prod) and np.signbit(f32(prod + pX[1] * y)) and _dist(S.X0, cl[0][0]) == 0.0
    assert _dist(S.X0, cl[0][0][1:]) == 0.5
    assert np.abs(cl[1][0][0, 2]).view(np.uint32) == 0x42C80000 and _dist(S.Z0, cl[1][0]) == 100.0
    assert _dist(S.Z0, cl[2][0]) == 100.0 and _dist(S.Z0, cl[2][1]) == 100.0 and cl[2][0][:, 2].min() > cl[2][1][0, 2] > 100
    assert np.isinf(cl[3][0][0, 2]) and _dist(S.Z0, cl[3][0]) == 100.0
    assert _dist(S.Z0, cl[4][0]) == 1 / 16 and _dist(S.Z0, cl[4][0][:2]) == 100.0
    assert _dist(S.Z0, cl[5][0]) == 1 / 16 and np.all(cl[5][0][:2, 2] == 0) and np.signbit(cl[5][0][1, 2])
    s2, s1 = cl[6][0][0, 2], cl[6][1][0, 2]
    assert 0 < s1 < s2 < np.finfo(f32).tiny and [int(v.view(np.uint32)) for v in (s1, s2)] == [1, 2]
    assert _dist(S.Z0, cl[6][0]) == float(s2) and _dist(S.Z0, cl[6][1]) == float(s1)
    assert len(cl[7][0]) == S.PM_CHUNK + 1 and _dist(S.Z0, cl[7][0][:S.PM_CHUNK]) == 100.0 and _dist(S.Z0, cl[7][0]) == 1 / 16
    assert np.signbit(cl[7][0][:S.PM_CHUNK, 2]).sum() == S.PM_CHUNK // 2
    assert len(cl[8][0]) == 0 and _dist(S.Z0, cl[9][0]) == 100.0 and len(cl[9][0]) == 3


def test_flag_points_sit_on_the_half_boundary_at_the_seams():
    sc = scenario("flags")
    below = np.nextafter(f32(0.5), f32(0))
    sizes = [len(m["points"]) for m in sc["maps"]]
    assert sizes == [2047, 0, 1, 2048, 2049, 4097, 2047, 2048, 2049, 4097]
    want = sc["steps"][0]["flags"]
    for s, m in enumerate(sc["maps"]):
        n, exact = sizes[s], s >= 6
        spots = sorted({i for i in S.FLAG_SPOTS if i < n} | ({n - 1} if n else set()))
        d = np.abs(m["points"][:, 2])
        for i in spots:
            assert d[i] == (0.5 if exact else below) and want[s][i] == (0 if exact else 1)
        if n > 5:
            assert np.isnan(m["points"][2, 0]) and want[s][2] == 0
        if s != 5:
            with np.errstate(invalid="ignore"):
                hit = (d < 0.5) & ~np.isnan(m["points"][:, 0])
            assert np.array_equal(hit.astype(np.uint8), want[s]) and np.all((d[hit] == below))
    # map 5: the two frames' sets are disjoint and both non-empty
    p5 = sc["maps"][5]["points"]
    with np.errstate(invalid="ignore"):
        zs, xs = (np.abs(p5[:, 2]) < 0.5) & ~np.isnan(p5[:, 0]), np.abs(p5[:, 0]) < 0.5
    assert zs.sum() == 6 and xs.sum() == 136 and not (zs & xs).any() and np.array_equal((zs | xs).astype(np.uint8), want[5])
    # the unmatched frame's plane would flag nearly every point of map 3
    fl, n = PN.flag_matched_plane_points(S.I4, [S.zplane(-2)], [0], sc["maps"][3]["points"])
    assert n > 2000


def test_changed_clouds_put_the_deciding_points_past_the_seam():
    sc = scenario("changed_clouds")
    hm = S.HostMaps(sc["maps"], NumpyImpl)
    fp = sc["steps"][0]["frames"][0]["coefs"][0]
    pM = PN.world_coef(S.I4, fp)
    dTh = float(S.TIGHT[0])

    def near(cloud):
        return np.flatnonzero(np.abs(cloud[:, 2] + pM[3]) < dTh)

    assert len(near(hm.clouds[0][0])) == 0 and len(near(hm.clouds[2][0])) == 0 and list(near(hm.clouds[1][0])) == [4099]
    assert len(hm.clouds[0][0]) == 2040 and len(hm.clouds[1][0]) == 4100 and len(hm.clouds[2][0]) == 2000
    steps = [st for st in sc["steps"] if st["kind"] != "match"]
    assert [st["kind"] for st in sc["steps"]] == ["match", "update", "match", "match", "rebuild", "edit", "edit", "rebuild", "match", "match"]
    assert [[fr["map"] for fr in st["frames"]] for st in sc["steps"] if st["kind"] == "match"] == [[0, 1, 2, 3, 4], [0], [2], [3], [0, 1, 2, 3, 4]]
    hm.replay(steps)
    assert len(hm.clouds[0][0]) == 2060 and list(near(hm.clouds[0][0])) == list(range(2048, 2060))
    assert len(hm.clouds[2][0]) == 2060 and list(near(hm.clouds[2][0])) == list(range(2048, 2060))
    assert len(hm.clouds[1][0]) == 10 and len(near(hm.clouds[1][0])) == 0
    assert len(hm.coefs[3]) == 2 and len(hm.clouds[3][1]) == 10 and list(hm.bad[4]) == [1, 0]
    # the first chunk alone (what a work list sized before the update would cover) gives no match
    for s in (0, 2):
        assert _dist(fp, hm.clouds[s][0][:S.PM_CHUNK]) > dTh > _dist(fp, hm.clouds[s][0])
    # the second frame plane of map 2's frame is the one that crosses the seam
    st = sc["steps"][1]
    assert len(sc["maps"][2]["clouds"][0]) + len(st["clouds"][1][0]) < S.PM_CHUNK < len(hm.clouds[2][0])


def test_long_segments_pass_every_stride_trip():
    sc = scenario("long_segments")
    st = sc["steps"]
    assert len(st[0]["clouds"][0][0]) == 70000 > S.MP_TRIP and len(sc["maps"][0]["clouds"][0]) == 30000 and 3 * 30000 > S.MP_TRIP
    assert [s["kind"] for s in st] == ["update", "update", "match", "update", "match"]
    a1, a2, a3 = (s["clouds_after"][(0, 0)] for s in (st[0], st[1], st[3]))
    assert len(a1) == len(a2) == 95000 and len(a3) == 95001 and 3 * 95000 > 2 * S.MP_TRIP
    assert len(st[1]["clouds"][0][0]) + len(a1) == S.SLOT and len(st[3]["clouds"][0][0]) + len(a2) == S.SLOT + 1
    assert st[0]["stats"]["repacks"] == st[1]["stats"]["repacks"] == 1 and st[3]["stats"]["repacks"] == 2
    # every cloud is one point per leaf, in leaf order
    for a in (a1, a2, a3):
        k = VS.leaf_keys(a)
        assert np.all(np.diff(k.astype(np.int64)) > 0)
    # the shared leaves changed, the others kept their point's bits
    res, fr1 = sc["maps"][0]["clouds"][0], S.lattice(np.arange(25000, 95000), 0.25)
    assert bits_equal(a1[:25000], res[:25000]) and bits_equal(a1[30000:], fr1[5000:])
    assert not np.any(np.all(a1[25000:30000] == res[25000:], 1)) and not np.any(np.all(a1[25000:30000] == fr1[:5000], 1))
    # the match after update 2 rests on points from index 65 536 on, the one after update 3 on the last point alone
    dTh = float(S.TIGHT[0])
    fp = st[2]["frames"][0]["coefs"][0]
    d = np.abs(a2[:, 2] + fp[3])
    assert np.all(d[65536:] == 0) and d[:65536].min() > dTh and _dist(fp, a2[:30 * S.PM_CHUNK]) > dTh
    fp = st[4]["frames"][0]["coefs"][0]
    d = np.abs(a3[:, 2] + fp[3])
    assert d[-1] == 0 and d[:-1].min() > 0.04 and _dist(fp, a2) > dTh
