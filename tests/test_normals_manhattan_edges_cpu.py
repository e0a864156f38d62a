"""CPU tests of the hand-built scenarios for surface normals -> Manhattan tracking (tests/normals_manhattan_scenarios.py;
DESIGN.md sections 9 and 11).  Every scenario goes through the oracle (oracle/post_oracle.cpp), the host entry
drfe_manhattan_track_host and the numpy restatement tests/manhattan_numpy.py, host == numpy bit for bit, and every scenario
must reach the branch or seam it names: that is asserted here from the oracle's cloud and normals, from `info`, from the bit
words and from the restatement's `hits` counter, so that tests/test_gpu_normals_manhattan_edges.py, which holds the device to
the same scenarios, never runs a construction that misses its target.  The only numeric conditions are on the inputs (counts,
gates, seeds); nothing here has a tolerance.

The oracle has no tap for the chamfer distance.  It is tied to the plain restatement in the scenarios module by what the
distance decides: a point carries a normal exactly where it is finite, inside the 10-point border and the restated window
min(dist, 10) is above 2 - on every scenario, the non-finite one included (the oracle defines non-finite depth: NaN and -inf
stay in the cloud and seed the depth-change map, +inf is above Point.MaxDistance and is zeroed)."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manhattan_numpy as MN  # noqa: E402
import normals_manhattan_scenarios as S  # noqa: E402

NORMALS = [sc["name"] for sc in S.normals_scenarios()]
MANHATTAN = [sc["name"] for sc in S.manhattan_scenarios()]
_ORACLE = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_floats(got, want):
    """NaN in the same places, identical float bits elsewhere"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def oracle_normals(O, depth_m, K4, maxd):
    """(cloud, normals, records) of one depth image by the oracle, computed once per image"""
    from dr_slam_amd import lib
    key = (np.asarray(depth_m).tobytes(), np.asarray(depth_m).shape, float(maxd))
    if key not in _ORACLE:
        cloud, nrm = O.post_surface_normals(depth_m, K4, maxd)
        on, oc, fx, fy = O.post_surface_normal_records(cloud, nrm)
        r = np.zeros(len(on), lib.SURFACE_NORMAL_DTYPE)
        r["normal"], r["camera_position"], r["frame_x"], r["frame_y"] = on, oc, fx, fy
        _ORACLE[key] = (cloud, nrm, r)
    return _ORACLE[key]


def check_records(rec, want):
    """the bar of tests/test_gpu_post.py::_check_records against the oracle's records"""
    assert len(rec) == len(want)
    assert same_floats(rec["normal"], want["normal"])
    assert same_floats(rec["camera_position"], want["camera_position"])
    assert np.array_equal(rec["frame_x"], want["frame_x"]) and np.array_equal(rec["frame_y"], want["frame_y"])


@pytest.mark.parametrize("name", NORMALS)
def test_normals_scenario_reaches_what_it_names(oracle_mod, name):
    sc = S.normals_scenarios()[NORMALS.index(name)]
    cam = sc["cam"]
    W, H = S.cloud_size(cam.w, cam.h)
    cloud, nrm, recs = oracle_normals(oracle_mod, sc["depth_m"], cam.K4, sc["maxd"])
    assert cloud.shape == (H, W, 3) and len(recs) == (W // 2) * (H // 2)
    if sc["d16"] is not None:
        assert np.array_equal(bits(sc["depth_m"]), bits(oracle_mod.depth_to_float(sc["d16"], S.INV)))
    z = S.cloud_z(sc["depth_m"], sc["maxd"])
    assert same_floats(z, cloud[..., 2])
    seed, dist = S.seeds(z), S.scenario_dist(sc)
    has = ~np.isnan(nrm).any(2)
    rw = S.window(dist)
    assert np.array_equal(has, S.interior(W, H) & (rw > 0) & np.isfinite(z))
    assert np.isnan(recs["normal"]).all(1).sum() + has[1::2, 1::2][:H // 2, :W // 2].sum() == len(recs)
    if "seeds" in sc:
        assert np.array_equal(seed, sc["seeds"])
    if sc.get("sizing"):
        assert seed.any() and (dist > 10).any() and has.sum() > 1000
    if "n_normals" in sc:
        assert has.sum() == sc["n_normals"] and (~np.isnan(recs["normal"]).any(1)).sum() == sc["n_record_normals"]
        if sc["n_record_normals"]:
            assert has[11, 11] and recs["frame_x"][~np.isnan(recs["normal"]).any(1)][0] == 33
    if "wrap_matters" in sc:
        assert (S.chamfer(seed, wrap=False) != dist).any() == sc["wrap_matters"]
    if sc.get("all_windows"):
        inner = S.interior(W, H)
        assert set(np.unique(rw[inner])) == {0} | set(range(2, 11))
        one, diag = np.float32(1.0), np.float32(1.4)
        assert {one, diag, one + one, diag + one, diag + diag} <= set(np.unique(dist[inner]))
        assert not has[inner & (dist <= 2.0)].any() and has[inner & (dist > 2.0)].all()
    if name == "jump_threshold":
        a, k = S.threshold_pair()
        da, db = np.float32(a) * S.INV, np.float32(a + k) * S.INV
        assert abs(da - db) == (np.float32(0.05) * (abs(da) + np.float32(1.0))) * np.float32(2.0)
        assert z[15, 15] == db and not seed[15, 14:17].any() and not seed[14, 15]
    if name == "max_distance_u16":
        raw = sc["d16"][::3, ::3]
        assert (raw == 15000).sum() >= 3 and (z[raw == 15000] == sc["maxd"]).all() and (z[raw <= 15000] > 0).all()
        assert (raw == 15001).any() or (raw > 15000).any()
        assert (cloud[raw > 15000] == 0).all()
    if "kept" in sc:
        assert z[sc["kept"]] == sc["maxd"] and (cloud[sc["zeroed"]] == 0).all()
        assert sc["depth_m"][3 * sc["zeroed"][0], 3 * sc["zeroed"][1]] == np.nextafter(sc["maxd"], np.float32(np.inf))
    if name == "nonfinite":
        assert np.isnan(z).sum() == 10 and np.isinf(z).sum() == 1 and z[20, 40] == 0
        assert seed[20, 20] and seed[31, 29] and seed[35, 50] and seed[20, 40] and not has[seed].any()


def replay(recs, call, hits):
    """one manhattan_track_batch call on the host: the host entry chained frame to frame, the numpy restatement on every frame
    from the same start; -> per frame (R_in, R_out, info, rec_bits, line_bits)"""
    from dr_slam_amd import lib
    out = []
    for s in range(call["nseq"]):
        R = call["R0"][s]
        for t in range(call["seq_len"]):
            f = s * call["seq_len"] + t
            d = call["dirs"][call["loff"][f]:call["loff"][f + 1]]
            Rh, ih, rbh, lbh = lib.manhattan_track_host(R, recs[f], d, call["n_calls"])
            Rn, infos, rbn, lbn, _ = MN.track(R, recs[f]["normal"], d, call["n_calls"], hits)
            MN.assert_equal_to_product(Rn, infos, rbn, lbn, Rh, ih, rbh, lbh)
            out.append((R, Rh, ih, rbh, lbh))
            R = Rh
    return out


def check_expect(exp, R_in, R_out, info, rb, lb, who):
    """the answer the builder states for call 0 of a frame"""
    c0 = info["call"][0]
    for key in ("found", "svd", "threshold", "deficient"):
        if key in exp:
            assert int(c0[key]) == exp[key], (who, key, int(c0[key]), exp[key])
    for key in ("n_selected", "in_cone"):
        if key in exp:
            assert list(c0[key]) == exp[key], (who, key, list(c0[key]), exp[key])
    if "n_selected0" in exp:
        assert int(c0["n_selected"][0]) == exp["n_selected0"], (who, list(c0["n_selected"]))
    if exp.get("unchanged"):
        assert np.array_equal(bits(R_out), bits(R_in)), who
    both = np.concatenate([rb, lb])
    for entry, axis in exp.get("pushed", ()):
        assert both[entry] & (1 << axis), (who, entry, axis)


def check_seams(info, rb, lb, who):
    """selected z entries of call 0 on both sides of the record / line seam and next to every chunk boundary inside the frame"""
    both = np.concatenate([rb, lb])
    sel = (both & 4) != 0
    assert int(info["call"][0]["n_selected"][2]) == int(sel.sum()), who          # nothing pushed and dropped
    assert sel[:len(rb)].any() and sel[len(rb):].any(), who
    for B in range(S.MF_CHUNK, len(both), S.MF_CHUNK):
        assert sel[B - 1] and sel[B], (who, B)
        assert sel[B - 64:B].sum() > 8 and sel[:B].sum() > 64, (who, B)


_REPLAY = {}


def scenario_replay(O, sc):
    """(per call the replayed frames, the restatement's hits) of a Manhattan scenario on the oracle's records, computed once"""
    if sc["name"] not in _REPLAY:
        recs = [oracle_normals(O, S.to_metres(d), sc["cam"].K4, S.MAXD)[2] for d in sc["depth"]]
        assert len(recs[0]) == S.n_records(sc["cam"].w, sc["cam"].h)
        hits = collections.Counter()
        _REPLAY[sc["name"]] = ([replay(recs, call, hits) for call in sc["calls"]], hits)
    return _REPLAY[sc["name"]]


@pytest.mark.parametrize("name", MANHATTAN)
def test_manhattan_scenario_reaches_what_it_names(oracle_mod, name):
    sc = S.manhattan_scenarios()[MANHATTAN.index(name)]
    results, hits = scenario_replay(oracle_mod, sc)
    boundaries = 0
    for ci, (call, res) in enumerate(zip(sc["calls"], results)):
        for f, (R_in, R_out, info, rb, lb) in enumerate(res):
            check_expect(call["expect"].get(f, {}), R_in, R_out, info, rb, lb, (name, ci, f))
            if sc.get("seams"):
                check_seams(info, rb, lb, (name, ci, f))
                boundaries += (len(rb) + len(lb) - 1) // S.MF_CHUNK
    for case in sc["hits"]:
        assert hits[case] > 0, case
    if sc.get("seams"):
        tot = [S.n_records(sc["cam"].w, sc["cam"].h) + int(c) for c in np.diff(sc["calls"][0]["loff"])]
        assert boundaries and tot[1] % S.MF_CHUNK == 0 and tot[0] == tot[1] - 1 and tot[2] == tot[1] + 1


def test_every_branch_the_issue_names_is_reached(oracle_mod):
    """the union over all scenarios: masks 1, 2, 4, 3, 6, 5, 7, det_flip, svd_zero_singular_value, zero_lambda_dropped, deficiency"""
    hits = collections.Counter()
    masks = set()
    for sc in S.manhattan_scenarios():
        results, h = scenario_replay(oracle_mod, sc)
        hits.update(h)
        for res in results:
            for _, _, info, _, _ in res:
                masks |= {int(c["found"]) for c in info["call"][:int(info["n_calls"])]}
    assert masks >= {0, 1, 2, 4, 3, 6, 5, 7}
    for case in ("found_0", "found_1", "pair_3", "pair_6", "pair_5", "found_3", "det_flip", "svd_zero_singular_value",
                 "zero_lambda_dropped", "deficiency", "nan_records", "lines_in_cone", "lines_outside_cone"):
        assert hits[case] > 0, case
