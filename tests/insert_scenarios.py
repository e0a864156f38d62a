"""Hand-built stores for the item loops of ProcessNewKeyFrame with hand-written results, the bridge between
an insert_numpy.Store and a LocalMap store, and seeded scripts that interleave the call with the other operations of the store.

Key frames 10, 20, 30, 40 have the ranks 1, 2, 3, 4 - except where a scenario says otherwise - rows of 8 points and 4 lines, and
(20, 3) is a stereo keypoint.  Key frame h has the camera centre (h / 10, 0, 0); the scales are 1, 1.25, 1.5.  Points are 100..,
lines 500...  A row entry is written with put(): the key frame names the item, the item does not observe the key frame yet - that
is the state ProcessNewKeyFrame meets.  Every scenario returns (store, handles, expect): expect holds the actions, lists and facts
about the store after the call, all worked out by hand from the reference's loops."""
import numpy as np

import fuse_scenarios as fs
import insert_numpy as inp
from insert_numpy import POINT, LINE, NULL, BAD, RECENT, ADDED, Store

SCALES = [1.0, 1.25, 1.5]


def base(ranks=((10, 1), (20, 2), (30, 3), (40, 4))):
    w = Store()
    w.scales = list(SCALES)
    for h, rank in ranks:
        w.add_kf(h, rank, 8, 4, stereo=[0, 0, 0, 1 if h == 20 else 0, 0, 0, 0, 0])
        w.set_pose(h, (h / 10.0, 0.0, 0.0))
    return w


def point(w, h, obs, world=(0.0, 0.0, 4.0), ref=None, level=0, **kw):
    w.add_item(POINT, h, obs, **kw)
    w.set_geo(h, world, obs[0][0] if ref is None and obs else ref, level)


def put(w, kind, kf, idx, item):
    w.kfs[kf]["rows"][kind][idx] = item


# ---- the bridge to a store ----

def load(lm, w, geometry=True):
    """fuse_scenarios.load without the pieces the world marks as missing, then the geometry"""
    root = min(w.kfs, key=lambda h: w.kfs[h]["rank"])
    lm.set_keyframes([dict(handle=h, rank=k["rank"], bad=k["bad"], points=k["rows"][POINT], lines=k["rows"][LINE],
                           parent=-1 if h == root else root, children=[c for c in w.kfs if c != root] if h == root else [])
                      for h, k in w.kfs.items()])
    pts, lns = w.items[POINT], w.items[LINE]
    if pts:
        lm.set_points([dict(handle=h, bad=p["bad"], obs=[k for k, _ in p["obs"]]) for h, p in pts.items()])
    if lns:
        lm.set_lines(list(lns), [l["bad"] for l in lns.values()])

    def fit(h, v):
        return v[:-1] if w.cull_fit.get(h) is False else v
    lm.set_cull_attributes(
        kfs=[dict(handle=h, th_depth=40.0, flags=2 if h == root else 0, octave=fit(h, [0] * len(k["stereo"])),
                  depth=fit(h, [1.0] * len(k["stereo"])), stereo=fit(h, list(k["stereo"]))) for h, k in w.kfs.items()],
        points=[dict(handle=h, n_obs=p["n_obs"], obs_index=[i for _, i in p["obs"]]) for h, p in pts.items() if not p.get("no_cull")])
    lm.set_recent_attributes(
        points=[dict(handle=h, found=p["found"], visible=p["visible"], first_kf=p["first_kf"]) for h, p in pts.items()],
        lines=[dict(handle=h, found=l["found"], visible=l["visible"], first_kf=l["first_kf"], n_obs=l["n_obs"],
                    obs=[k for k, _ in l["obs"]], obs_index=[i for _, i in l["obs"]]) for h, l in lns.items() if not l.get("no_state")])
    if not geometry:
        return
    if w.scales:
        lm.set_scales(w.scales)
    if w.poses:
        lm.set_poses(list(w.poses), np.stack([w.poses[h] for h in w.poses]))
    if w.geo:
        lm.set_point_geometry([dict(handle=h, world=g["world"], ref_kf=g["ref_kf"], ref_level=g["ref_level"]) for h, g in w.geo.items()])


def state_of_world(w):
    return fs.state_of_world(w)


def state_of_store(lm, w):
    """the getters of the store, for the items that have every piece"""
    whole = Store()
    whole.kfs = w.kfs
    whole.items = {POINT: {h: p for h, p in w.items[POINT].items() if not p.get("no_cull")},
                   LINE: {h: l for h, l in w.items[LINE].items() if not l.get("no_state")}}
    return fs.state_of_store(lm, whole)


def same_state(got, want):
    assert got["rows"] == want["rows"]
    for key in got["items"]:
        assert got["items"][key] == want["items"][key], "item %s: %r != %r" % (key, got["items"][key], want["items"][key])


def same_result(got, want, normals=True):
    """a LocalMap.insert result against a Store.insert result: the floats bit for bit"""
    for name in ("point_action", "line_action"):
        assert [[int(a) for a in row] for row in got[name]] == [list(row) for row in want[name]], name
    for name in ("added_points", "added_lines"):
        assert [tuple(int(v) for v in r) for r in got[name]] == [tuple(r) for r in want[name]], name
    for name in ("recent_points", "recent_lines"):
        assert [int(v) for v in got[name]] == list(want[name]), name
    if not normals:
        return
    m = len(want["added_points"])
    assert len(got["status"]) == m and [int(s) for s in got["status"]] == list(want["status"])
    if m:
        assert np.array_equal(got["normal"].view(np.uint32), np.stack(want["normal"]).astype(np.float32).view(np.uint32)), "normal"
        for name in ("max_distance", "min_distance"):
            assert np.array_equal(got[name].view(np.uint32), np.array(want[name], np.float32).view(np.uint32)), name


def same_results(a, b):
    """two LocalMap.insert results, byte for byte"""
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], list):
            assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert a[k].tobytes() == b[k].tobytes(), k


def check_expect(r, state, expect):
    for name in ("point_action", "line_action"):
        if name in expect:
            assert [[int(a) for a in row] for row in r[name]] == expect[name], name
    for name in ("added_points", "added_lines"):
        if name in expect:
            assert [tuple(int(v) for v in x) for x in r[name]] == expect[name], name
    for name in ("recent_points", "recent_lines"):
        if name in expect:
            assert [int(v) for v in r[name]] == expect[name], name
    for (kind, h), obs in expect.get("obs", {}).items():
        assert state["items"][(kind, h)]["obs"] == obs, (kind, h)
    for (kind, h), n in expect.get("n_obs", {}).items():
        assert state["items"][(kind, h)]["n_obs"] == n, (kind, h)
    if expect.get("nan_normal"):
        assert np.isnan(r["normal"]).all()
    if "max_distance" in expect:
        assert [float(v) for v in r["max_distance"]] == expect["max_distance"]
        assert [float(v) for v in r["min_distance"]] == expect["min_distance"]


N8, N4 = [NULL] * 8, [NULL] * 4


def row(n, **at):
    r = [NULL] * n
    for k, v in at.items():
        r[int(k[1:])] = v
    return r


# ---- the scenarios ----

def null_bad_observing():
    """a null entry, a bad point, a point that already observes the key frame (at another index: IsInKeyFrame asks the map, not
    the index), and one that does not"""
    w = base()
    point(w, 100, [(10, 0)], bad=1)
    point(w, 101, [(10, 1), (20, 5)])
    point(w, 102, [(10, 2)])
    put(w, POINT, 20, 0, 100)
    put(w, POINT, 20, 2, 101)
    put(w, POINT, 20, 4, 102)
    return w, [20], dict(
        point_action=[row(8, i0=BAD, i2=RECENT, i4=ADDED, i5=RECENT)], line_action=[N4],
        added_points=[(102, 20, 4)], recent_points=[101, 101],
        obs={(POINT, 102): [(10, 2), (20, 4)], (POINT, 101): [(10, 1), (20, 5)], (POINT, 100): [(10, 0)]}, n_obs={(POINT, 102): 2})


def twice_in_a_row():
    """a point at two indices of one row: ADDED at the first, RECENT at the second, pushed once"""
    w = base()
    point(w, 100, [(10, 0)])
    put(w, POINT, 30, 6, 100)
    put(w, POINT, 30, 1, 100)
    return w, [30], dict(point_action=[row(8, i1=ADDED, i6=RECENT)], added_points=[(100, 30, 1)], recent_points=[100],
                         obs={(POINT, 100): [(10, 0), (30, 1)]}, n_obs={(POINT, 100): 2})


def two_and_three_callers():
    """point 100 in the rows of two called key frames, point 101 in three: every report covers one more observer.  The call order
    40, 20, 30 is not the rank order, so the second addition enters in front of the first."""
    w = base()
    point(w, 100, [(10, 0)])
    point(w, 101, [(10, 1)])
    for kf in (40, 20):
        put(w, POINT, kf, 2, 100)
    for kf in (40, 20, 30):
        put(w, POINT, kf, 5, 101)
    return w, [40, 20, 30], dict(
        point_action=[row(8, i2=ADDED, i5=ADDED), row(8, i2=ADDED, i5=ADDED), row(8, i5=ADDED)],
        added_points=[(100, 40, 2), (101, 40, 5), (100, 20, 2), (101, 20, 5), (101, 30, 5)], recent_points=[],
        obs={(POINT, 100): [(10, 0), (20, 2), (40, 2)], (POINT, 101): [(10, 1), (20, 5), (30, 5), (40, 5)]},
        n_obs={(POINT, 100): 3, (POINT, 101): 4})


def insertion_places():
    """the new observer 20 enters in front (of 30, 40), in the middle (between 10 and 40), at the end (after 10), and - in a
    stored list that is not in rank order - in front of the first greater one (40), not behind 10"""
    w = base()
    point(w, 100, [(30, 0), (40, 0)])
    point(w, 101, [(10, 1), (40, 1)])
    point(w, 102, [(10, 2)])
    point(w, 103, [(40, 3), (10, 3), (30, 3)])
    for i, p in enumerate((100, 101, 102, 103)):
        put(w, POINT, 20, i + 4, p)
    return w, [20], dict(
        point_action=[row(8, i4=ADDED, i5=ADDED, i6=ADDED, i7=ADDED)],
        obs={(POINT, 100): [(20, 4), (30, 0), (40, 0)], (POINT, 101): [(10, 1), (20, 5), (40, 1)], (POINT, 102): [(10, 2), (20, 6)],
             (POINT, 103): [(20, 7), (40, 3), (10, 3), (30, 3)]})


def unordered_two_adders():
    """two called key frames into a stored list that is not in rank order: 30 lands in front of 40, then 20 in front of 30"""
    w = base()
    point(w, 100, [(40, 0), (10, 0)])
    put(w, POINT, 30, 1, 100)
    put(w, POINT, 20, 1, 100)
    return w, [30, 20], dict(obs={(POINT, 100): [(20, 1), (30, 1), (40, 0), (10, 0)]})


def stereo_and_mono():
    """(20, 3) is a stereo keypoint: +2; (20, 4) is not: +1"""
    w = base()
    point(w, 100, [(10, 0)])
    point(w, 101, [(10, 1)])
    put(w, POINT, 20, 3, 100)
    put(w, POINT, 20, 4, 101)
    return w, [20], dict(n_obs={(POINT, 100): 3, (POINT, 101): 2})


def centre_on_the_point():
    """the point lies in the camera centre of its new observer: cv::norm is 0, the scale inf, 0 * inf = NaN in all three
    components, as OpenCV computes it"""
    w = base()
    point(w, 100, [(10, 0)], world=(2.0, 0.0, 0.0))
    put(w, POINT, 20, 0, 100)
    return w, [20], dict(added_points=[(100, 20, 0)], nan_normal=True)


def reference_is_the_called():
    """the reference key frame of the point is the called key frame itself: its stored centre is read twice.  The point (0, 0, 4)
    is sqrt(20) from the centre (2, 0, 0); level 2 scales by 1.5, and the last level divides by 1.5 again"""
    w = base()
    point(w, 100, [(10, 0)], ref=20, level=2)
    put(w, POINT, 20, 0, 100)
    return w, [20], dict(
        added_points=[(100, 20, 0)], max_distance=[float(np.float32(np.float32(np.sqrt(20.0)) * np.float32(1.5)))],
        min_distance=[float(np.float32(np.float32(np.float32(np.sqrt(20.0)) * np.float32(1.5)) / np.float32(1.5)))])


def lines_mirror():
    """the line row: null, bad, observing, twice in a row, two callers, the insertion rule; nObs grows by 1"""
    w = base()
    w.add_item(LINE, 500, [(10, 0)], bad=1)
    w.add_item(LINE, 501, [(10, 1), (20, 3)])
    w.add_item(LINE, 502, [(40, 2), (10, 2)])
    put(w, LINE, 20, 0, 500)
    put(w, LINE, 20, 1, 501)
    put(w, LINE, 20, 2, 502)
    put(w, LINE, 30, 0, 502)
    put(w, LINE, 30, 3, 502)
    return w, [30, 20], dict(
        point_action=[N8, N8], line_action=[[ADDED, NULL, NULL, RECENT], [BAD, RECENT, ADDED, RECENT]],
        added_lines=[(502, 30, 0), (502, 20, 2)], recent_lines=[502, 501, 501],
        obs={(LINE, 502): [(20, 2), (30, 0), (40, 2), (10, 2)], (LINE, 501): [(10, 1), (20, 3)]}, n_obs={(LINE, 502): 4})


def empty_call():
    w = base()
    point(w, 100, [(10, 0)])
    return w, [], dict(point_action=[], line_action=[], added_points=[], recent_points=[])


SCENARIOS = (null_bad_observing, twice_in_a_row, two_and_three_callers, insertion_places, unordered_two_adders, stereo_and_mono,
             centre_on_the_point, reference_is_the_called, lines_mirror, empty_call)


# ---- the refusals: (store, handles, normals, code) ----

def refusals():
    out = []
    w = base()
    point(w, 100, [(10, 0)])
    put(w, POINT, 20, 0, 100)
    out.append(("unknown_keyframe", w, [20, 77], True, inp.ERR_INVALID))
    out.append(("repeated_keyframe", w.clone(), [20, 30, 20], True, inp.ERR_INVALID))
    v = w.clone()
    v.cull_fit[20] = False
    out.append(("keyframe_attributes_do_not_fit", v, [20], False, inp.ERR_STATE))
    v = w.clone()
    v.items[POINT][100]["no_cull"] = True
    out.append(("point_without_attributes", v, [20], False, inp.ERR_STATE))
    v = w.clone()
    v.add_item(LINE, 500, [(10, 0)])
    v.items[LINE][500]["no_state"] = True
    put(v, LINE, 20, 0, 500)
    out.append(("line_without_state", v, [20], False, inp.ERR_STATE))
    v = w.clone()
    v.scales = []
    out.append(("no_scales", v, [20], True, inp.ERR_STATE))
    v = w.clone()
    del v.geo[100]
    out.append(("no_position", v, [20], True, inp.ERR_STATE))
    v = w.clone()
    del v.poses[10]
    v.geo[100]["ref_kf"] = 30
    out.append(("observer_without_pose", v, [20], True, inp.ERR_STATE))
    v = w.clone()
    del v.poses[20]
    v.geo[100]["ref_kf"] = 30
    out.append(("called_without_pose", v, [20], True, inp.ERR_STATE))
    v = w.clone()
    del v.poses[30]
    v.geo[100]["ref_kf"] = 30
    out.append(("reference_without_pose", v, [20], True, inp.ERR_STATE))
    v = w.clone()
    v.geo[100]["ref_kf"] = 99                                           # no stored key frame: the reference is -1 in the image
    out.append(("reference_not_stored", v, [20], True, inp.ERR_STATE))
    v = w.clone()
    v.geo[100]["ref_level"] = 3
    out.append(("level_out_of_range", v, [20], True, inp.ERR_STATE))
    # refused at the second key frame: the first one's additions are not kept either
    v = w.clone()
    point(v, 101, [(10, 1)])
    del v.geo[101]
    put(v, POINT, 30, 0, 101)
    out.append(("second_keyframe_refused", v, [20, 30], True, inp.ERR_STATE))
    return out


# ---- seeded worlds and scripts ----

def random_world(rng, n_kfs=12, n_points=60, n_lines=16, row=24, line_row=8):
    """key frames with shuffled ranks; items with stored observers in a random order (not the rank order); rows that name items
    the key frame is not an observer of yet - some of them twice, some bad, some in several rows"""
    w = Store()
    w.scales = [1.0, 1.2, 1.44, 1.728]
    handles = [10 * (k + 1) for k in range(n_kfs)]
    ranks = rng.permutation(n_kfs) + 1
    for h, r in zip(handles, ranks):
        w.add_kf(h, int(r), row, line_row, stereo=[int(v) for v in rng.integers(0, 2, row)])
        w.set_pose(h, [float(v) for v in rng.integers(-8, 9, 3) / 4.0])
    free = {(h, kind): list(rng.permutation(row if kind == POINT else line_row)) for h in handles for kind in (POINT, LINE)}
    for kind, first, count in ((POINT, 100, n_points), (LINE, 500, n_lines)):
        for i in range(count):
            ks = [int(k) for k in rng.choice(handles, int(rng.integers(0, 5)), replace=False)]
            obs = [(k, int(free[(k, kind)].pop())) for k in ks if free[(k, kind)]]
            bad = int(rng.random() < 0.1)
            if kind == POINT:
                point(w, first + i, obs, world=[float(v) for v in rng.integers(-16, 17, 3) / 2.0 + 0.125],
                      ref=int(rng.choice(handles)), level=int(rng.integers(0, 4)), bad=bad)
            else:
                w.add_item(LINE, first + i, obs, bad=bad)
    return w


def random_puts(rng, w, handles, share=0.5):
    """new row entries of the key frames `handles`: items they do not observe, now and then one twice, one they do observe"""
    for h in handles:
        for kind in (POINT, LINE):
            r = w.kfs[h]["rows"][kind]
            empty = [i for i, v in enumerate(r) if v < 0]
            items = sorted(w.items[kind])
            for i in empty:
                if rng.random() < share:
                    r[i] = int(rng.choice(items))


def push_rows(lm, w, handles):
    """the rows of these key frames into a store, as a caller does after tracking"""
    root = min(w.kfs, key=lambda h: w.kfs[h]["rank"])
    lm.set_keyframes([dict(handle=h, rank=w.kfs[h]["rank"], bad=w.kfs[h]["bad"], points=w.kfs[h]["rows"][POINT],
                           lines=w.kfs[h]["rows"][LINE], parent=-1 if h == root else root,
                           children=[c for c in w.kfs if c != root] if h == root else []) for h in handles])
    lm.set_cull_attributes(kfs=[dict(handle=h, th_depth=40.0, flags=2 if h == root else 0, octave=[0] * len(w.kfs[h]["stereo"]),
                                     depth=[1.0] * len(w.kfs[h]["stereo"]), stereo=w.kfs[h]["stereo"]) for h in handles], points=[])
