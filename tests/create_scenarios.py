"""Hand-built stores for map-point and map-line creation with hand-written results, the bridge between an
insert_numpy.Store and a LocalMap store, and seeded worlds.

The key frames, ranks and scales are insert_scenarios': 10, 20, 30, 40 with the ranks 1, 2, 3, 4, rows of 8 points and 4 lines,
(20, 3) a stereo keypoint, the camera centre of key frame h at (h / 10, 0, 0), the scales 1, 1.25, 1.5.  The keypoint at index i
of every key frame has the octave i % 3.  Stored points are 100.., stored lines 500.., created points 200.., created lines 600...
Every scenario returns (store, points, lines, expect): expect holds the displaced handles, facts about the store after the call
and the records, all worked out by hand from the reference's lines."""
import numpy as np

import create_numpy as cn
import fuse_scenarios as fs
import insert_scenarios as ins
from insert_numpy import POINT, LINE, Store

f32 = np.float32


def base():
    w = ins.base()
    for k in w.kfs.values():
        k["octave"] = [i % 3 for i in range(8)]
    return w


def pt(handle, obs, ref=None, world=(0.0, 0.0, 4.0), first_kf=7):
    return dict(handle=handle, obs=list(obs), ref_kf=obs[0][0] if ref is None else ref, first_kf=first_kf, world=world)


def ln(handle, obs, ref=None, first_kf=7):
    return dict(handle=handle, obs=list(obs), ref_kf=obs[0][0] if ref is None else ref, first_kf=first_kf)


# ---- the bridge to a store ----

def load(lm, w, geometry=True):
    """insert_scenarios.load with the octaves of the world"""
    ins.load(lm, w, geometry)
    root = min(w.kfs, key=lambda h: w.kfs[h]["rank"])

    def fit(h, v):
        return v[:-1] if w.cull_fit.get(h) is False else v
    lm.set_cull_attributes(
        kfs=[dict(handle=h, th_depth=40.0, flags=2 if h == root else 0, octave=fit(h, list(k.get("octave", [0] * len(k["stereo"])))),
                  depth=fit(h, [1.0] * len(k["stereo"])), stereo=fit(h, list(k["stereo"]))) for h, k in w.kfs.items()], points=[])
    stamped = [h for h, g in w.geo.items() if g.get("by") or g.get("by_ref")]
    if geometry and stamped:
        lm.set_point_geometry([dict(handle=h, world=w.geo[h]["world"], ref_kf=w.geo[h]["ref_kf"], ref_level=w.geo[h]["ref_level"],
                                    corrected_by=w.geo[h].get("by", 0), corrected_ref=w.geo[h].get("by_ref", 0)) for h in stamped])


def push_rows(lm, w, handles):
    """the match rows of these key frames into a store through drfe_lmap_set_keyframes, with the graph the store holds for them
    (the neighbours are the head of the ordered connections, as a connect or a cull leaves them), and their attributes"""
    g = lm.get_connections(handles)
    lm.set_keyframes([dict(handle=h, rank=w.kfs[h]["rank"], bad=w.kfs[h]["bad"], points=w.kfs[h]["rows"][POINT],
                           lines=w.kfs[h]["rows"][LINE], parent=int(g["parent"][i]), children=g["children"][i],
                           neighbours=g["ordered"][i][:10, 0] if len(g["ordered"][i]) else ()) for i, h in enumerate(handles)])
    root = min(w.kfs, key=lambda h: w.kfs[h]["rank"])
    lm.set_cull_attributes(kfs=[dict(handle=h, th_depth=40.0, flags=2 if h == root else 0,
                                     octave=list(w.kfs[h].get("octave", [0] * len(w.kfs[h]["stereo"]))),
                                     depth=[1.0] * len(w.kfs[h]["stereo"]), stereo=w.kfs[h]["stereo"]) for h in handles], points=[])


def by_setters(lm, w, points, lines):
    """the items `points` and `lines` (handles) of the world into a store the way a caller did it before the create entry: the
    five setters"""
    touched = sorted(set(k for kind, hs in ((POINT, points), (LINE, lines)) for h in hs for k, _ in w.items[kind][h]["obs"]) |
                     set(h for h, k in w.kfs.items() if set(k["rows"][POINT]) & set(points) or set(k["rows"][LINE]) & set(lines)))
    if points:
        lm.set_points([dict(handle=h, bad=0, obs=[k for k, _ in w.items[POINT][h]["obs"]]) for h in points])
    if lines:
        lm.set_lines(list(lines), [0] * len(lines))
    push_rows(lm, w, touched)
    if points:
        lm.set_point_geometry([dict(handle=h, world=w.geo[h]["world"], ref_kf=w.geo[h]["ref_kf"], ref_level=w.geo[h]["ref_level"])
                               for h in points])
        lm.set_cull_attributes(kfs=[], points=[dict(handle=h, n_obs=w.items[POINT][h]["n_obs"],
                                                    obs_index=[i for _, i in w.items[POINT][h]["obs"]]) for h in points])
    lm.set_recent_attributes(
        points=[dict(handle=h, found=1, visible=1, first_kf=w.items[POINT][h]["first_kf"]) for h in points],
        lines=[dict(handle=h, found=1, visible=1, first_kf=w.items[LINE][h]["first_kf"], n_obs=w.items[LINE][h]["n_obs"],
                    obs=[k for k, _ in w.items[LINE][h]["obs"]], obs_index=[i for _, i in w.items[LINE][h]["obs"]]) for h in lines])


def state_of_world(w):
    st = fs.state_of_world(w)
    st["first"] = {(kind, h): it["first_kf"] for kind in (POINT, LINE) for h, it in w.items[kind].items()}
    st["geo"] = {h: (g["world"].tobytes(), g["ref_kf"], g["ref_level"], g.get("by", 0), g.get("by_ref", 0))
                 for h, g in w.geo.items() if h in w.items[POINT]}
    return st


def state_of_store(lm, w):
    """every getter of the store: rows, flags, observers with indices, nObs, counters, mnFirstKFid, mpReplaced, geometry, and
    that a point has no adjustment state"""
    st = ins.state_of_store(lm, w)
    ph, lh = sorted(w.items[POINT]), sorted(w.items[LINE])
    rec = lm.get_recent_attributes(point_handles=ph, line_handles=lh)
    st["first"] = {(POINT, h): int(rec["points"][i]["first_kf"]) for i, h in enumerate(ph)}
    st["first"].update({(LINE, h): int(rec["lines"][i]["first_kf"]) for i, h in enumerate(lh)})
    gh = sorted(h for h in w.geo if h in w.items[POINT])
    st["geo"] = {}
    if gh:
        g = lm.get_point_geometry(gh)
        st["geo"] = {h: (g["world"][i].tobytes(), int(g["ref_kf"][i]), int(g["ref_level"][i]), int(g["corrected_by"][i]),
                         int(g["corrected_ref"][i])) for i, h in enumerate(gh)}
    return st


def same_state(got, want):
    ins.same_state(got, want)
    assert set(got["items"]) == set(want["items"])
    assert got["first"] == want["first"]
    assert got["geo"] == want["geo"]


def same_result(got, want, normals=True):
    """a LocalMap.create result against a create_numpy.create result: the floats bit for bit"""
    for name in ("point_displaced", "line_displaced"):
        assert [[int(v) for v in r] for r in got[name]] == [list(r) for r in want[name]], name
    if not normals:
        assert "normal" not in got
        return
    m = len(want["point_displaced"])
    assert len(got["status"]) == m and [int(s) for s in got["status"]] == list(want["status"])
    if m:
        assert np.array_equal(got["normal"].view(np.uint32), np.stack(want["normal"]).astype(f32).view(np.uint32)), "normal"
        for name in ("max_distance", "min_distance"):
            assert np.array_equal(got[name].view(np.uint32), np.array(want[name], f32).view(np.uint32)), name


def same_results(a, b):
    """two LocalMap.create results, byte for byte"""
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def check_expect(r, state, expect):
    for name in ("point_displaced", "line_displaced"):
        if name in expect:
            assert [[int(v) for v in x] for x in r[name]] == expect[name], name
    for (kind, h), obs in expect.get("obs", {}).items():
        assert state["items"][(kind, h)]["obs"] == obs, (kind, h)
        assert state["items"][(kind, h)]["bad"] == 0 and state["items"][(kind, h)]["replaced"] == -1
        assert state["items"][(kind, h)]["found"] == 1 or h < 200
    for (kind, h), n in expect.get("n_obs", {}).items():
        assert state["items"][(kind, h)]["n_obs"] == n, (kind, h)
    for (kf, kind, i), h in expect.get("rows", {}).items():
        assert state["rows"][(kf, kind)][i] == h, (kf, kind, i)
    for h, lv in expect.get("level", {}).items():
        assert state["geo"][h][2] == lv, h
    for h, ref in expect.get("ref", {}).items():
        assert state["geo"][h][1] == ref and state["first"][(POINT, h)] == 7, h
    if expect.get("nan_normal"):
        assert np.isnan(np.asarray(r["normal"])).all()
    if "max_distance" in expect:
        assert [float(v) for v in r["max_distance"]] == expect["max_distance"]
        assert [float(v) for v in r["min_distance"]] == expect["min_distance"]


def dist_pair(d2, scale):
    """max and min distance of a point whose squared distance to the reference centre is d2, at a level of that scale"""
    mx = f32(f32(np.sqrt(np.float64(d2))) * f32(scale))
    return float(mx), float(f32(mx / f32(1.5)))


# ---- the scenarios ----

def descending_rank():
    """the observations are given as (30, 1), (10, 2): the stored list is in rank order, 10 first.  The reference key frame 30 is
    at (3, 0, 0), 5 from the point (0, 0, 4); the keypoint (30, 1) has the octave 1, scale 1.25.  (With two observers a float sum
    from zero is the same in either order; the list order is what shows.)"""
    w = base()
    mx, mn = dist_pair(25.0, 1.25)
    return w, [pt(200, [(30, 1), (10, 2)])], [], dict(
        point_displaced=[[-1, -1]], obs={(POINT, 200): [(10, 2), (30, 1)]}, n_obs={(POINT, 200): 2},
        rows={(30, POINT, 1): 200, (10, POINT, 2): 200}, level={200: 1}, ref={200: 30}, max_distance=[mx], min_distance=[mn], stale=0)


def one_observer():
    """CreateNewKeyFrame's and StereoInitialization's form: (20, 4) has the octave 1; the centre (2, 0, 0) is sqrt(20) away"""
    w = base()
    mx, mn = dist_pair(20.0, 1.25)
    return w, [pt(200, [(20, 4)])], [], dict(
        point_displaced=[[-1, -1]], obs={(POINT, 200): [(20, 4)]}, n_obs={(POINT, 200): 1}, rows={(20, POINT, 4): 200},
        level={200: 1}, max_distance=[mx], min_distance=[mn], stale=0)


def stereo_entries():
    """nObs 2 (one stereo observer), 3 (a stereo and a mono one), 4 (two stereo ones)"""
    w = base()
    w.kfs[20]["stereo"] = [0, 0, 0, 1, 1, 1, 0, 0]
    w.kfs[30]["stereo"][3] = 1
    return w, [pt(200, [(20, 3)]), pt(201, [(20, 4), (10, 0)]), pt(202, [(20, 5), (30, 3)])], [], dict(
        n_obs={(POINT, 200): 2, (POINT, 201): 3, (POINT, 202): 4},
        obs={(POINT, 201): [(10, 0), (20, 4)], (POINT, 202): [(20, 5), (30, 3)]}, stale=0)


def both_on_one_keyframe():
    """two observations on key frame 20: the second is no observer, both row entries are written; the octave is the first's"""
    w = base()
    return w, [pt(200, [(20, 1), (20, 6)])], [], dict(
        point_displaced=[[-1, -1]], obs={(POINT, 200): [(20, 1)]}, n_obs={(POINT, 200): 1},
        rows={(20, POINT, 1): 200, (20, POINT, 6): 200}, level={200: 1}, stale=0)


def occupied_entry():
    """(20, 2) holds point 100: it is displaced and reported, and keeps its observation of 20 and its nObs"""
    w = base()
    ins.point(w, 100, [(10, 0), (20, 2)])
    return w, [pt(200, [(20, 2), (30, 0)])], [], dict(
        point_displaced=[[100, -1]], obs={(POINT, 200): [(20, 2), (30, 0)], (POINT, 100): [(10, 0), (20, 2)]},
        n_obs={(POINT, 100): 2, (POINT, 200): 2}, rows={(20, POINT, 2): 200, (10, POINT, 0): 100}, stale=0)


def two_on_one_entry():
    """two creations name (20, 0): the later holds the row and reports the earlier, which keeps its observation"""
    w = base()
    return w, [pt(200, [(20, 0)]), pt(201, [(20, 0), (30, 0)])], [], dict(
        point_displaced=[[-1, -1], [200, -1]], obs={(POINT, 200): [(20, 0)], (POINT, 201): [(20, 0), (30, 0)]},
        n_obs={(POINT, 200): 1, (POINT, 201): 2}, rows={(20, POINT, 0): 201, (30, POINT, 0): 201}, stale=0)


def reference_second():
    """the monocular initialisation: the reference key frame 40 is the second observation; (40, 5) has the octave 2, and the centre
    (4, 0, 0) is sqrt(32) from the point"""
    w = base()
    mx, mn = dist_pair(32.0, 1.5)
    return w, [pt(200, [(10, 5), (40, 5)], ref=40)], [], dict(
        obs={(POINT, 200): [(10, 5), (40, 5)]}, level={200: 2}, ref={200: 40}, max_distance=[mx], min_distance=[mn], stale=0)


def point_at_a_centre():
    """the point lies in the camera centre of key frame 20: cv::norm is 0, the scale inf, 0 * inf = NaN in every component, and
    the NaN stays through the sum"""
    w = base()
    return w, [pt(200, [(20, 0), (10, 0)], ref=10, world=(2.0, 0.0, 0.0))], [], dict(nan_normal=True, max_distance=[1.0],
                                                                                      min_distance=[float(f32(1.0) / f32(1.5))], stale=0)


def lines_alone():
    """a line's nObs grows by 1 per observer, at the stereo index (20, 3) too; stored list in rank order; an occupied entry"""
    w = base()
    w.add_item(LINE, 500, [(10, 0)])
    return w, [], [ln(600, [(30, 1), (10, 0)]), ln(601, [(20, 3)]), ln(602, [(40, 2), (40, 3)])], dict(
        line_displaced=[[-1, 500], [-1, -1], [-1, -1]],
        obs={(LINE, 600): [(10, 0), (30, 1)], (LINE, 601): [(20, 3)], (LINE, 602): [(40, 2)], (LINE, 500): [(10, 0)]},
        n_obs={(LINE, 600): 2, (LINE, 601): 1, (LINE, 602): 1, (LINE, 500): 1},
        rows={(10, LINE, 0): 600, (30, LINE, 1): 600, (20, LINE, 3): 601, (40, LINE, 2): 602, (40, LINE, 3): 602}, stale=0)


def both_kinds():
    """points and lines in one call, behind stored items of both kinds"""
    w = base()
    ins.point(w, 100, [(10, 0)])
    w.add_item(LINE, 500, [(10, 0)])
    return w, [pt(200, [(20, 0), (10, 1)]), pt(205, [(30, 2)])], [ln(600, [(20, 0), (10, 1)])], dict(
        point_displaced=[[-1, -1], [-1, -1]], line_displaced=[[-1, -1]],
        obs={(POINT, 200): [(10, 1), (20, 0)], (POINT, 205): [(30, 2)], (LINE, 600): [(10, 1), (20, 0)]}, stale=0)


def empty_call():
    w = base()
    ins.point(w, 100, [(10, 0)])
    return w, [], [], dict(point_displaced=[], line_displaced=[], stale=0)


def handle_below_the_stored():
    """point 50 is below the stored 100: no slot at the end.  The call is as correct, and leaves the image to the next call"""
    w = base()
    ins.point(w, 100, [(10, 0)])
    return w, [pt(50, [(20, 0), (10, 0)])], [], dict(
        point_displaced=[[-1, 100]], obs={(POINT, 50): [(10, 0), (20, 0)], (POINT, 100): [(10, 0)]}, rows={(10, POINT, 0): 50}, stale=1)


def handles_descending():
    """201 before 200: not ascending in call order"""
    w = base()
    return w, [pt(201, [(20, 0)]), pt(200, [(20, 1)])], [ln(600, [(10, 0)])], dict(
        obs={(POINT, 200): [(20, 1)], (POINT, 201): [(20, 0)]}, stale=1)


SCENARIOS = (descending_rank, one_observer, stereo_entries, both_on_one_keyframe, occupied_entry, two_on_one_entry, reference_second,
             point_at_a_centre, lines_alone, both_kinds, empty_call, handle_below_the_stored, handles_descending)


# ---- the refusals: (name, store, points, lines, normals, code, a word of the message) ----

def refusals():
    w = base()
    ins.point(w, 100, [(10, 0)])
    w.add_item(LINE, 500, [(10, 0)])
    out = [("stored_handle", w, [pt(100, [(20, 0)])], [], True, cn.ERR_INVALID, "map point 100"),
           ("stored_line_handle", w, [], [ln(500, [(20, 0)])], True, cn.ERR_INVALID, "map line 500"),
           ("handle_twice", w, [pt(200, [(20, 0)]), pt(200, [(20, 1)])], [], True, cn.ERR_INVALID, "twice"),
           ("unknown_keyframe", w, [pt(200, [(20, 0), (77, 0)])], [], True, cn.ERR_INVALID, "77"),
           ("index_outside_the_row", w, [pt(200, [(20, 8)])], [], True, cn.ERR_INVALID, "index 8"),
           ("line_index_outside_the_row", w, [], [ln(600, [(20, 4)])], True, cn.ERR_INVALID, "index 4"),
           ("negative_index", w, [pt(200, [(20, -1)])], [], True, cn.ERR_INVALID, "index -1"),
           ("no_observation", w, [pt(200, [], ref=20)], [], True, cn.ERR_INVALID, "observations"),
           ("three_observations", w, [pt(200, [(10, 1), (20, 1), (30, 1)])], [], True, cn.ERR_INVALID, "observations"),
           ("reference_not_an_observer", w, [pt(200, [(10, 1), (20, 1)], ref=30)], [], True, cn.ERR_INVALID, "reference"),
           # refused at the second creation: the first one is not kept either
           ("second_creation_refused", w, [pt(200, [(20, 0)]), pt(201, [(77, 0)])], [ln(600, [(10, 1)])], True, cn.ERR_INVALID, "77")]
    v = w.clone()
    v.cull_fit[20] = False
    out.append(("keyframe_attributes_do_not_fit", v, [pt(200, [(10, 1), (20, 1)])], [], False, cn.ERR_STATE, "key frame 20"))
    v = w.clone()
    v.scales = []
    out.append(("no_scales", v, [pt(200, [(20, 0)])], [], True, cn.ERR_STATE, "scales"))
    v = w.clone()
    del v.poses[10]
    out.append(("observer_without_pose", v, [pt(200, [(20, 0), (10, 1)])], [], True, cn.ERR_STATE, "observer 10"))
    v = w.clone()
    v.kfs[20]["octave"][0] = 3
    out.append(("octave_outside_the_scales", v, [pt(200, [(20, 0)])], [], True, cn.ERR_STATE, "octave 3"))
    return out


# ---- seeded worlds ----

def random_world(rng, **kw):
    """insert_scenarios.random_world with an octave per keypoint, inside its four scales"""
    w = ins.random_world(rng, **kw)
    for k in w.kfs.values():
        k["octave"] = [int(v) for v in rng.integers(0, 4, len(k["stereo"]))]
    return w


def random_creations(rng, w, n_points, n_lines, first_point=None, first_line=None, two=None):
    """creations on random entries of the world, occupied or not, now and then two on one entry or on one key frame; the handles
    ascend from above the stored ones unless first_* says otherwise.  two: None mixes 1 and 2 observers, else that many"""
    kfs = sorted(w.kfs)
    out = {}
    for kind, n, first in ((POINT, n_points, first_point), (LINE, n_lines, first_line)):
        h = (max(w.items[kind], default=99 if kind == POINT else 499) + 1) if first is None else first
        row = len(w.kfs[kfs[0]]["rows"][kind])
        made, out[kind] = [], []
        for t in range(n):
            m = int(rng.integers(1, 3)) if two is None else two
            ks = [int(k) for k in rng.choice(kfs, m, replace=rng.random() < 0.1)]
            obs = [(k, int(rng.integers(0, row))) for k in ks]
            if made and rng.random() < 0.15:
                obs[0] = made[int(rng.integers(0, len(made)))]
                if len(obs) == 2 and obs[1][0] == obs[0][0] and rng.random() < 0.5:
                    obs = obs[:1]
            made.extend(obs)
            c = dict(handle=h + t, obs=obs, ref_kf=obs[int(rng.integers(0, len(obs)))][0], first_kf=int(rng.integers(0, 1 << 40)))
            if kind == POINT:
                c["world"] = [float(v) for v in rng.integers(-16, 17, 3) / 2.0 + 0.125]
            out[kind].append(c)
    return out[POINT], out[LINE]
