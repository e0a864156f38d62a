"""Hand-built stores for LocalMapping::MapPointCulling and MapLineCulling, one per rule kept from the reference
(src/LocalMapping.cc:175-231, MapPoint::SetBadFlag, MapLine::SetBadFlag), each with what it must return written out by hand, and
seeded random scripts.  Nothing here imports the library; the random scripts are grown on the restatement
(tests/recent_cull_numpy.py), which tells the generator what is still alive.

A script is a list of operations that play() runs on lib.LocalMap or on recent_cull_numpy.Store: those of cull_scenarios and
    ("recent", points, lines)  ("rcull", current_kf_id, points, lines, monocular)  ("inc", kind, handles, d_found, d_visible)
A scenario returns (script, expect, paths): expect has, per rcull of the script, the hand-written result by kind (action, kept,
culled, erased; a key that is left out is not compared); paths names the branches of recent_cull_numpy.PATHS that the scenario
was built to reach."""
import numpy as np

import cull_numpy as un
import cull_scenarios as us
import lmap_scenarios as ls
import recent_cull_numpy as rn

KEYFRAME, POINT, LINE = ls.KEYFRAME, ls.POINT, ls.LINE
CUR = 10                                        # mpCurrentKeyFrame->mnId of most scenarios


class World(us.World):
    """cull_scenarios.World plus map lines and the recent-list attributes.  rpoint / rline append the item to each observer's row
    and record the index; obs_of() is that record, in stored order."""

    def __init__(self):
        super().__init__()
        self.init_recent()

    def init_recent(self):
        self.lns, self.rpt, self.rln = {}, {}, {}
        return self

    def rpoint(self, kfs, found=1, visible=1, first=CUR, n_obs=None, bad=0, h=None):
        h = self.point([(k, 0) for k in kfs], n_obs=n_obs, bad=bad, h=h)
        self.rpt[h] = dict(handle=h, found=found, visible=visible, first_kf=first)
        return h

    def rline(self, kfs, found=1, visible=1, first=CUR, n_obs=None, bad=0, h=None):
        if h is None:
            h, self.next = self.next, self.next + 1
        idx = []
        for k in kfs:
            self.kfs[k]["lines"].append(h)
            idx.append(len(self.kfs[k]["lines"]) - 1)
        self.lns[h] = bad
        self.rln[h] = dict(handle=h, found=found, visible=visible, first_kf=first, n_obs=len(kfs) if n_obs is None else n_obs,
                           obs=list(kfs), obs_index=idx)
        return h

    def item(self, kind, *a, **kw):
        return (self.rpoint if kind == POINT else self.rline)(*a, **kw)

    def stale(self, kind, h, k, idx):
        """an observation alone: the item names index idx of k's row, whatever stands there"""
        if kind == POINT:
            self.observe(h, k, idx)
        else:
            self.rln[h]["obs"].append(k)
            self.rln[h]["obs_index"].append(idx)

    def obs_of(self, kind, h):
        if kind == POINT:
            return [[k, i] for k, i in zip(self.pts[h]["obs"], self.apt[h]["obs_index"])]
        return [[k, i] for k, i in zip(self.rln[h]["obs"], self.rln[h]["obs_index"])]

    def ops(self):
        out = super().ops()
        if self.lns:
            out.append(("lines", sorted(self.lns), [self.lns[h] for h in sorted(self.lns)]))
        out.append(("recent", [dict(r) for r in self.rpt.values()],
                    [dict(r, obs=list(r["obs"]), obs_index=list(r["obs_index"])) for r in self.rln.values()]))
        return out


def play(ops, store, mode="host"):
    """the results of the script's calls, in order"""
    out = []
    for op in ops:
        if op[0] == "recent":
            store.set_recent_attributes(op[1], op[2])
        elif op[0] == "rcull":
            out.append(store.recent_cull(op[1], op[2], op[3], monocular=op[4], mode=mode))
        elif op[0] == "inc":
            store.recent_increase(op[1], op[2], op[3], op[4])
        else:
            out += us.play([op], store, mode=mode)
    return out


def check(results, expect):
    calls = [r for r in results if "points" in r and "lines" in r]
    assert len(calls) == len(expect)
    for r, e in zip(calls, expect):
        for name, want in e.items():
            for k, v in want.items():
                got = [a.tolist() for a in r[name][k]] if k == "erased" else np.asarray(r[name][k]).tolist()
                assert got == v, (name, k, got, v)


def _base():
    """the key frames 1 .. 5 and the bad key frame 6; none is ever called, they only hold rows"""
    w = World()
    w.kf(1, 10, flags=un.ORIGIN, ch=[2, 3, 4, 5, 6])
    for h in (2, 3, 4, 5):
        w.kf(h, 10 * h, parent=1)
    w.kf(6, 60, parent=1, bad=1)
    return w


def _both_kinds(build):
    """a scenario that holds for points and for lines alike: build(w, kind) returns (list, expect of that kind)"""
    w = _base()
    lp, ep = build(w, POINT)
    ll, el = build(w, LINE)
    return w, lp, ll, dict(points=ep, lines=el)


def each_action():
    def build(w, kind):
        good = dict(found=3, visible=4)
        a = w.item(kind, [1, 2], bad=1, **good)
        b = w.item(kind, [1, 2], found=1, visible=5)                         # 0.2, and 1 / 5 == 0
        c = w.item(kind, [1, 2, 3], first=CUR - 2, **(good if kind == POINT else dict(found=4, visible=4)))
        d = w.item(kind, [1, 2, 3, 4], first=CUR - 3, **(good if kind == POINT else dict(found=4, visible=4)))
        e = w.item(kind, [1, 2], first=CUR - 1, **(good if kind == POINT else dict(found=4, visible=4)))
        return [a, b, c, d, e], dict(action=[1, 2, 3, 4, 0], kept=[e], culled=[b, c], erased=[w.obs_of(kind, b), w.obs_of(kind, c)])
    w, lp, ll, e = _both_kinds(build)
    return w.ops() + [("rcull", CUR, lp, ll, 0)], [e], ("was_bad", "point_ratio", "line_ratio", "culled_observations", "aged_out", "kept", "nulled_own")


def float_division_not_integers():
    """16777219 / 67108877 in float is exactly 0.25 (kept) while 4 * found < visible; 1 / 4 is kept, 1 / 5 is not"""
    w = _base()
    a = w.rpoint([1, 2], found=16777219, visible=67108877)
    b = w.rpoint([1, 2], found=1, visible=4)
    c = w.rpoint([1, 2], found=1, visible=5)
    e = dict(points=dict(action=[0, 0, 2], kept=[a, b], culled=[c], erased=[w.obs_of(POINT, c)]))
    return w.ops() + [("rcull", CUR, [a, b, c], [], 0)], [e], ("point_ratio_exactly_quarter", "point_ratio")


def visible_zero_points():
    """0 / 0 is NaN and 3 / 0 is inf: neither is less than 0.25"""
    w = _base()
    a = w.rpoint([1], found=0, visible=0)
    b = w.rpoint([1], found=3, visible=0)
    c = w.rpoint([1], found=-3, visible=0)                                    # -inf is less
    e = dict(points=dict(action=[0, 0, 2], kept=[a, b], culled=[c]))
    return w.ops() + [("rcull", CUR, [a, b, c], [], 0)], [e], ("point_ratio_nan", "point_ratio_inf")


def line_integer_division():
    """found < visible culls whatever the ratio; found == 3 * visible is 3"""
    w = _base()
    a = w.rline([1, 2], found=2, visible=3)
    b = w.rline([1, 2], found=6, visible=2)
    c = w.rline([1, 2], found=99, visible=100)
    d = w.rline([1, 2], found=0, visible=7)
    e = dict(lines=dict(action=[2, 0, 2, 2], kept=[b], culled=[a, c, d]))
    return w.ops() + [("rcull", CUR, [], [a, b, c, d], 0)], [e], ("line_ratio", "line_ratio_whole_multiple")


def first_kf_minus_one():
    """mnFirstKFid == -1 against the key frame 1: the difference is 2"""
    def build(w, kind):
        a = w.item(kind, [1, 2], first=-1)                                    # 2 observations: culled
        b = w.item(kind, [1, 2, 3, 4], first=-1)                              # 4: stays, 2 < 3
        return [a, b], dict(action=[3, 0], kept=[b], culled=[a])
    w, lp, ll, e = _both_kinds(build)
    return w.ops() + [("rcull", 1, lp, ll, 0)], [e], ("first_kf_negative", "culled_observations")


def ids_above_bit_31():
    """both ids are truncated to int: 2^32 + 5 against 5 is 0, 5 against 2^32 + 2 is 3"""
    def build(w, kind):
        a = w.item(kind, [1], first=5)                                        # age 0 at current 2^32 + 5
        return [a], dict(action=[0], kept=[a], culled=[])
    w, lp, ll, e1 = _both_kinds(build)
    b = w.rpoint([1, 2, 3, 4], first=(1 << 32) + 2)
    c = w.rline([1, 2, 3, 4], first=(1 << 32) + 2)
    e2 = dict(points=dict(action=[4], kept=[], culled=[]), lines=dict(action=[4], kept=[], culled=[]))
    return w.ops() + [("rcull", (1 << 32) + 5, lp, ll, 0), ("rcull", 5, [b], [c], 0)], [e1, e2], ("id_above_bit_31", "aged_out")


def _threshold(monocular):
    def build(w, kind):
        hs = [w.item(kind, [1, 2, 3, 4][:n], first=CUR - 2) for n in (2, 3, 4)]
        act = [3, 0, 0] if monocular else [3, 3, 0]
        return hs, dict(action=act, kept=[h for h, a in zip(hs, act) if a == 0], culled=[h for h, a in zip(hs, act) if a == 3])
    w, lp, ll, e = _both_kinds(build)
    return w.ops() + [("rcull", CUR, lp, ll, monocular)], [e], ("observations_at_threshold", "observations_above_threshold")


def observations_at_the_threshold():
    return _threshold(0)


def observations_at_the_threshold_monocular():
    return _threshold(1)


def handle_twice_first_culled():
    def build(w, kind):
        b = w.item(kind, [1, 2], found=1, visible=5)
        e = w.item(kind, [1, 2])
        return [b, e, b, b], dict(action=[2, 0, 1, 1], kept=[e], culled=[b], erased=[w.obs_of(kind, b)])
    w, lp, ll, e = _both_kinds(build)
    return w.ops() + [("rcull", CUR, lp, ll, 0)], [e], ("second_of_culled",)


def handle_twice_kept_and_aged():
    def build(w, kind):
        e = w.item(kind, [1, 2])
        d = w.item(kind, [1, 2, 3, 4], first=CUR - 3)
        return [e, d, e, d], dict(action=[0, 4, 0, 4], kept=[e, e], culled=[])
    w, lp, ll, e = _both_kinds(build)
    return w.ops() + [("rcull", CUR, lp, ll, 0)], [e], ("second_of_kept",)


def stale_index_nulls_a_live_item():
    """the culled item holds an observation whose index is where a live item stands; that item is kept later in the same list"""
    def build(w, kind):
        b = w.item(kind, [1], found=1, visible=5)
        e = w.item(kind, [1, 2])
        w.stale(kind, b, 2, w.obs_of(kind, e)[1][1])
        return [b, e], dict(action=[2, 0], kept=[e], culled=[b], erased=[w.obs_of(kind, b)])
    w, lp, ll, e = _both_kinds(build)
    return w.ops() + [("rcull", CUR, lp, ll, 0)], [e], ("nulled_other",)


def two_culled_items_name_one_entry():
    def build(w, kind):
        a = w.item(kind, [1, 2], found=1, visible=5)
        b = w.item(kind, [3], found=1, visible=5)
        w.stale(kind, b, 1, w.obs_of(kind, a)[0][1])
        return [a, b], dict(action=[2, 2], kept=[], culled=[a, b], erased=[w.obs_of(kind, a), w.obs_of(kind, b)])
    w, lp, ll, e = _both_kinds(build)
    return w.ops() + [("rcull", CUR, lp, ll, 0)], [e], ("nulled_already_null",)


def bad_observer_and_no_observations():
    def build(w, kind):
        a = w.item(kind, [6, 1], found=1, visible=5)                          # key frame 6 is bad
        b = w.item(kind, [], found=1, visible=5)
        return [a, b], dict(action=[2, 2], kept=[], culled=[a, b], erased=[w.obs_of(kind, a), []])
    w, lp, ll, e = _both_kinds(build)
    return w.ops() + [("rcull", CUR, lp, ll, 0)], [e], ("bad_observer", "no_observations")


HAND = {f.__name__: f for f in (
    each_action, float_division_not_integers, visible_zero_points, line_integer_division, first_kf_minus_one, ids_above_bit_31,
    observations_at_the_threshold, observations_at_the_threshold_monocular, handle_twice_first_culled, handle_twice_kept_and_aged,
    stale_index_nulls_a_live_item, two_culled_items_name_one_entry, bad_observer_and_no_observations)}


def random_world(rng, n_kf=16, n_pt=180, n_ln=60):
    """cull_scenarios' random world, recent-list attributes for every point, and lines seen by 0 .. 5 key frames"""
    w = us.random_world(rng, n_kf, n_pt)
    w.__class__ = World
    w.init_recent()
    draw = lambda: dict(found=int(rng.integers(0, 12)), visible=int(rng.integers(0 if rng.random() < 0.1 else 1, 12)),
                        first=int(rng.integers(CUR - 5, CUR + 1)))
    for h in sorted(w.pts):
        a = draw()
        w.rpt[h] = dict(handle=h, found=a["found"], visible=a["visible"], first_kf=a["first"])
    for _ in range(n_ln):
        a = draw()
        kfs = [int(k) for k in rng.permutation(np.arange(1, n_kf + 1))[:int(rng.integers(0, 6))]]
        h = w.rline(kfs, found=a["found"], visible=max(1, a["visible"]), first=a["first"], bad=int(rng.random() < 0.1))
        if kfs and rng.random() < 0.2:                                        # a stale index into another key frame's row
            others = [k for k in range(1, n_kf + 1) if k not in kfs and w.kfs[k]["lines"]]
            if others:
                k = int(rng.choice(others))
                w.stale(LINE, h, k, int(rng.integers(0, len(w.kfs[k]["lines"]))))
    return w


def random_script(seed, calls=5, per_list=40):
    """a world, then recent-list calls (with duplicates) interleaved with updates, connects, key-frame culls, counter edits and a
    set_bad; grown on the restatement"""
    rng = np.random.default_rng(seed)
    w = random_world(rng)
    n_kf = len(w.kfs)
    ops = w.ops()
    ref = rn.Store()
    play(ops, ref)

    def emit(op):
        ops.append(op)
        return play([op], ref)

    def draw(table, k):
        hs = [int(h) for h in rng.choice(sorted(table), size=min(k, len(table)), replace=False)]
        hs += [int(h) for h in rng.choice(hs, size=max(1, len(hs) // 8))]     # pushed once per row index
        return [int(h) for h in rng.permutation(hs)]

    for c in range(calls):
        emit(("rcull", CUR + c, draw(ref.mp, per_list), draw(ref.ml, per_list // 2), int(c == 2)))
        kind = c % 5
        live = [h for h in range(2, n_kf + 1) if not ref.kf[h].bad]
        if kind == 0:
            emit(("update", [dict(frame_id=100 + c, points=[int(p) for p in rng.choice(sorted(ref.mp), size=40, replace=False)],
                                  lines=[int(p) for p in rng.choice(sorted(ref.ml), size=20, replace=False)])]))
        elif kind == 1 and live:
            emit(("connect", [int(h) for h in rng.permutation(live)[:4]]))
        elif kind == 2 and live:
            emit(("cull", [int(h) for h in rng.permutation(live)[:6]], 0))
        elif kind == 3:
            hs = [int(h) for h in rng.choice(sorted(ref.rec_mp), size=30)]
            emit(("inc", POINT, hs, [int(v) for v in rng.integers(0, 3, 30)], [int(v) for v in rng.integers(0, 3, 30)]))
            ok = [h for h in sorted(ref.rec_ml) if not ref.ml[h].bad]
            hs = [int(h) for h in rng.choice(ok, size=10)]
            emit(("inc", LINE, hs, [int(v) for v in rng.integers(1, 3, 10)], [0] * 10))
        elif kind == 4:
            p = int(rng.choice([q for q in sorted(ref.mp) if not ref.mp[q].bad]))
            emit(("bad", POINT, [p], [1]))
    return ops
