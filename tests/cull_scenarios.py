"""Hand-built graphs for LocalMapping::KeyFrameCulling and KeyFrame::SetBadFlag, one per rule kept from the reference
(src/LocalMapping.cc:1226-1285, src/KeyFrame.cc:574-705, src/MapPoint.cc:145-202), each with what it must return written out by
hand, and seeded random scripts.  Nothing here imports the library; the random scripts are grown on the restatement
(tests/cull_numpy.py), which tells the generator which key frames are still alive.

A script is a list of operations that play() runs on lib.LocalMap or on cull_numpy.Store: those of conn_scenarios and
    ("attr", kfs, points)  ("cull", handles, monocular)  ("poses", handles, Tcw)  ("geo", rows)
A scenario returns (script, expect, paths): expect has, per cull of the script, hand-written values of the result (a key that is
left out is not compared; "attr_flags" maps key frames to their flags byte afterwards); paths names the branches of
cull_numpy.PATHS that the scenario was built to reach."""
import numpy as np

import conn_scenarios as cs
import cull_numpy as un
import lmap_scenarios as ls

KEYFRAME, POINT, LINE = ls.KEYFRAME, ls.POINT, ls.LINE
W, O, P, CH, NU, BAD = 1, 2, 4, 8, 16, 32      # flag bits of a touched key frame
TH = np.float32(40.0)


class World:
    """key frames, points, connection rows and culling attributes that agree with each other unless a scenario says otherwise.
    point(h, [(kf, octave, depth, stereo), ...]) appends the point to each observer's match row and records the index."""

    def __init__(self):
        self.kfs, self.pts, self.akf, self.apt, self.conns, self.poses, self.geo = {}, {}, {}, {}, {}, {}, []
        self.next = 1000

    def kf(self, h, rank, parent=-1, ch=(), th=TH, flags=0, bad=0):
        self.kfs[h] = ls.kf(h, rank, bad=bad, parent=parent, ch=ch)
        self.akf[h] = dict(handle=h, th_depth=th, flags=flags, octave=[], depth=[], stereo=[])
        return self

    def entry(self, k, p, octave=0, depth=1.0, stereo=0):
        """a match-row entry alone; returns its index"""
        self.kfs[k]["points"].append(p)
        a = self.akf[k]
        a["octave"].append(octave)
        a["depth"].append(depth)
        a["stereo"].append(stereo)
        return len(a["octave"]) - 1

    def point(self, obs, n_obs=None, bad=0, h=None):
        if h is None:
            h, self.next = self.next, self.next + 1
        self.pts[h] = ls.mp(h, [o[0] for o in obs], bad=bad)
        idx = [self.entry(o[0], h, *o[1:]) for o in obs]
        own = sum(2 if (len(o) > 3 and o[3]) else 1 for o in obs)
        self.apt[h] = dict(handle=h, n_obs=own if n_obs is None else n_obs, obs_index=idx)
        return h

    def observe(self, p, k, idx):
        """an observation alone: the point names index idx of k's row, whatever stands there"""
        self.pts[p]["obs"].append(k)
        self.apt[p]["obs_index"].append(idx)

    def redundant(self, a, others, n, octave=0):
        """n points that a and three others see at one octave: each is redundant for a (and for each of the others)"""
        return [self.point([(a, octave)] + [(o, octave) for o in others]) for _ in range(n)]

    def plain(self, a, other, n):
        """n points with two mono observations: counted, never looked at"""
        return [self.point([(a, 0), (other, 0)]) for _ in range(n)]

    def conn(self, h, weights, ordered=None, first=0):
        rank = lambda k: self.kfs[k]["rank"]
        if ordered is None:
            ordered = sorted(weights, key=lambda e: (e[1], rank(e[0])), reverse=True)
        self.conns[h] = cs.conn(h, first=first, weights=weights, ordered=ordered)
        return self

    def link(self, a, b, w):
        """a symmetric covisibility edge, both ordered rows re-sorted"""
        for x, y in ((a, b), (b, a)):
            c = self.conns.get(x, cs.conn(x))
            self.conn(x, [e for e in c["weights"] if e[0] != y] + [(y, w)])
        return self

    def ops(self):
        out = [("kfs", [ls.snap(r) for r in self.kfs.values()]), ("points", [ls.snap(r) for r in self.pts.values()])]
        if self.conns:
            out.append(("conn", [dict(r) for r in self.conns.values()]))
        out.append(("attr", [dict(r) for r in self.akf.values()], [dict(r) for r in self.apt.values()]))
        if self.poses:
            hs = sorted(self.poses)
            out.append(("poses", hs, np.stack([self.poses[h] for h in hs])))
        if self.geo:
            out.append(("geo", list(self.geo)))
        return out


def play(ops, store, mode="host"):
    """the results of the script's culls, connects and updates, in order"""
    out = []
    for op in ops:
        if op[0] == "attr":
            store.set_cull_attributes(op[1], op[2])
        elif op[0] == "cull":
            out.append(store.cull(op[1], monocular=op[2], mode=mode))
        elif op[0] == "poses":
            store.set_poses(op[1], op[2])
        elif op[0] == "geo":
            store.set_point_geometry(op[1])
        else:
            out += cs.play([op], store, mode=mode)
    return out


def check(results, expect, store):
    """the hand-written expectations against what cull() returned and what the store holds afterwards"""
    culls = [r for r in results if "culled" in r]
    assert len(culls) == len(expect)
    for r, e in zip(culls, expect):
        for k, want in e.items():
            if k == "attr_flags":
                continue
            if k in ("weights", "ordered"):
                got = [cs.pairs(a) for a in r[k]]
            elif k in ("children", "nulled", "obs", "obs_index"):
                got = [[int(v) for v in a] for a in r[k]]
            else:
                got = np.asarray(r[k]).tolist()
            assert got == want, (k, got, want)
    flags = expect[-1].get("attr_flags", {})
    if flags:
        hs = sorted(flags)
        g = store.get_cull_attributes(hs, [])
        assert [a["flags"] for a in g["kfs"]] == [flags[h] for h in hs]


def _base(w, extra=()):
    """a root 1 (the origin) and the by-standers 2, 3, 4 that are never called, children of the root"""
    w.kf(1, 10, flags=un.ORIGIN, ch=[2, 3, 4] + list(extra))
    for h in (2, 3, 4):
        w.kf(h, 10 * h, parent=1)
    return w


def earlier_cull_keeps_a_later_one():
    """10 points seen by 5, 6 and the by-standers 2 and 3, n_obs 4.  Alone, each of 5 and 6 is redundant in all 10.  In one call 5
    goes first and lowers every n_obs to 3, so 6 never looks at a list: kept."""
    w = _base(World(), extra=[5, 6]).kf(5, 50, parent=1).kf(6, 60, parent=1)
    pts = [w.point([(5, 0), (6, 0), (2, 0), (3, 0)]) for _ in range(10)]
    ops = w.ops() + [("cull", [5, 6], 0)]
    expect = [dict(record=[[10, 10, 1, 1], [10, 0, 0, 0]], culled=[5], touched=[1, 5], flags=[CH, BAD], children=[[2, 3, 4, 6], []],
                   points=pts, point_n_obs=[3] * 10, point_bad=[0] * 10, obs=[[6, 2, 3]] * 10, obs_index=[[i, i, i] for i in range(10)])]
    return ops, expect, ("decision_saw_lowered_count", "few_observations", "exactly_3_observations", "exactly_4_observations")


def earlier_cull_alone_and_later_alone():
    """the same graph called as [6] and then [5]: each is culled when it comes first - 6 by the first call, and 5, whose points
    are at n_obs 3 by then, is kept by the second"""
    ops, _, _ = earlier_cull_keeps_a_later_one()
    ops = ops[:-1] + [("cull", [6], 0), ("cull", [5], 0)]
    expect = [dict(record=[[10, 10, 1, 1]], culled=[6]), dict(record=[[10, 0, 0, 0]], culled=[])]
    return ops, expect, ("verdict_yes", "verdict_no")


def earlier_cull_dooms_a_later_one():
    """the reverse.  6 sees 9 redundant points (with 2, 3, 4) and 2 points that only 5 shares with it: alone 9 > 0.9 * 11 fails.
    5 sees those 2 and 20 redundant points of its own; it is culled first, the 2 shared points drop to n_obs 1 and die, their
    entries in 6's row are nulled, and 6 stands at 9 > 0.9 * 9."""
    w = _base(World(), extra=[5, 6]).kf(5, 50, parent=1).kf(6, 60, parent=1)
    w.redundant(6, [2, 3, 4], 9)
    shared = w.plain(6, 5, 2)
    w.redundant(5, [2, 3, 4], 20)
    ops = w.ops() + [("cull", [5, 6], 0)]
    expect = [dict(record=[[22, 20, 1, 1], [9, 9, 1, 1]], culled=[5, 6], nulled=[[], [], [9, 10]], touched=[1, 5, 6],
                   flags=[CH, BAD, NU | BAD])]
    alone = w.ops() + [("cull", [6], 0)]
    return ops, expect, ("decision_saw_null_from_this_call", "point_died", "nulled_own_point"), alone, shared


def stereo_and_mono_cross_the_line():
    """two points at n_obs 4 in key frame 5's row: one that 5 sees in stereo (2 + 1 + 1) drops to 2 and dies, one that 5 sees mono
    (1 + 2 + 1) drops to 3 and lives.  20 redundant points get 5 culled."""
    w = _base(World(), extra=[5]).kf(5, 50, parent=1)
    a = w.point([(5, 0, 1.0, 1), (2, 0), (3, 0)])
    b = w.point([(5, 0, 1.0, 0), (2, 0, 1.0, 1), (3, 0)])
    red = w.redundant(5, [2, 3, 4], 20)
    ops = w.ops() + [("cull", [5], 0)]
    expect = [dict(record=[[22, 20, 1, 1]], culled=[5], points=[a, b] + red, point_n_obs=[2, 3] + [3] * 20, point_bad=[1, 0] + [0] * 20,
                   touched=[1, 2, 3, 5], flags=[CH, NU, NU, BAD], nulled=[[], [0], [0], []], obs=[[], [2, 3]] + [[2, 3, 4]] * 20)]
    return ops, expect, ("died_by_stereo", "erase_stereo", "erase_mono")


def observations_of_3_and_4():
    """nObs is the counter, not the list: two points with the same four observers, one at n_obs 3 (never looked at) and one at 4"""
    w = _base(World(), extra=[5]).kf(5, 50, parent=1)
    w.point([(5, 0), (2, 0), (3, 0), (4, 0)], n_obs=3)
    w.point([(5, 0), (2, 0), (3, 0), (4, 0)], n_obs=4)
    ops = w.ops() + [("cull", [5], 0)]
    return ops, [dict(record=[[2, 1, 0, 0]], culled=[], touched=[], points=[])], ("exactly_3_observations", "exactly_4_observations")


def third_observer_is_the_key_frame_itself():
    """in rank order the observers are 2, 3, then key frame 5 itself, then 6 at an octave too coarse: two count, the key frame
    would have been the third"""
    w = _base(World(), extra=[5, 6]).kf(5, 50, parent=1).kf(6, 60, parent=1)
    w.point([(2, 0), (3, 0), (5, 0), (6, 2)])
    ops = w.ops() + [("cull", [5], 0)]
    return ops, [dict(record=[[1, 0, 0, 0]], culled=[])], ("self_was_third", "observer_at_plus_2", "list_ended_short")


def octave_plus_one_and_plus_two():
    """key frame 5 sees both points at octave 2.  Three observers at octave 3 make the first redundant; with the third at 4 the
    second is not."""
    w = _base(World(), extra=[5]).kf(5, 50, parent=1)
    w.point([(5, 2), (2, 3), (3, 3), (4, 3)])
    w.point([(5, 2), (2, 3), (3, 3), (4, 4)])
    ops = w.ops() + [("cull", [5], 0)]
    return ops, [dict(record=[[2, 1, 0, 0]], culled=[])], ("observer_at_plus_1", "observer_at_plus_2", "stopped_at_3")


def _depths(w):
    th = np.float32(3.3)
    w.kf(5, 50, parent=1, th=th)
    for d in (th, np.nextafter(th, np.float32(np.inf)), np.float32(-0.5), np.float32(np.nan), np.float32(0.0)):
        w.point([(5, 0, d), (2, 0)])
    return w


def depth_gate():
    """depth at th_depth to the float counts, one float above is skipped, a negative depth is skipped, NaN counts (neither
    comparison holds), 0 counts"""
    ops = _depths(_base(World(), extra=[5])).ops() + [("cull", [5], 0)]
    return ops, [dict(record=[[3, 0, 0, 0]], culled=[])], ("depth_at_threshold", "depth_far", "depth_negative", "depth_nan_counted")


def monocular_on():
    """the same row with mbMonocular: no depth is looked at"""
    ops = _depths(_base(World(), extra=[5])).ops() + [("cull", [5], 1)]
    return ops, [dict(record=[[5, 0, 0, 0]], culled=[])], ("monocular_entry",)


def ninety_percent():
    """0.9 * nMPs in double.  nMPs 10: the product is 9.0 exactly, 9 redundant is not above it (5, kept) and 10 is (6, culled).
    nMPs 11: the product is not a double's integer, 9.9 to the last bit; 9 stays below (7, kept), 10 is above (8, culled)."""
    w = _base(World(), extra=[5, 6, 7, 8])
    for h, red, plain in ((5, 9, 1), (6, 10, 0), (7, 9, 2), (8, 10, 1)):
        w.kf(h, 10 * h, parent=1)
        w.redundant(h, [2, 3, 4], red)
        w.plain(h, 2, plain)
    ops = w.ops() + [("cull", [5, 6, 7, 8], 0)]
    return ops, [dict(record=[[10, 9, 0, 0], [10, 10, 1, 1], [11, 9, 0, 0], [11, 10, 1, 1]], culled=[6, 8])], ("verdict_yes", "verdict_no")


def no_map_points():
    """an empty row, a row of nulls and bad points: nMPs 0, and 0 > 0.0 does not hold"""
    w = _base(World(), extra=[5, 6]).kf(5, 50, parent=1).kf(6, 60, parent=1)
    w.entry(6, -1)
    w.point([(6, 0), (2, 0)], bad=1)
    ops = w.ops() + [("cull", [5, 6], 0)]
    return ops, [dict(record=[[0, 0, 0, 0], [0, 0, 0, 0]], culled=[], touched=[])], ("verdict_no_mps", "null_entry", "bad_entry")


def origin_and_not_erase():
    """the origin is skipped before its row is read; a key frame with mbNotErase gets the verdict and only mbToBeErased"""
    w = World().kf(1, 10, flags=un.ORIGIN, ch=[2, 3, 4, 5])
    for h in (2, 3, 4):
        w.kf(h, 10 * h, parent=1)
    w.kf(5, 50, parent=1, flags=un.NOT_ERASE)
    w.redundant(1, [2, 3, 4], 4)
    w.redundant(5, [2, 3, 4], 4)
    ops = w.ops() + [("cull", [1, 5], 0)]
    expect = [dict(record=[[0, 0, 0, 3], [4, 4, 1, 2]], culled=[], touched=[], points=[],
                   attr_flags={1: un.ORIGIN, 5: un.NOT_ERASE | un.TO_BE_ERASED})]
    return ops, expect, ("origin_skipped", "deferred")


def point_twice_in_a_row():
    """key frame 5's row holds one point at indices 0 and 2; its observation names 0.  Both entries count; the second
    EraseObservation finds nothing."""
    w = _base(World(), extra=[5]).kf(5, 50, parent=1)
    p = w.point([(5, 0), (2, 0), (3, 0), (4, 0)])
    w.entry(5, -1)
    w.entry(5, p)
    red = w.redundant(5, [2, 3, 4], 18)
    ops = w.ops() + [("cull", [5], 0)]
    expect = [dict(record=[[20, 20, 1, 1]], culled=[5], points=[p] + red, point_n_obs=[3] * 19)]
    return ops, expect, ("erase_twice_in_row",)


def observation_and_row_disagree():
    """Points a and a2 (key frame 5 in stereo, n_obs 3) each hold an observation of key frame 6 at index 0, where 6's row holds
    point b.  Point c (5 and 2, n_obs 3) stands in 6's row without observing 6.  Point d is bad and still holds observations.
    Key frame 5 is culled: a dies and EraseMapPointMatch(0) takes b out of 6's row; a2 dies and finds a null there; c drops to 2
    and dies, but nothing tells 6's row; d loses its observation of 5 like any point.  Then 6 meets a null at 0 and a point that
    went bad in this call at 1, is culled on its 20 redundant points, cannot erase b (no longer in its row, so b keeps observing
    6) and asks c to erase an observation it never had."""
    w = _base(World(), extra=[5, 6]).kf(5, 50, parent=1).kf(6, 60, parent=1)
    b = w.point([(6, 0), (2, 0), (3, 0), (4, 0)])
    a = w.point([(5, 0, 1.0, 1)], n_obs=3)
    w.observe(a, 6, 0)
    a2 = w.point([(5, 0, 1.0, 1)], n_obs=3)
    w.observe(a2, 6, 0)
    c = w.point([(5, 0), (2, 0)], n_obs=3)
    w.entry(6, c)
    d = w.point([(5, 0), (2, 0), (3, 0)], n_obs=7, bad=1)
    w.redundant(5, [2, 3, 4], 40)
    red6 = w.redundant(6, [2, 3, 4], 20)
    ops = w.ops() + [("cull", [5, 6], 0)]
    expect = [dict(record=[[43, 40, 1, 1], [20, 20, 1, 1]], culled=[5, 6], nulled=[[], [1], [], [0]], touched=[1, 2, 5, 6],
                   flags=[CH, NU, BAD, NU | BAD], points=[a, a2, c, d] + list(range(d + 1, d + 61)),
                   point_n_obs=[1, 1, 2, 6] + [3] * 60, point_bad=[1, 1, 1, 1] + [0] * 60)]
    return ops, expect, ("nulled_other_point", "nulled_already_null", "erase_not_observed", "erase_bad_point",
                         "decision_saw_dead_from_this_call", "decision_saw_null_from_this_call"), (a, b, c, red6)


def spanning_tree():
    """Key frame 5 (parent 2) is culled with children 6, 7, 8, 9, 11 in rank order.  Round 1: 6 and 7 both reach the candidate 2
    with weight 5 - the first in rank order keeps it (strict >).  Round 2: 7 reaches the new candidate 6 with 7, above its 5 to 2.
    Round 3: 9 knows only 7.  Round 4: 11 has no link to any candidate and 8 is bad: no winner; both go to 2 and stay in 5's set."""
    w = World().kf(1, 10, flags=un.ORIGIN, ch=[2, 3, 4])
    for h in (2, 3, 4):
        w.kf(h, 10 * h, parent=1)
    w.kfs[2]["children"] = [5]
    w.kf(5, 50, parent=2, ch=[6, 7, 8, 9, 11])
    for h in (6, 7, 9, 11):
        w.kf(h, 10 * h, parent=5)
    w.kf(8, 80, parent=5, bad=1)
    w.redundant(5, [2, 3, 4], 4)
    w.conn(6, [(2, 5), (5, 9)]).conn(7, [(2, 5), (6, 7), (5, 9)]).conn(8, [(2, 50)]).conn(9, [(7, 3)]).conn(11, [(3, 8)])
    w.conn(5, [(6, 9), (7, 9)])
    ops = w.ops() + [("cull", [5], 0)]
    expect = [dict(record=[[4, 4, 1, 1]], culled=[5], touched=[2, 5, 6, 7, 8, 9, 11],
                   flags=[CH, W | O | BAD | CH, W | O | P | CH, W | O | P | CH, P, P, P],
                   parent=[1, 2, 2, 6, 2, 7, 2], children=[[6, 8, 11], [8, 11], [7], [9], [], [], []],
                   weights=[[], [], [(2, 5)], [(2, 5), (6, 7)], [(2, 50)], [(7, 3)], [(3, 8)]],
                   ordered=[[], [], [(2, 5)], [(6, 7), (2, 5)], [(2, 50)], [(7, 3)], [(3, 8)]])]
    return ops, expect, ("tree_tie_kept_first", "tree_bad_child", "tree_no_link", "tree_to_grandparent", "tree_second_round_winner",
                         "erase_connection")


def equal_weights_after_erase_connection():
    """EraseConnection sorts all the weights again: key frame 6 holds 5 and, at one weight, 2 and 3: the higher rank comes first.
    Key frame 7 names 5 only in its ordered row: nothing to erase, the stale list stays."""
    w = _base(World(), extra=[5, 6, 7]).kf(5, 50, parent=1).kf(6, 60, parent=1).kf(7, 70, parent=1)
    w.redundant(5, [2, 3, 4], 4)
    w.conn(6, [(5, 30), (2, 12), (3, 12)], ordered=[(5, 30)]).conn(7, [], ordered=[(5, 4)]).conn(5, [(6, 30), (7, 4)])
    ops = w.ops() + [("cull", [5], 0)]
    expect = [dict(record=[[4, 4, 1, 1]], culled=[5], touched=[1, 5, 6], flags=[CH, W | O | BAD, W | O],
                   weights=[[], [], [(2, 12), (3, 12)]], ordered=[[], [], [(3, 12), (2, 12)]])]
    return ops, expect, ("resort_tie", "erase_connection_absent")


def reference_key_frame():
    """with geometry in the store: point a (5, 3, 2 stored in that order, reference 5) gets the lowest-ranked remaining observer 2;
    point b (5 alone, reference 5) is left with an empty map: the stored reference stays and the read is counted.  Tcp of 5 is its
    pose times the inverse of its parent's."""
    w = _base(World(), extra=[5]).kf(5, 50, parent=1)
    a = w.point([(5, 0), (3, 0), (2, 0)], n_obs=5)
    b = w.point([(5, 0)], n_obs=1)
    w.redundant(5, [2, 3, 4], 20)
    w.geo = [dict(handle=a, world=[0, 0, 1], ref_kf=5), dict(handle=b, world=[0, 0, 2], ref_kf=5)]
    T5, T1 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    T5[:3, 3] = (1, 2, 3)
    T1[:3, 3] = (0.5, 0, 0)
    w.poses = {5: T5, 1: T1}
    ops = w.ops() + [("cull", [5], 0)]
    Tcp = np.eye(4, dtype=np.float32)
    Tcp[:3, 3] = (0.5, 2, 3)
    expect = [dict(record=[[22, 20, 1, 1]], culled=[5], has_Tcp=[1], Tcp=[Tcp.tolist()], points=[a, b] + list(range(1002, 1022)),
                   point_ref=[2, 5] + [-1] * 20, point_n_obs=[4, 0] + [3] * 20, point_bad=[0, 1] + [0] * 20)]
    return ops, expect, ("ref_moved", "empty_begin")


def every_key_frame_culled():
    """a chain 1 <- 5 <- 6 <- 7, each with redundant points of its own that only by-standers share: all three go, each child is
    handed up to the parent its parent had just been given"""
    w = World().kf(1, 10, flags=un.ORIGIN, ch=[2, 3, 4, 5])
    for h in (2, 3, 4):
        w.kf(h, 10 * h, parent=1)
    w.kf(5, 50, parent=1, ch=[6]).kf(6, 60, parent=5, ch=[7]).kf(7, 70, parent=6)
    for h in (5, 6, 7):
        w.redundant(h, [2, 3, 4], 5)
    ops = w.ops() + [("cull", [5, 6, 7], 0)]
    expect = [dict(record=[[5, 5, 1, 1]] * 3, culled=[5, 6, 7], touched=[1, 5, 6, 7], flags=[CH, BAD, P | BAD, P | BAD],
                   parent=[-1, 1, 1, 1], children=[[2, 3, 4], [6], [7], []])]
    return ops, expect, ("tree_to_grandparent",)


HAND = {f.__name__: f for f in (
    earlier_cull_keeps_a_later_one, earlier_cull_alone_and_later_alone, earlier_cull_dooms_a_later_one,
    stereo_and_mono_cross_the_line, observations_of_3_and_4, third_observer_is_the_key_frame_itself, octave_plus_one_and_plus_two,
    depth_gate, monocular_on, ninety_percent, no_map_points, origin_and_not_erase, point_twice_in_a_row,
    observation_and_row_disagree, spanning_tree, equal_weights_after_erase_connection, reference_key_frame, every_key_frame_culled)}


def random_world(rng, n_kf, n_pt, obs=(4, 7), levels=4, p_stereo=0.3, p_far=0.1, root_children=True):
    """a tree of key frames under the origin 1 (handles 1 .. n_kf, ranks shuffled), points seen by obs[0] .. obs[1] of them, and
    covisibility weights from the points they share"""
    w = World()
    ranks = rng.permutation(n_kf) * 7 + 3
    w.kf(1, int(ranks[0]), flags=un.ORIGIN)
    for h in range(2, n_kf + 1):
        par = int(rng.integers(1, h))
        flags = un.NOT_ERASE if rng.random() < 0.05 else 0
        w.kf(h, int(ranks[h - 1]), parent=par, flags=flags, th=np.float32(rng.choice([3.0, 40.0])))
        w.kfs[par]["children"].append(h)
    thin = rng.choice([0.0, 0.0, 0.05, 0.3], size=n_kf + 1)       # how many of a key frame's own points few others see
    for i in range(n_pt):
        own = 2 + i % (n_kf - 1)
        k = 1 if rng.random() < thin[own] else int(rng.integers(obs[0], obs[1] + 1))
        others = [h for h in range(1, n_kf + 1) if h != own]
        seen = [own] + [int(s) for s in rng.choice(others, size=min(k, n_kf - 1), replace=False)]
        lvl = int(rng.integers(0, levels))
        row = [(int(s), int(np.clip(lvl + rng.choice([-1, 0, 0, 0, 1, 2]), 0, 7)),
                np.float32(5.0 if rng.random() < p_far else rng.random() * 2.5), int(rng.random() < p_stereo)) for s in seen]
        h = w.point(row, bad=int(rng.random() < 0.03))
        if rng.random() < 0.1:
            w.apt[h]["n_obs"] += int(rng.integers(-1, 2))          # the counter is the reference's own, not the list's
    for h in range(1, n_kf + 1):
        if rng.random() < 0.3:
            w.entry(h, -1)
    share = {}
    for p in w.pts.values():
        for a in p["obs"]:
            for b in p["obs"]:
                if a != b:
                    share[(a, b)] = share.get((a, b), 0) + 1
    for h in range(1, n_kf + 1):
        ws = [(b, v) for (a, b), v in share.items() if a == h]
        w.conn(h, ws)
        w.kfs[h]["neighbours"] = [k for k, _ in w.conns[h]["ordered"][:10]]
    return w


def random_script(seed, n_kf=24, n_pt=260, calls=5, per_call=8):
    """a world, then culls in the order of a covisibility row interleaved with connects, updates, edits of the attributes, a set_bad
    and a key frame that comes and goes; grown on the restatement, which says who is still alive"""
    rng = np.random.default_rng(seed)
    w = random_world(rng, n_kf, n_pt)
    ops = w.ops()
    ref = un.Store()
    play(ops, ref)

    def emit(op):
        ops.append(op)
        return play([op], ref)

    alive = lambda: [h for h in range(2, n_kf + 1) if not ref.kf[h].bad]
    for c in range(calls):
        live = alive()
        if not live:
            break
        call = [int(h) for h in rng.permutation(live)[:per_call]]
        if c == 1:
            call.insert(int(rng.integers(0, len(call) + 1)), 1)    # the origin among them
        emit(("cull", call, int(c == 3)))
        live = alive()
        kind = c % 5
        if kind == 0 and live:
            emit(("connect", [int(h) for h in rng.permutation(live)[:4]]))
        elif kind == 1:
            pts = [int(p) for p in rng.choice(sorted(ref.mp), size=40, replace=False)]
            emit(("update", [dict(frame_id=100 + c, points=pts)]))
        elif kind == 2 and live:
            h = int(rng.choice(live))
            a = ref.get_cull_attributes([h], [])["kfs"][0]
            emit(("attr", [dict(handle=h, th_depth=np.float32(1.5), flags=a["flags"] & ~un.NOT_ERASE, octave=a["octave"].tolist(),
                               depth=a["depth"].tolist(), stereo=a["stereo"].tolist())], []))
            p = int(rng.choice([q for q in sorted(ref.mp) if not ref.mp[q].bad]))
            b = ref.get_cull_attributes([], [p])["points"][0]
            emit(("attr", [], [dict(handle=p, n_obs=b["n_obs"] + 1, obs_index=b["obs_index"].tolist())]))
        elif kind == 3:
            p = int(rng.choice([q for q in sorted(ref.mp) if not ref.mp[q].bad]))
            emit(("bad", POINT, [p], [1]))
        elif kind == 4:
            emit(("kfs", [ls.kf(900, 100000, parent=1)]))
            emit(("attr", [dict(handle=900, th_depth=TH)], []))
            emit(("remove", KEYFRAME, 900))
    return ops
