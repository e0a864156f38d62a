"""Hand-built stores for the fuse commit with hand-written results, the bridge between a fuse_numpy.World and
a LocalMap store, and seeded scripts that interleave the call with the other operations of the store.

Key frames 10, 20, 30, 40 have the ranks 1, 2, 3, 4 - except where a scenario says otherwise - rows of 8 points and 4 lines, and
(20, 3) is a stereo keypoint.  Points are 100.., lines 500...  Every scenario returns (world, steps, expect): expect holds per step
the actions and nFused, and `after`, a dict of facts about the world after the call, all worked out by hand from the reference's
loops."""
import numpy as np

import fuse_numpy as fn
from fuse_numpy import (POINT, LINE, NEIGHBOURS, LOOP, MATCHED, NONE, SKIPPED, ADDED, ROW_ONLY, OCCUPANT_BAD, CANDIDATE_REPLACED,
                        OCCUPANT_REPLACED, SELF, RECORDED)


def base():
    w = fn.World()
    for h, rank in ((10, 1), (20, 2), (30, 3), (40, 4)):
        w.add_kf(h, rank, 8, 4, stereo=[0, 0, 0, 1 if h == 20 else 0, 0, 0, 0, 0])
    return w


def step(kf, cands, best=None, kind=POINT, form=NEIGHBOURS):
    s = dict(keyframe=kf, kind=kind, form=form, candidates=list(cands))
    if best is not None:
        s["best_idx"] = list(best)
    return s


# ---- the bridge to a store ----

def load(lm, w):
    """the key frame of the lowest rank is the origin and the parent of all others, so that a KeyFrameCulling may follow"""
    root = min(w.kfs, key=lambda h: w.kfs[h]["rank"])
    lm.set_keyframes([dict(handle=h, rank=k["rank"], bad=k["bad"], points=k["rows"][POINT], lines=k["rows"][LINE],
                           parent=-1 if h == root else root, children=[c for c in w.kfs if c != root] if h == root else [])
                      for h, k in w.kfs.items()])
    pts, lns = w.items[POINT], w.items[LINE]
    if pts:
        lm.set_points([dict(handle=h, bad=p["bad"], obs=[k for k, _ in p["obs"]]) for h, p in pts.items()])
    if lns:
        lm.set_lines(list(lns), [l["bad"] for l in lns.values()])
    lm.set_cull_attributes(
        kfs=[dict(handle=h, th_depth=40.0, flags=2 if h == root else 0, octave=[0] * len(k["stereo"]),
                  depth=[1.0] * len(k["stereo"]), stereo=k["stereo"]) for h, k in w.kfs.items()],
        points=[dict(handle=h, n_obs=p["n_obs"], obs_index=[i for _, i in p["obs"]]) for h, p in pts.items()])
    lm.set_recent_attributes(
        points=[dict(handle=h, found=p["found"], visible=p["visible"], first_kf=p["first_kf"]) for h, p in pts.items()],
        lines=[dict(handle=h, found=l["found"], visible=l["visible"], first_kf=l["first_kf"], n_obs=l["n_obs"],
                    obs=[k for k, _ in l["obs"]], obs_index=[i for _, i in l["obs"]]) for h, l in lns.items()])


def state_of_world(w):
    return dict(rows={(h, kind): list(k["rows"][kind]) for h, k in w.kfs.items() for kind in (POINT, LINE)},
                items={(kind, h): dict(bad=int(bool(it["bad"])), obs=list(it["obs"]), n_obs=it["n_obs"], found=it["found"],
                                       visible=it["visible"], replaced=it["replaced"])
                       for kind in (POINT, LINE) for h, it in w.items[kind].items()})


def state_of_store(lm, w):
    """every getter of the store, in the shape of state_of_world"""
    rows = {(h, kind): [int(v) for v in lm.get_match_row(kind, h)] for h in w.kfs for kind in (POINT, LINE)}
    items = {}
    ph, lh = sorted(w.items[POINT]), sorted(w.items[LINE])
    cull = lm.get_cull_attributes(point_handles=ph)["points"] if ph else []
    rec = lm.get_recent_attributes(point_handles=ph, line_handles=lh)
    rep = {POINT: lm.get_replaced(POINT, ph), LINE: lm.get_replaced(LINE, lh)}
    for i, h in enumerate(ph):
        bad, obs = lm.get_observers(POINT, h)
        assert len(obs) == len(cull[i]["obs_index"])
        items[(POINT, h)] = dict(bad=bad, obs=[(int(k), int(x)) for k, x in zip(obs, cull[i]["obs_index"])], n_obs=cull[i]["n_obs"],
                                 found=rec["points"][i]["found"], visible=rec["points"][i]["visible"], replaced=int(rep[POINT][i]))
    for i, h in enumerate(lh):
        bad, obs = lm.get_observers(LINE, h)
        r = rec["lines"][i]
        assert [int(k) for k in obs] == [int(k) for k in r["obs"]]
        items[(LINE, h)] = dict(bad=bad, obs=[(int(k), int(x)) for k, x in zip(r["obs"], r["obs_index"])], n_obs=r["n_obs"],
                                found=r["found"], visible=r["visible"], replaced=int(rep[LINE][i]))
    return dict(rows=rows, items=items)


def same_result(got, want):
    """a LocalMap.fuse result against a World.fuse result"""
    assert len(got["steps"]) == len(want["steps"])
    for s, (g, x) in enumerate(zip(got["steps"], want["steps"])):
        assert [int(a) for a in g["action"]] == list(x["action"]), "actions of step %d" % s
        assert g["n_fused"] == x["n_fused"], "nFused of step %d" % s
        assert [int(v) for v in g["replace"]] == list(x["replace"]), "replace of step %d" % s
    assert [(k, l, wi) for k, l, wi, _ in got["replaced"]] == [(k, l, wi) for k, l, wi, _ in want["replaced"]]
    for (_, l, _, g), (_, _, _, x) in zip(got["replaced"], want["replaced"]):
        assert [tuple(int(v) for v in r) for r in g] == [tuple(r) for r in x], "records of the Replace of %d" % l
    assert [int(v) for v in got["touched_points"]] == want["touched_points"]
    assert [int(v) for v in got["touched_lines"]] == want["touched_lines"]


def same_state(got, want):
    assert got["rows"] == want["rows"]
    assert set(got["items"]) == set(want["items"])
    for key in want["items"]:
        assert got["items"][key] == want["items"][key], "item %s: %r != %r" % (key, got["items"][key], want["items"][key])


def same_results(a, b):
    """two LocalMap.fuse results, byte for byte"""
    for g, x in zip(a["steps"], b["steps"]):
        assert np.array_equal(g["action"], x["action"]) and g["n_fused"] == x["n_fused"] and np.array_equal(g["replace"], x["replace"])
    assert len(a["steps"]) == len(b["steps"]) and len(a["replaced"]) == len(b["replaced"])
    for g, x in zip(a["replaced"], b["replaced"]):
        assert g[:3] == x[:3] and np.array_equal(g[3], x[3])
    assert np.array_equal(a["touched_points"], b["touched_points"]) and np.array_equal(a["touched_lines"], b["touched_lines"])


# ---- the scenarios ----

def add_in_front():
    """an empty entry: AddObservation, AddMapPoint; key frame 10 has the lowest rank, so it enters in front"""
    w = base()
    w.add_item(POINT, 100, [(20, 0)])
    return w, [step(10, [100, -1, 100], [2, 3, -1])], dict(
        steps=[([ADDED, NONE, NONE], 1)],
        after={"row": {(10, 2): 100}, "obs": {100: [(10, 2), (20, 0)]}, "n_obs": {100: 2}, "touched_points": [100]})


def insertion_places():
    """the new observer enters in front of the first stored observer of greater rank: in the middle (20 between 10 and 40), at
    the end (40 after 10, 30), and - in a list that is not in rank order - in front of the first greater one, not the last"""
    w = base()
    w.add_item(POINT, 100, [(10, 0), (40, 0)])
    w.add_item(POINT, 101, [(10, 1), (30, 1)])
    w.add_item(POINT, 102, [(40, 2), (10, 2), (30, 2)])
    return w, [step(20, [100, 102], [5, 6]), step(40, [101], [5])], dict(
        steps=[([ADDED, ADDED], 2), ([ADDED], 1)],
        after={"obs": {100: [(10, 0), (20, 5), (40, 0)], 101: [(10, 1), (30, 1), (40, 5)], 102: [(20, 6), (40, 2), (10, 2), (30, 2)]}})


def tie_occupant_loses():
    """equal nObs: pMPinKF->Replace(pMP); the candidate observes none of the occupant's key frames, so every entry moves"""
    w = base()
    w.add_item(POINT, 101, [(10, 2), (30, 4)], found=3, visible=5)
    w.add_item(POINT, 100, [(20, 0), (40, 1)], found=7, visible=11)
    return w, [step(10, [100], [2])], dict(
        steps=[([OCCUPANT_REPLACED], 1)],
        after={"row": {(10, 2): 100, (30, 4): 100}, "bad": {101: 1, 100: 0}, "replaced": {101: 100}, "obs": {101: [], 100: [(10, 2), (20, 0), (30, 4), (40, 1)]},
               "n_obs": {100: 4, 101: 2}, "found": {100: 10, 101: 3}, "visible": {100: 16},
               "replaced_list": [(POINT, 101, 100, [(10, 2, 1), (30, 4, 1)])], "touched_points": [100]})


def stereo_decides():
    """two observations each, but (20, 3) is stereo and counts 2: the occupant has 3 > 2, the candidate is replaced"""
    w = base()
    w.add_item(POINT, 101, [(10, 2), (20, 3)])
    w.add_item(POINT, 100, [(30, 0), (40, 0)])
    return w, [step(10, [100], [2])], dict(
        steps=[([CANDIDATE_REPLACED], 1)],
        after={"bad": {100: 1, 101: 0}, "n_obs": {101: 5, 100: 2}, "row": {(30, 0): 101, (40, 0): 101, (10, 2): 101},
               "obs": {101: [(10, 2), (20, 3), (30, 0), (40, 0)]}, "replaced": {100: 101}})


def erase_branch_and_stereo_gain():
    """the winner already observes 30: that entry of the loser is erased; it gains the stereo (20, 3), which adds 2"""
    w = base()
    w.add_item(POINT, 101, [(10, 2), (20, 3), (30, 1)])           # nObs 4
    w.add_item(POINT, 100, [(30, 0), (40, 0)], n_obs=9)           # wins on its stored counter
    return w, [step(10, [100], [2])], dict(
        steps=[([OCCUPANT_REPLACED], 1)],
        after={"row": {(10, 2): 100, (20, 3): 100, (30, 1): -1, (30, 0): 100}, "n_obs": {100: 12},
               "replaced_list": [(POINT, 101, 100, [(10, 2, 1), (20, 3, 1), (30, 1, 0)])]})


def bad_candidate_and_in_keyframe_at_its_turn():
    """102 goes bad earlier in its own step (it is the occupant that loses to 100), 100 comes to be in key frame 10 earlier in its
    step; both are skipped when their turn comes.  103 is bad from the start."""
    w = base()
    w.add_item(POINT, 102, [(10, 2)])
    w.add_item(POINT, 100, [(20, 0), (30, 0)])
    w.add_item(POINT, 103, [], bad=1)
    return w, [step(10, [100, 102, 100, 103], [2, 5, 6, 7])], dict(
        steps=[([OCCUPANT_REPLACED, SKIPPED, SKIPPED, SKIPPED], 1)],
        after={"row": {(10, 2): 100, (10, 5): -1, (10, 6): -1, (10, 7): -1}, "bad": {102: 1}})


def second_meets_first():
    """two candidates with one best_idx: the second finds the first in the entry; 1 + 1 observations against 2: a tie, the
    first loses"""
    w = base()
    w.add_item(POINT, 100, [(20, 0)])
    w.add_item(POINT, 101, [(30, 0), (40, 0)])
    return w, [step(10, [100, 101], [4, 4])], dict(
        steps=[([ADDED, OCCUPANT_REPLACED], 2)],
        after={"row": {(10, 4): 101, (20, 0): 101}, "bad": {100: 1}, "obs": {101: [(10, 4), (20, 0), (30, 0), (40, 0)]},
               "touched_points": [100, 101]})


def bad_occupant_and_self():
    """a bad occupant: nothing happens, the candidate counts; an entry that names the candidate without an observation behind
    it: Replace by itself returns at once and counts"""
    w = base()
    w.add_item(POINT, 101, [(10, 2)], bad=1)
    w.add_item(POINT, 100, [(20, 0)])
    w.kfs[10]["rows"][POINT][3] = 100                               # stale: 100 does not observe 10
    return w, [step(10, [100, 100], [2, 3])], dict(
        steps=[([OCCUPANT_BAD, SELF], 2)],
        after={"row": {(10, 2): 101, (10, 3): 100}, "bad": {100: 0, 101: 1}, "obs": {100: [(20, 0)]}, "replaced_list": []})


def stale_index_overwrites_a_third():
    """the loser's observation (30, 1) is stale: the entry holds the live 102, and is overwritten all the same"""
    w = base()
    w.add_item(POINT, 101, [(10, 2), (30, 1)])
    w.add_item(POINT, 102, [(30, 1), (40, 3)])                      # placed after 101: the entry names 102
    w.add_item(POINT, 100, [(20, 0), (40, 0)], n_obs=5)
    return w, [step(10, [100], [2])], dict(
        steps=[([OCCUPANT_REPLACED], 1)],
        after={"row": {(30, 1): 100, (10, 2): 100}, "obs": {102: [(30, 1), (40, 3)], 100: [(10, 2), (20, 0), (30, 1), (40, 0)]}, "bad": {102: 0}})


def matched_form():
    """CorrectLoop's loop: no bad test (the bad 104 wins and takes the observations), no comparison (100 has fewer observations
    and wins), AddMapPoint then AddObservation on an empty entry, the candidate itself, a null candidate"""
    w = base()
    w.add_item(POINT, 101, [(10, 0), (20, 1), (30, 1)])
    w.add_item(POINT, 100, [(40, 0)])
    w.add_item(POINT, 102, [(10, 1)])
    w.add_item(POINT, 104, [], bad=1, found=2, visible=2)
    w.add_item(POINT, 105, [(10, 3)])
    w.add_item(POINT, 106, [(20, 6)])
    return w, [step(10, [100, 104, -1, 105, 106, -1, -1, -1], form=MATCHED)], dict(
        steps=[([OCCUPANT_REPLACED, OCCUPANT_REPLACED, NONE, SELF, ADDED, NONE, NONE, NONE], 4)],
        after={"row": {(10, 0): 100, (20, 1): 100, (10, 1): 104, (10, 3): 105, (10, 4): 106}, "bad": {101: 1, 102: 1, 104: 1},
               "obs": {104: [(10, 1)], 106: [(10, 4), (20, 6)]}, "found": {104: 3}, "touched_points": [100, 104, 106]})


def loop_snapshot_against_live_read(form=LOOP):
    """the same input in both forms.  100 is added at (10, 4) by the first candidate.  LOOP took spAlreadyFound at the start:
    the second occurrence of 100 is not in it, finds an empty (10, 5) and is added again (the observation is a no-op, the row
    entry is written).  NEIGHBOURS reads IsInKeyFrame at its turn and skips it."""
    w = base()
    w.add_item(POINT, 100, [(20, 0)])
    w.add_item(POINT, 101, [(10, 1)])                               # in the row at the start: LOOP skips it, NEIGHBOURS as well
    if form == LOOP:
        steps, after = [([ADDED, ROW_ONLY, SKIPPED], 2)], {"row": {(10, 4): 100, (10, 5): 100}, "obs": {100: [(10, 4), (20, 0)]}, "n_obs": {100: 2}}
    else:
        steps, after = [([ADDED, SKIPPED, SKIPPED], 1)], {"row": {(10, 4): 100, (10, 5): -1}, "obs": {100: [(10, 4), (20, 0)]}}
    return w, [step(10, [100, 100, 101], [4, 5, 6], form=form)], dict(steps=steps, after=after)


def loop_recorded_twice():
    """one occupant recorded by two candidates: the second Replace runs on the emptied item - no observations move, mpReplaced is
    rewritten, and found and visible are added a second time.  The occupant 103 is bad and is not recorded."""
    w = base()
    w.add_item(POINT, 101, [(10, 2), (30, 1)], found=3, visible=4)
    w.add_item(POINT, 103, [(10, 6)], bad=1)
    w.add_item(POINT, 100, [(20, 0)], found=10, visible=20)
    w.add_item(POINT, 102, [(40, 0)], found=100, visible=200)
    return w, [step(10, [100, 102, 102, 100], [2, 2, 6, -1], form=LOOP)], dict(
        steps=[([RECORDED, RECORDED, OCCUPANT_BAD, NONE], 3)],
        replace=[[101, 101, -1, -1]],
        after={"row": {(10, 2): 100, (30, 1): 100}, "replaced": {101: 102}, "found": {100: 13, 102: 103}, "visible": {100: 24, 102: 204},
               "obs": {100: [(10, 2), (20, 0), (30, 1)], 102: [(40, 0)]},
               "replaced_list": [(POINT, 101, 100, [(10, 2, 1), (30, 1, 1)]), (POINT, 101, 102, [])], "touched_points": [100, 102]})


def loop_candidate_bad_in_pass2():
    """pass 1 records 101 for 100, adds 100 at (10, 5), records 100 for 102 and 103 for 100.  Pass 2: 101.Replace(100) - 100
    observes 10 by now, so (10, 2) is erased; 100.Replace(102) - 100 goes bad and its two observations move; 103.Replace(100) -
    the candidate went bad in pass 2 and takes 103's observations all the same"""
    w = base()
    w.add_item(POINT, 101, [(10, 2)])
    w.add_item(POINT, 103, [(10, 3), (40, 2)])
    w.add_item(POINT, 100, [(20, 0)])
    w.add_item(POINT, 102, [(30, 0)])
    return w, [step(10, [100, 100, 102, 100], [2, 5, 5, 3], form=LOOP)], dict(
        steps=[([RECORDED, ADDED, RECORDED, RECORDED], 4)],
        replace=[[101, -1, 100, 103]],
        after={"bad": {101: 1, 100: 1, 103: 1, 102: 0}, "replaced": {101: 100, 100: 102, 103: 100},
               "obs": {102: [(10, 5), (20, 0), (30, 0)], 100: [(10, 3), (40, 2)], 101: [], 103: []},
               "row": {(10, 2): -1, (10, 5): 102, (20, 0): 102, (10, 3): 100, (40, 2): 100},
               "replaced_list": [(POINT, 101, 100, [(10, 2, 0)]), (POINT, 100, 102, [(10, 5, 1), (20, 0, 1)]),
                                 (POINT, 103, 100, [(10, 3, 1), (40, 2, 1)])]})


def lines_and_bad_keyframe():
    """LSDmatcher::Fuse on a key frame that is bad (the reference does not look): a line's nObs grows by 1 per observation, also
    through Replace, and there is no stereo flag for lines"""
    w = base()
    w.kfs[20]["bad"] = 1
    w.add_item(LINE, 500, [(10, 0), (30, 0)])
    w.add_item(LINE, 501, [(20, 3), (40, 1)])
    w.add_item(LINE, 502, [(40, 2)])
    return w, [step(20, [500, 502, -1], [3, 1, 0], kind=LINE)], dict(
        steps=[([OCCUPANT_REPLACED, ADDED, NONE], 2)],
        after={"lrow": {(20, 3): 500, (40, 1): 500, (20, 1): 502}, "lobs": {500: [(10, 0), (20, 3), (30, 0), (40, 1)], 502: [(20, 1), (40, 2)]},
               "ln_obs": {500: 4, 502: 2}, "lbad": {501: 1}, "touched_lines": [500, 502]})


def line_in_keyframe_goes_on():
    """LSDmatcher::Fuse does not ask IsInKeyFrame (its test is commented out): a line that observes key frame 10 already is not
    skipped; on an empty entry its AddObservation is a no-op and AddMapLine writes the row; at its own entry it meets itself"""
    w = base()
    w.add_item(LINE, 500, [(10, 0)])
    return w, [step(10, [500, 500], [2, 0], kind=LINE)], dict(
        steps=[([ROW_ONLY, SELF], 2)],
        after={"lrow": {(10, 2): 500, (10, 0): 500}, "lobs": {500: [(10, 0)]}, "ln_obs": {500: 1}, "touched_lines": [], "replaced_list": []})


def two_steps_one_keyframe():
    """the second step finds what the first left: 100 is in key frame 10 now, and 101 meets it in the entry"""
    w = base()
    w.add_item(POINT, 100, [(20, 0)])
    w.add_item(POINT, 101, [(30, 0), (40, 0), (20, 1)])
    return w, [step(10, [100], [4]), step(10, [100, 101], [5, 4])], dict(
        steps=[([ADDED], 1), ([SKIPPED, OCCUPANT_REPLACED], 1)],
        after={"row": {(10, 4): 101, (20, 0): -1}, "bad": {100: 1}, "replaced_list": [(POINT, 100, 101, [(10, 4, 1), (20, 0, 0)])]})


SCENARIOS = [add_in_front, insertion_places, tie_occupant_loses, stereo_decides, erase_branch_and_stereo_gain,
             bad_candidate_and_in_keyframe_at_its_turn, second_meets_first, bad_occupant_and_self, stale_index_overwrites_a_third,
             matched_form, loop_snapshot_against_live_read, lambda: loop_snapshot_against_live_read(NEIGHBOURS), loop_recorded_twice,
             loop_candidate_bad_in_pass2, lines_and_bad_keyframe, line_in_keyframe_goes_on, two_steps_one_keyframe]


def check_expect(result, state, expect):
    """a result and a state (of a world or of a store) against the hand-written facts"""
    for s, (actions, fused) in enumerate(expect["steps"]):
        assert [int(a) for a in result["steps"][s]["action"]] == actions, "actions of step %d" % s
        assert result["steps"][s]["n_fused"] == fused
    for s, rep in enumerate(expect.get("replace", [])):
        assert [int(v) for v in result["steps"][s]["replace"]] == rep
    a = expect["after"]
    for (kf, idx), v in a.get("row", {}).items():
        assert state["rows"][(kf, POINT)][idx] == v, "row[%d][%d]" % (kf, idx)
    for (kf, idx), v in a.get("lrow", {}).items():
        assert state["rows"][(kf, LINE)][idx] == v
    for name, kind, field in (("bad", POINT, "bad"), ("obs", POINT, "obs"), ("n_obs", POINT, "n_obs"), ("found", POINT, "found"),
                              ("visible", POINT, "visible"), ("replaced", POINT, "replaced"), ("lbad", LINE, "bad"),
                              ("lobs", LINE, "obs"), ("ln_obs", LINE, "n_obs")):
        for h, v in a.get(name, {}).items():
            assert state["items"][(kind, h)][field] == v, "%s of %d: %r" % (name, h, state["items"][(kind, h)][field])
    if "replaced_list" in a:
        got = [(k, l, wi, [tuple(int(v) for v in r) for r in rec]) for k, l, wi, rec in result["replaced"]]
        assert got == a["replaced_list"]
    for name in ("touched_points", "touched_lines"):
        if name in a:
            assert [int(v) for v in result[name]] == a[name]


# ---- a KeyFrameCulling between two fusions ----

def redundant_world():
    """six key frames that see the same twelve points: 30 and 40 are redundant and a KeyFrameCulling takes them out"""
    w = fn.World()
    for k in range(6):
        w.add_kf(10 * (k + 1), k + 1, 16, 4, stereo=[int(i % 5 == 0) for i in range(16)])
    for i in range(12):
        w.add_item(POINT, 100 + i, [(10 * (k + 1), i) for k in range(6) if (i + k) % 6 != 5])
    w.add_item(POINT, 200, [(20, 14)])
    w.add_item(POINT, 201, [(50, 13), (60, 13)])
    w.add_item(LINE, 500, [(30, 0), (40, 1)])
    return w


def apply_cull(w, r):
    """what a LocalMap.cull result says the store did to itself, told to the world: the culled key frames are bad, the touched
    points have the observations, nObs and bad flag it returns, the nulled entries are null"""
    for h in r["culled"]:
        w.kfs[int(h)]["bad"] = 1
    for t, idxs in zip(r["touched"], r["nulled"]):
        for i in idxs:
            w.kfs[int(t)]["rows"][POINT][int(i)] = -1
    for p, n, bad, obs, idx in zip(r["points"], r["point_n_obs"], r["point_bad"], r["obs"], r["obs_index"]):
        w.items[POINT][int(p)].update(n_obs=int(n), bad=int(bad), obs=[(int(k), int(i)) for k, i in zip(obs, idx)])


def steps_around_a_cull():
    """before the cull; then after it: a step on the culled (bad) key frame 30, whose row still names points that no longer observe
    it - 200 meets 100 there, whose nObs shrank, and 100 is added to key frame 30 a second time - and steps on the others"""
    before = [step(10, [200, 201], [13, 12])]
    after = [step(30, [200, 100, 103], [0, 14, 15]), step(20, [101, 201, 104], [3, 1, 15]),
             step(50, [102, 105, 200], [2, 2, 12], form=LOOP), step(60, [106] + [-1] * 14 + [107], form=MATCHED)]
    return before, after


# ---- seeded worlds and scripts ----

def random_world(rng, n_kf=12, row=24, n_pts=120, n_lns=30, max_obs=6):
    w = fn.World()
    ranks = rng.permutation(n_kf) + 1
    for k in range(n_kf):
        w.add_kf(10 * (k + 1), int(ranks[k]), row, row // 2, stereo=[int(v) for v in rng.integers(0, 2, row)])
    kfs = sorted(w.kfs)
    for kind, n, base_h, width in ((POINT, n_pts, 1000, row), (LINE, n_lns, 5000, row // 2)):
        for i in range(n):
            ks = [int(k) for k in rng.choice(kfs, int(rng.integers(0, max_obs + 1)), replace=False)]
            if rng.random() < 0.7:
                ks.sort(key=lambda k: w.kfs[k]["rank"])                 # most lists are in rank order, as a std::map's
            obs = [(k, int(rng.integers(0, width))) for k in ks]
            w.add_item(kind, base_h + i, obs, found=int(rng.integers(0, 50)), visible=int(rng.integers(1, 60)), first_kf=int(rng.integers(0, 9)),
                       bad=int(rng.random() < 0.08), n_obs=None if rng.random() < 0.8 else int(rng.integers(0, 9)))
    return w


def random_steps(rng, w, n_steps=4, n_cand=40, answered=0.5):
    steps, kfs = [], sorted(w.kfs)
    for _ in range(n_steps):
        kf = int(rng.choice(kfs))
        u = rng.random()
        kind, form = (LINE, NEIGHBOURS) if u < 0.25 else (POINT, NEIGHBOURS if u < 0.55 else LOOP if u < 0.8 else MATCHED)
        pool = sorted(w.items[kind])
        width = len(w.kfs[kf]["rows"][kind])
        if form == MATCHED:
            cands = [int(rng.choice(pool)) if rng.random() < 0.3 else -1 for _ in range(width)]
            steps.append(step(kf, cands, kind=kind, form=form))
            continue
        cands = [int(c) for c in rng.choice(pool, n_cand)]
        if form == NEIGHBOURS:
            cands = [-1 if rng.random() < 0.1 else c for c in cands]
        best = [int(rng.integers(0, width)) if rng.random() < answered else -1 for _ in cands]
        steps.append(step(kf, cands, best, kind=kind, form=form))
    return steps
