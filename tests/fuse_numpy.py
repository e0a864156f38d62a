"""The fuse commit restated on objects: ORBmatcher::Fuse / LSDmatcher::Fuse, the Sim3 form with
SearchAndFuse's loop, the matched-point loop of CorrectLoop, with MapPoint::Replace / MapLine::Replace and AddObservation.

A World holds key frames with real match rows and items with a real observation list each ((key frame, index) pairs in stored
order).  Every Replace runs to its end before the next candidate.  paths() counts the branches taken since the world was made.
Nothing here knows of slots, logs or records in device order: it is the reference's loops, line by line."""
import copy
from collections import Counter

POINT, LINE = 1, 2                       # DRFE_LMAP_POINT, DRFE_LMAP_LINE
NEIGHBOURS, LOOP, MATCHED = 0, 1, 2
NONE, SKIPPED, ADDED, ROW_ONLY, OCCUPANT_BAD, CANDIDATE_REPLACED, OCCUPANT_REPLACED, SELF, RECORDED = range(9)


def _wrap(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


class World:
    def __init__(self):
        self.kfs = {}                    # handle -> dict(rank, bad, rows={POINT: [...], LINE: [...]}, stereo=[...])
        self.items = {POINT: {}, LINE: {}}   # handle -> dict(bad, obs=[(kf, idx)], n_obs, found, visible, first_kf, replaced)
        self._paths = Counter()

    def add_kf(self, handle, rank, n_points, n_lines=0, stereo=None, bad=0):
        self.kfs[handle] = dict(rank=rank, bad=bad, rows={POINT: [-1] * n_points, LINE: [-1] * n_lines},
                                stereo=list(stereo) if stereo is not None else [0] * n_points)

    def add_item(self, kind, handle, obs=(), n_obs=None, found=1, visible=1, first_kf=0, bad=0, place=True):
        """obs: (key frame, index) pairs in stored order; place: also write the item into those row entries"""
        obs = [(int(k), int(i)) for k, i in obs]
        if n_obs is None:
            n_obs = sum(2 if kind == POINT and self.kfs[k]["stereo"][i] else 1 for k, i in obs)
        self.items[kind][handle] = dict(bad=bad, obs=obs, n_obs=n_obs, found=found, visible=visible, first_kf=first_kf, replaced=-1)
        if place:
            for k, i in obs:
                self.kfs[k]["rows"][kind][i] = handle

    def clone(self):
        w = World()
        w.kfs = copy.deepcopy(self.kfs)
        w.items = copy.deepcopy(self.items)
        return w

    def paths(self):
        return dict(self._paths)

    # ---- the reference's members ----

    def _in_kf(self, kind, item, kf):
        return any(k == kf for k, _ in self.items[kind][item]["obs"])

    def _add_observation(self, kind, item, kf, idx):
        it = self.items[kind][item]
        if self._in_kf(kind, item, kf):
            self._paths["add_observation_noop"] += 1
            return False
        rank = self.kfs[kf]["rank"]
        at = 0
        while at < len(it["obs"]) and self.kfs[it["obs"][at][0]]["rank"] <= rank:
            at += 1
        self._paths["insert_front" if at == 0 and it["obs"] else "insert_end" if at == len(it["obs"]) else "insert_middle"] += 1
        it["obs"].insert(at, (kf, idx))
        it["n_obs"] += 2 if kind == POINT and self.kfs[kf]["stereo"][idx] else 1
        return True

    def _replace(self, kind, loser, winner, out):
        if loser == winner:
            self._paths["replace_self"] += 1
            return
        L, W = self.items[kind][loser], self.items[kind][winner]
        obs, L["obs"] = L["obs"], []
        L["bad"] = 1
        L["replaced"] = winner
        if not obs:
            self._paths["replace_emptied"] += 1
        if W["bad"]:
            self._paths["replace_bad_winner"] += 1
        records = []
        for kf, idx in obs:
            if not self._in_kf(kind, winner, kf):
                self.kfs[kf]["rows"][kind][idx] = winner
                self._add_observation(kind, winner, kf, idx)
                records.append((kf, idx, 1))
                self._paths["replace_moved"] += 1
            else:
                self.kfs[kf]["rows"][kind][idx] = -1
                records.append((kf, idx, 0))
                self._paths["replace_erased"] += 1
        W["found"] = _wrap(W["found"] + L["found"])
        W["visible"] = _wrap(W["visible"] + L["visible"])
        out["replaced"].append((kind, loser, winner, records))
        self._touch(out, kind, winner)

    @staticmethod
    def _touch(out, kind, item):
        lst = out["touched_points" if kind == POINT else "touched_lines"]
        if item not in lst:
            lst.append(item)

    def _add(self, kind, item, kf, idx, out, row_first=False):
        if row_first:
            self.kfs[kf]["rows"][kind][idx] = item
        gained = self._add_observation(kind, item, kf, idx)
        self.kfs[kf]["rows"][kind][idx] = item
        if gained:
            self._touch(out, kind, item)
        return ADDED if gained else ROW_ONLY

    # ---- a call ----

    def fuse(self, steps):
        out = dict(steps=[], replaced=[], touched_points=[], touched_lines=[])
        for st in steps:
            kf, kind, form, cands = st["keyframe"], st["kind"], st["form"], [int(c) for c in st["candidates"]]
            best = list(range(len(cands))) if form == MATCHED else [int(b) for b in st["best_idx"]]
            row, items = self.kfs[kf]["rows"][kind], self.items[kind]
            action, replace, fused = [NONE] * len(cands), [-1] * len(cands), 0
            self._paths["form_%d" % form] += 1
            if form == NEIGHBOURS:
                for i, c in enumerate(cands):
                    if c < 0 or best[i] < 0:
                        self._paths["none"] += 1
                        continue
                    if items[c]["bad"] or (kind == POINT and self._in_kf(kind, c, kf)):   # LSDmatcher::Fuse does not ask IsInKeyFrame
                        self._paths["skipped_bad" if items[c]["bad"] else "skipped_in_kf"] += 1
                        action[i] = SKIPPED
                        continue
                    occ = row[best[i]]
                    if occ >= 0:
                        if items[occ]["bad"]:
                            action[i] = OCCUPANT_BAD
                        elif occ == c:
                            self._replace(kind, occ, c, out)
                            action[i] = SELF
                        elif items[occ]["n_obs"] > items[c]["n_obs"]:
                            self._replace(kind, c, occ, out)
                            action[i] = CANDIDATE_REPLACED
                        else:
                            if items[occ]["n_obs"] == items[c]["n_obs"]:
                                self._paths["tie"] += 1
                            self._replace(kind, occ, c, out)
                            action[i] = OCCUPANT_REPLACED
                    else:
                        action[i] = self._add(kind, c, kf, best[i], out)
                    fused += 1
            elif form == LOOP:
                already = set(p for p in row if p >= 0)
                skip = [items[c]["bad"] or c in already for c in cands]
                for i, c in enumerate(cands):
                    if best[i] < 0:
                        continue
                    if skip[i]:
                        action[i] = SKIPPED
                        continue
                    occ = row[best[i]]
                    if occ >= 0:
                        if not items[occ]["bad"]:
                            replace[i] = occ
                            action[i] = RECORDED
                        else:
                            action[i] = OCCUPANT_BAD
                    else:
                        action[i] = self._add(kind, c, kf, best[i], out)
                    fused += 1
                for i, c in enumerate(cands):
                    if replace[i] >= 0:
                        if items[c]["bad"]:
                            self._paths["loop_candidate_bad_in_pass2"] += 1
                        self._replace(kind, replace[i], c, out)
            else:
                for i, c in enumerate(cands):
                    if c < 0:
                        continue
                    occ = row[i]
                    if occ >= 0:
                        self._replace(kind, occ, c, out)
                        action[i] = SELF if occ == c else OCCUPANT_REPLACED
                    else:
                        action[i] = self._add(kind, c, kf, i, out, row_first=True)
                    fused += 1
            for a in action:
                self._paths["action_%d" % a] += 1
            out["steps"].append(dict(action=action, n_fused=fused, replace=replace))
        return out
