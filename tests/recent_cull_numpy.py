"""A literal restatement of LocalMapping::MapPointCulling and MapLineCulling (reference src/LocalMapping.cc:175-231) with
MapPoint::SetBadFlag (src/MapPoint.cc:175-202) and MapLine::SetBadFlag on Python objects: every item carries a real observation
dict {key frame: index}, the recent list is a Python list that is walked with erasure as the reference walks its std::list, and
every SetBadFlag runs to its end before the next entry is looked at.  It shares nothing with dr_slam_amd/csrc/recent_core.h: no
slots, no claims, no prefix.  It extends cull_numpy.Store, so that update(), connect() and cull() read what recent_cull() left, and
has lib.LocalMap's interface, so a script (tests/recent_cull_scenarios.py) plays on either.

paths() counts the branches the walks took since the store was made."""
import numpy as np

import cull_numpy as un
import lmap_numpy as ln

KEPT, WAS_BAD, RATIO, OBSERVATIONS, AGED = range(5)
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -3, -4
Refused = un.Refused
f32 = np.float32

PATHS = ("was_bad", "point_ratio", "point_ratio_nan", "point_ratio_inf", "point_ratio_exactly_quarter", "line_ratio",
         "line_ratio_whole_multiple", "culled_observations", "observations_at_threshold", "observations_above_threshold", "aged_out",
         "kept", "first_kf_negative", "id_above_bit_31", "second_of_culled", "second_of_kept", "nulled_own", "nulled_other",
         "nulled_already_null", "bad_observer", "no_observations")


def c_int(v):
    """(int) of a long, as the compilers the reference builds with do it"""
    v = int(v) & 0xffffffff
    return v - (1 << 32) if v >= (1 << 31) else v


def wrap32(v):
    return c_int(v)


def c_div(a, b):
    """int / int, truncating toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


class Store(un.Store):
    def __init__(self):
        super().__init__()
        self.rec_mp, self.rec_ml = {}, {}
        self.rcounts = dict(calls=0, entries=0, culled_ratio=0, culled_observations=0, aged_out=0, dropped_bad=0, nulled=0)
        self._rpaths = dict.fromkeys(PATHS, 0)

    def paths(self):
        return dict(self._rpaths)

    # -- the store's interface --------------------------------------------------------------------------------------------------
    def set_recent_attributes(self, points=(), lines=()):
        for r in points:
            self.rec_mp[int(r["handle"])] = dict(found=int(r["found"]), visible=int(r["visible"]), first_kf=int(r["first_kf"]))
        for r in lines:
            obs, idx = [int(v) for v in r.get("obs", ())], [int(v) for v in r.get("obs_index", ())]
            assert len(obs) == len(idx) == len(set(obs))
            self.rec_ml[int(r["handle"])] = dict(found=int(r["found"]), visible=int(r["visible"]), first_kf=int(r["first_kf"]),
                                                 n_obs=int(r["n_obs"]), observations=dict(zip(obs, idx)))

    def get_recent_attributes(self, point_handles=(), line_handles=()):
        pts = [dict(handle=int(h), **self.rec_mp[int(h)]) for h in point_handles]
        lns = []
        for h in line_handles:
            a = self.rec_ml[int(h)]
            lns.append(dict(handle=int(h), found=a["found"], visible=a["visible"], first_kf=a["first_kf"], n_obs=a["n_obs"],
                            obs=np.array(list(a["observations"]), np.int32),
                            obs_index=np.array(list(a["observations"].values()), np.int32)))
        return dict(points=pts, lines=lns)

    def recent_increase(self, kind, handles, d_found, d_visible):
        table = self.rec_mp if kind == ln.POINT else self.rec_ml
        if any(int(h) not in table for h in handles):
            raise Refused(ERR_INVALID, "a handle without attributes")
        for h, df, dv in zip(handles, d_found, d_visible):
            a = table[int(h)]
            a["found"], a["visible"] = wrap32(a["found"] + int(df)), wrap32(a["visible"] + int(dv))

    def remove(self, kind, handle):
        super().remove(kind, handle)
        (self.rec_mp if kind == ln.POINT else self.rec_ml if kind == ln.LINE else {}).pop(int(handle), None)

    # -- what the walks read ------------------------------------------------------------------------------------------------------
    def _recent_item(self, kind, h):
        return (self.mp if kind == ln.POINT else self.ml)[h]

    def _recent_attr(self, kind, h):
        """(found, visible, first, nObs, observations) of an item, refusing when a piece is not there"""
        name = f"map point {h}" if kind == ln.POINT else f"map line {h}"
        a = (self.rec_mp if kind == ln.POINT else self.rec_ml).get(h)
        if a is None:
            raise Refused(ERR_STATE, name)
        if kind == ln.POINT:
            c = self.cull_mp.get(h)
            if c is None or len(c["obs_index"]) != len(self.mp[h].observations):
                raise Refused(ERR_STATE, name)
            n_obs, obs = c["n_obs"], dict(zip(self.mp[h].observations, c["obs_index"]))
        else:
            n_obs, obs = a["n_obs"], a["observations"]
        for kh, idx in obs.items():
            if kh not in self.kf:
                raise Refused(ERR_STATE, f"{name} names unknown handle {kh}")
            row = self.kf[kh].mvpMapPoints if kind == ln.POINT else self.kf[kh].mvpMapLines
            if not 0 <= idx < len(row):
                raise Refused(ERR_STATE, f"{name}: obs_index {idx}")
        return a["found"], a["visible"], a["first_kf"], n_obs, obs

    def _recent_check(self, kind, handles):
        table = self.mp if kind == ln.POINT else self.ml
        for h in handles:
            if h not in table:
                raise Refused(ERR_INVALID, "unknown handle")
        for h in handles:
            if table[h].bad:
                continue
            found, visible, _, _, _ = self._recent_attr(kind, h)
            if kind == ln.LINE and (visible == 0 or (found == -(1 << 31) and visible == -1)):
                raise Refused(ERR_STATE, f"map line {h}: mnFound / mnVisible is not defined")

    def _item_set_bad_flag(self, kind, h):
        """MapPoint::SetBadFlag / MapLine::SetBadFlag; returns the erased observations in stored order"""
        P = self._rpaths
        obs = self._recent_attr(kind, h)[4]
        item = self._recent_item(kind, h)
        item.bad = True
        erased = list(obs.items())
        if kind == ln.POINT:
            item.observations = []
            self.cull_mp[h]["obs_index"] = []
        else:
            self.rec_ml[h]["observations"] = {}
        P["no_observations"] += not erased
        for kh, idx in erased:                                      # pKF->EraseMapPointMatch(mit->second)
            pKF = self.kf[kh]
            row = pKF.mvpMapPoints if kind == ln.POINT else pKF.mvpMapLines
            P["bad_observer"] += bool(pKF.bad)
            P["nulled_own" if row[idx] == h else "nulled_already_null" if row[idx] == -1 else "nulled_other"] += 1
            self.rcounts["nulled"] += row[idx] != -1
            row[idx] = -1
        return erased

    def _found_ratio_low(self, kind, found, visible):
        P = self._rpaths
        if kind == ln.POINT:
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = f32(found) / f32(visible)
            P["point_ratio_nan"] += bool(np.isnan(ratio))
            P["point_ratio_inf"] += bool(np.isinf(ratio))
            P["point_ratio_exactly_quarter"] += bool(ratio == f32(0.25))
            return bool(ratio < f32(0.25))
        ratio = f32(c_div(found, visible))
        P["line_ratio_whole_multiple"] += found != 0 and found % visible == 0
        return bool(ratio < f32(0.25))

    def _recent_walk(self, kind, handles, current, monocular):
        """the list walked with erasure; returns (action per original entry, the list that is left, culled handles, erased)"""
        P, C = self._rpaths, self.rcounts
        lst = [(h, i) for i, h in enumerate(handles)]
        action = [None] * len(lst)
        culled, erased, verdicts = [], [], {}
        th = 2 if monocular else 3
        at = 0
        while at < len(lst):
            h, i = lst[at]
            item = self._recent_item(kind, h)
            if item.bad:
                P["was_bad"] += 1
                P["second_of_culled"] += h in culled
                C["dropped_bad"] += 1
                action[i] = WAS_BAD
                del lst[at]
                continue
            found, visible, first, n_obs, _ = self._recent_attr(kind, h)
            P["second_of_kept"] += h in verdicts
            age = c_int(current) - c_int(first)
            P["first_kf_negative"] += first < 0
            P["id_above_bit_31"] += c_int(current) != current or c_int(first) != first
            if self._found_ratio_low(kind, found, visible):
                P["point_ratio" if kind == ln.POINT else "line_ratio"] += 1
                C["culled_ratio"] += 1
                action[i] = RATIO
            elif age >= 2 and n_obs <= th:
                P["culled_observations"] += 1
                P["observations_at_threshold"] += n_obs == th
                C["culled_observations"] += 1
                action[i] = OBSERVATIONS
            elif age >= 3:
                P["aged_out"] += 1
                C["aged_out"] += 1
                action[i] = AGED
            else:
                P["kept"] += 1
                P["observations_above_threshold"] += age >= 2 and n_obs == th + 1
                action[i] = KEPT
            verdicts[h] = action[i]
            if action[i] in (RATIO, OBSERVATIONS):
                erased.append(self._item_set_bad_flag(kind, h))
                culled.append(h)
            if action[i] == KEPT:
                at += 1
            else:
                del lst[at]
        return action, [h for h, _ in lst], culled, erased

    def recent_cull(self, current_kf_id, points=(), lines=(), monocular=False, mode=None, capacity=None):
        points, lines = [int(h) for h in points], [int(h) for h in lines]
        self._recent_check(ln.POINT, points)
        self._recent_check(ln.LINE, lines)
        if capacity is not None:
            # what the call would erase, on a copy of nothing: the verdict of an item reads only the item
            for kind, hs, cap in ((ln.POINT, points, capacity[0]), (ln.LINE, lines, capacity[1])):
                total, seen = 0, set()
                th = 2 if monocular else 3
                for h in hs:
                    if self._recent_item(kind, h).bad or h in seen:
                        continue
                    found, visible, first, n_obs, obs = self._recent_attr(kind, h)
                    age = c_int(current_kf_id) - c_int(first)
                    saved = dict(self._rpaths)
                    low = self._found_ratio_low(kind, found, visible)
                    self._rpaths = saved
                    if low or (age >= 2 and n_obs <= th):
                        seen.add(h)
                        total += len(obs)
                if total > cap:
                    raise Refused(ERR_CAPACITY, "erased_capacity")
        self.rcounts["calls"] += bool(points or lines)
        self.rcounts["entries"] += len(points) + len(lines)
        res = {}
        for name, kind, hs in (("points", ln.POINT, points), ("lines", ln.LINE, lines)):
            action, kept, culled, erased = self._recent_walk(kind, hs, int(current_kf_id), monocular)
            res[name] = dict(action=np.array(action, np.uint8), kept=np.array(kept, np.int32), culled=np.array(culled, np.int32),
                             erased=[np.array(e, np.int32).reshape(-1, 2) for e in erased])
        return res


def same_recent(a, b):
    for name in ("points", "lines"):
        x, y = a[name], b[name]
        for k in ("action", "kept", "culled"):
            assert np.asarray(x[k]).dtype == np.asarray(y[k]).dtype and np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), (name, k, x[k], y[k])
        assert len(x["erased"]) == len(y["erased"]), name
        for i, (u, v) in enumerate(zip(x["erased"], y["erased"])):
            assert u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes(), (name, "erased", i, u, v)


def same_attributes(a, b, pts, lns):
    x, y = a.get_recent_attributes(pts, lns), b.get_recent_attributes(pts, lns)
    for k in ("points", "lines"):
        assert len(x[k]) == len(y[k])
        for r, s in zip(x[k], y[k]):
            assert set(r) == set(s)
            for f in r:
                assert np.asarray(r[f]).tolist() == np.asarray(s[f]).tolist(), (k, r["handle"], f, r[f], s[f])
