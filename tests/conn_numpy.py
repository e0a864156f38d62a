"""A literal restatement of KeyFrame::UpdateConnections, AddConnection and UpdateBestCovisibles (reference src/KeyFrame.cc:200-234,
366-500) on Python objects: every key frame carries a real mConnectedKeyFrameWeights dict keyed by key-frame objects, the ordered
lists, mbFirstConnection, mpParent and mspChildrens; KFcounter is a dict walked in rank order (the reference's pointer order); the
calls of a connect() run one after another.  It shares nothing with dr_slam_amd/csrc/conn_core.h: no slots, no keys, no closed
form.  It extends lmap_numpy.Store, so that update() reads the graph that connect() left, and has lib.LocalMap's interface, so a
script (tests/conn_scenarios.py) plays on either."""
import numpy as np

import lmap_numpy as ln

TH = 15


class Store(ln.Store):
    def __init__(self):
        super().__init__()
        self.conn = {}          # handle -> dict(first, weights {handle: w}, ordered [(handle, w)]): what set_connections gave
        self.ccounts = dict(calls=0, keyframes=0, counter_entries=0, listed=0, touched=0, first_connections=0, empty_counters=0)

    # -- the store's interface --------------------------------------------------------------------------------------------------
    def set_connections(self, rows):
        for r in rows:
            self.conn[int(r["handle"])] = dict(first=bool(r.get("first")), weights={int(k): int(w) for k, w in r.get("weights", ())},
                                               ordered=[(int(k), int(w)) for k, w in r.get("ordered", ())])

    def remove(self, kind, handle):
        super().remove(kind, handle)
        if kind == ln.KEYFRAME:
            self.conn.pop(int(handle), None)

    def _state(self, h):
        return self.conn.setdefault(h, dict(first=False, weights={}, ordered=[]))

    def get_connections(self, handles):
        rank = lambda h: self.kf[h].rank
        out = dict(parent=[], first=[], weights=[], ordered=[], children=[])
        for h in (int(x) for x in handles):
            st = self._state(h)
            out["parent"].append(self.kf[h].parent)
            out["first"].append(int(st["first"]))
            out["weights"].append(np.array([(k, st["weights"][k]) for k in sorted(st["weights"], key=rank)], np.int32).reshape(-1, 2))
            out["ordered"].append(np.array(st["ordered"], np.int32).reshape(-1, 2))
            out["children"].append(np.array(sorted(self.kf[h].children, key=rank), np.int32))
        out["parent"] = np.array(out["parent"], np.int32)
        out["first"] = np.array(out["first"], np.uint8)
        return out

    # -- the three functions ----------------------------------------------------------------------------------------------------
    def _best_covisibles(self, h):
        """UpdateBestCovisibles: every entry of the weights as pair<int, KeyFrame*>, sorted ascending, walked into push_front"""
        st = self._state(h)
        pairs = sorted(((w, self.kf[k].rank, k) for k, w in st["weights"].items()))
        ordered = []
        for w, _, k in pairs:
            ordered.insert(0, (k, w))
        st["ordered"] = ordered

    def _add_connection(self, h, other, weight):
        st = self._state(h)
        if other not in st["weights"]:
            st["weights"][other] = weight
        elif st["weights"][other] != weight:
            st["weights"][other] = weight
        else:
            return
        self._best_covisibles(h)

    def _update_connections(self, h):
        """returns (KFcounter in rank order, record, new parent)"""
        me = self.kf[h]
        counter = {}
        for ph in me.mvpMapPoints:
            if ph == -1:
                continue
            pMP = self.mp[ph]
            if pMP.bad:
                continue
            for oh in pMP.observations:
                if oh == h:
                    continue
                counter[oh] = counter.get(oh, 0) + 1
        walk = sorted(counter, key=lambda k: self.kf[k].rank)
        in_rank_order = [(k, counter[k]) for k in walk]
        if not counter:
            return in_rank_order, [0, 0, 0, -1], -1
        nmax, pKFmax = 0, None
        vPairs = []
        for k in walk:
            if counter[k] > nmax:
                nmax, pKFmax = counter[k], k
            if counter[k] >= TH:
                vPairs.append((counter[k], k))
                self._add_connection(k, h, counter[k])
        if not vPairs:
            vPairs.append((nmax, pKFmax))
            self._add_connection(pKFmax, h, nmax)
        vPairs.sort(key=lambda p: (p[0], self.kf[p[1]].rank))
        lKFs, lWs = [], []
        for w, k in vPairs:
            lKFs.insert(0, k)
            lWs.insert(0, w)
        st = self._state(h)
        st["weights"] = dict(counter)
        st["ordered"] = list(zip(lKFs, lWs))
        new_parent = -1
        if st["first"]:
            me.parent = lKFs[0]
            if h not in self.kf[me.parent].children:            # a set<KeyFrame*>
                self.kf[me.parent].children.append(h)
            st["first"] = False
            new_parent = me.parent
            self.ccounts["first_connections"] += 1
        return in_rank_order, [len(counter), len(vPairs), nmax, pKFmax], new_parent

    def connect(self, handles, mode=None, capacity=None):
        handles = [int(h) for h in handles]
        assert len(set(handles)) == len(handles)
        before = {}

        def snap(h):
            if h not in before:
                st = self._state(h)
                before[h] = (dict(st["weights"]), list(st["ordered"]), self.kf[h].parent)

        counters, records, parents = [], [], []
        for h in handles:
            snap(h)
            # every key frame this call can reach is known only after the vote, so the states are snapped through a dry vote
            for ph in self.kf[h].mvpMapPoints:
                if ph != -1 and not self.mp[ph].bad:
                    for oh in self.mp[ph].observations:
                        if oh != h:
                            snap(oh)
            c, rec, par = self._update_connections(h)
            counters.append(np.array(c, np.int32).reshape(-1, 2))
            records.append(rec)
            parents.append(par)
        # touched: called, or listed by a called key frame
        touched = set(handles)
        for h, c, rec in zip(handles, counters, records):
            listed = [int(k) for k, v in c if v >= TH]
            if len(c) and not listed:
                listed = [rec[3]]
            touched.update(listed)
        touched = sorted(touched, key=lambda k: self.kf[k].rank)
        res = self.get_connections(touched)
        res.pop("children")
        flags = []
        for i, h in enumerate(touched):
            w0, o0, p0 = before[h]
            st = self._state(h)
            flags.append((1 if st["weights"] != w0 else 0) | (2 if st["ordered"] != o0 else 0) | (4 if self.kf[h].parent != p0 else 0))
            if st["ordered"] != o0:                             # the commit: GetBestCovisibilityKeyFrames(10) for UpdateLocalMap
                self.kf[h].neighbours = [k for k, _ in st["ordered"][:10]]
        res.update(counter=counters, record=np.array(records, np.int32).reshape(len(handles), 4), new_parent=np.array(parents, np.int32),
                   touched=np.array(touched, np.int32), flags=np.array(flags, np.uint8))
        if handles:
            self.ccounts["calls"] += 1
            self.ccounts["keyframes"] += len(handles)
            self.ccounts["counter_entries"] += sum(len(c) for c in counters)
            self.ccounts["listed"] += sum(r[1] for r in records)
            self.ccounts["touched"] += len(touched)
            self.ccounts["empty_counters"] += sum(1 for r in records if r[0] == 0)
        return res


CONNECT_LISTS = ("counter", "weights", "ordered")
CONNECT_ARRAYS = ("record", "new_parent", "touched", "parent", "first", "flags")


def same_connect(a, b):
    """two results of connect(): equal bytes"""
    for k in CONNECT_ARRAYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (k, x, y)
    for k in CONNECT_LISTS:
        assert len(a[k]) == len(b[k]), k
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (k, i, x.tolist(), y.tolist())


def same_state(a, b, handles):
    """two stores answer get_connections alike"""
    ga, gb = a.get_connections(handles), b.get_connections(handles)
    for k in ("parent", "first"):
        assert np.asarray(ga[k]).tobytes() == np.asarray(gb[k]).tobytes(), (k, ga[k], gb[k])
    for k in ("weights", "ordered", "children"):
        for i, (x, y) in enumerate(zip(ga[k], gb[k])):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (k, handles[i], x.tolist(), y.tolist())
