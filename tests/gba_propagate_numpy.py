"""The map update that ends LoopClosing::RunGlobalBundleAdjustment (reference src/LoopClosing.cc:722-783) restated line by line
in numpy float32 / float64 on the Python stores of lmap_numpy / conn_numpy / loop_correct_numpy: the FIFO over the spanning tree
with list.pop(0), the children in rank order, then every map point.  It shares nothing with the C++.  Parity with a build of the
reference's LoopClosing.cc is not pinned (no OpenCV here): the two cv::Mat products are read as in DESIGN.md section 29.

Where the reference would read an empty cv::Mat or loop for ever the restatement raises Refused with the handle of the item, as the
store refuses the call; it does so before it has changed anything only because it works on copies until the end."""
import copy

import numpy as np

import lmap_numpy as ln
import loop_correct_numpy as rn

f32, f64 = np.float32, np.float64
POS, REF = 1, 2


class Refused(Exception):
    def __init__(self, handle, why):
        super().__init__(f"{why} {handle}")
        self.handle = handle


def gemm_c(T, x):
    """T.rowRange(0,3).colRange(0,3) * x + T.rowRange(0,3).col(3): one cv::gemm with a C term on CV_32F, small-matrix path"""
    o = np.zeros(3, f32)
    for r in range(3):
        t = T[r][0] * x[0] + T[r][1] * x[1] + T[r][2] * x[2]
        o[r] = f32(f64(t) * f64(1.0) + f64(T[r][3]) * f64(1.0))
    return o


class KfGBA:
    def __init__(self):
        self.mTcwGBA = None
        self.mTcwBefGBA = None
        self.mnBAGlobalForKF = 0


class MpGBA:
    def __init__(self):
        self.mPosGBA = None
        self.mnBAGlobalForKF = 0


class Store(rn.Store):
    def __init__(self):
        super().__init__()
        self.kf_gba, self.mp_gba = {}, {}
        self.gcounts = dict(calls=0, visited=0, composed=0, deepest_chain=0, kind_pos=0, kind_ref=0, skipped_ref=0)

    def set_gba_keyframes(self, handles, TcwGBA, stamps):
        T = np.asarray(TcwGBA, f32).reshape(len(handles), 4, 4)
        for h, t, s in zip(handles, T, stamps):
            g = self.kf_gba.setdefault(int(h), KfGBA())
            g.mTcwGBA, g.mnBAGlobalForKF = t.copy(), int(s)

    def set_gba_points(self, handles, PosGBA, stamps):
        X = np.asarray(PosGBA, f32).reshape(len(handles), 3)
        for h, x, s in zip(handles, X, stamps):
            g = self.mp_gba.setdefault(int(h), MpGBA())
            g.mPosGBA, g.mnBAGlobalForKF = x.copy(), int(s)

    def get_gba_keyframes(self, handles):
        g = [self.kf_gba[int(h)] for h in handles]
        z = np.zeros((4, 4), f32)
        return {"TcwGBA": np.stack([z if k.mTcwGBA is None else k.mTcwGBA for k in g]).reshape(-1, 4, 4),
                "stamp": np.array([k.mnBAGlobalForKF for k in g], np.int32),
                "TcwBefGBA": np.stack([z if k.mTcwBefGBA is None else k.mTcwBefGBA for k in g]).reshape(-1, 4, 4),
                "has_TcwGBA": np.array([k.mTcwGBA is not None for k in g], np.uint8),
                "has_TcwBefGBA": np.array([k.mTcwBefGBA is not None for k in g], np.uint8)}

    def get_gba_points(self, handles):
        g = [self.mp_gba[int(h)] for h in handles]
        return {"PosGBA": np.stack([np.zeros(3, f32) if p.mPosGBA is None else p.mPosGBA for p in g]).reshape(-1, 3),
                "stamp": np.array([p.mnBAGlobalForKF for p in g], np.int32),
                "has_PosGBA": np.array([p.mPosGBA is not None for p in g], np.uint8)}

    def remove(self, kind, handle):
        super().remove(kind, handle)
        (self.kf_gba if kind == ln.KEYFRAME else self.mp_gba if kind == ln.POINT else {}).pop(int(handle), None)

    # -- LoopClosing::RunGlobalBundleAdjustment :722-783 ----------------------------------------------------------------------------
    def gba(self, loop, origins, mode=None, capacity=None, inverse_after_set_pose=False):
        """inverse_after_set_pose: the wrong reading, for the scenario that tells the two apart"""
        nLoopKF = int(loop)
        pose, kf_gba = copy.deepcopy(self.pose), copy.deepcopy(self.kf_gba)
        stamp_of = lambda h: kf_gba[h].mnBAGlobalForKF if h in kf_gba else 0
        visited = dict(keyframes=[], Tcw=[], TcwBef=[], composed=[])
        composed_now, chain, seen = set(), {}, set()
        lpKFtoCheck = [int(h) for h in origins]
        for h in lpKFtoCheck:
            if h not in self.kf:
                raise Refused(h, "unknown origin")
        seen |= set(lpKFtoCheck)
        with np.errstate(all="ignore"):
            while lpKFtoCheck:
                h = lpKFtoCheck[0]
                pKF = self.kf[h]
                if h not in pose:
                    raise Refused(h, "no pose")
                if h not in kf_gba or kf_gba[h].mTcwGBA is None:
                    raise Refused(h, "no TcwGBA")
                sChilds = sorted(pKF.children, key=lambda c: self.kf[c].rank)
                Twc = rn.Pose(kf_gba[h].mTcwGBA).Twc if inverse_after_set_pose else pose[h].Twc.copy()
                for c in sChilds:
                    if c in seen:
                        raise Refused(c, "visited twice")
                    seen.add(c)
                    if c not in pose:
                        raise Refused(c, "no pose")
                    if stamp_of(c) != nLoopKF:
                        Tchildc = rn.gemm4(pose[c].Tcw, Twc)
                        g = kf_gba.setdefault(c, KfGBA())
                        g.mTcwGBA = rn.gemm4(Tchildc, kf_gba[h].mTcwGBA)
                        g.mnBAGlobalForKF = nLoopKF
                        composed_now.add(c)
                        chain[c] = chain.get(h, 0) + 1
                    lpKFtoCheck.append(c)
                kf_gba[h].mTcwBefGBA = pose[h].Tcw.copy()
                pose[h] = rn.Pose(kf_gba[h].mTcwGBA)
                lpKFtoCheck.pop(0)
                visited["keyframes"].append(h)
                visited["Tcw"].append(pose[h].Tcw.copy())
                visited["TcwBef"].append(kf_gba[h].mTcwBefGBA.copy())
                visited["composed"].append(1 if h in composed_now else 0)
            moved = dict(points=[], world=[], kind=[])
            world, skipped = {}, 0
            for ph in sorted(self.mp):
                pMP = self.mp[ph]
                if pMP.bad:
                    continue
                if ph not in self.geo:
                    raise Refused(ph, "no geometry")
                g = self.geo[ph]
                if (self.mp_gba[ph].mnBAGlobalForKF if ph in self.mp_gba else 0) == nLoopKF:
                    if ph not in self.mp_gba or self.mp_gba[ph].mPosGBA is None:
                        raise Refused(ph, "no PosGBA")
                    world[ph] = self.mp_gba[ph].mPosGBA.copy()
                    kind = POS
                else:
                    r = g.ref_kf
                    if r not in self.kf:
                        raise Refused(ph, "unknown reference key frame of")
                    if stamp_of(r) != nLoopKF:
                        skipped += 1
                        continue
                    if r not in pose:
                        raise Refused(ph, "reference key frame without a pose of")
                    if r not in kf_gba or kf_gba[r].mTcwBefGBA is None:
                        raise Refused(ph, "reference key frame without TcwBefGBA of")
                    Xc = gemm_c(kf_gba[r].mTcwBefGBA, g.world)
                    world[ph] = gemm_c(pose[r].Twc, Xc)
                    kind = REF
                moved["points"].append(ph)
                moved["world"].append(world[ph].copy())
                moved["kind"].append(kind)
        if capacity is not None and (len(visited["keyframes"]) > capacity[0] or len(moved["points"]) > capacity[1]):
            raise Refused(-1, "capacity")
        self.pose, self.kf_gba = pose, kf_gba
        for ph, x in world.items():
            self.geo[ph].world = x
        c = self.gcounts
        c["calls"] += 1
        c["visited"] += len(visited["keyframes"])
        c["composed"] += len(composed_now)
        c["deepest_chain"] = max([c["deepest_chain"]] + list(chain.values()))
        c["kind_pos"] += moved["kind"].count(POS)
        c["kind_ref"] += moved["kind"].count(REF)
        c["skipped_ref"] += skipped
        v, m = len(visited["keyframes"]), len(moved["points"])
        return {"keyframes": np.array(visited["keyframes"], np.int32), "Tcw": np.array(visited["Tcw"], f32).reshape(v, 4, 4),
                "TcwBef": np.array(visited["TcwBef"], f32).reshape(v, 4, 4), "composed": np.array(visited["composed"], np.uint8),
                "points": np.array(moved["points"], np.int32), "world": np.array(moved["world"], f32).reshape(m, 3),
                "kind": np.array(moved["kind"], np.uint8)}


GBA_KEYS = ("keyframes", "Tcw", "TcwBef", "composed", "points", "world", "kind")


def same_bits(x, y, what):
    """equal bytes; where both hold a NaN only NaN-ness is compared (payloads are exempt)"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape, (what, x.dtype, y.dtype, x.shape, y.shape)
    if x.dtype.kind == "f":
        nx, ny = np.isnan(x), np.isnan(y)
        assert np.array_equal(nx, ny), (what, x, y)
        x, y = np.where(nx, x.dtype.type(0), x), np.where(ny, y.dtype.type(0), y)
    assert x.tobytes() == y.tobytes(), (what, x, y)


def same_gba(a, b):
    for k in GBA_KEYS:
        same_bits(a[k], b[k], k)


def snapshot(store, kfs, pts):
    """every getter the call may change, for the handles that have the piece"""
    out = {}
    for h in kfs:
        for name, get in (("pose", store.get_poses), ("gba_kf", store.get_gba_keyframes)):
            try:
                out[(name, h)] = get([h])
            except Exception:
                out[(name, h)] = None
    for h in pts:
        for name, get in (("geo", store.get_point_geometry), ("gba_mp", store.get_gba_points)):
            try:
                out[(name, h)] = get([h])
            except Exception:
                out[(name, h)] = None
    return out


def same_snapshot(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            for f in a[k]:
                same_bits(a[k][f], b[k][f], (k, f))


def same_store(a, b, kfs, pts):
    same_snapshot(snapshot(a, kfs, pts), snapshot(b, kfs, pts))
