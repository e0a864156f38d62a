"""The item loops of LocalMapping::ProcessNewKeyFrame restated on objects, from the reference's lines:
src/LocalMapping.cc:113-173, MapPoint::AddObservation and UpdateNormalAndDepth (src/MapPoint.cc:124-138, :370-417),
MapLine::AddObservation (src/MapLine.cpp:91-100).

A Store is a fuse_numpy.World - key frames with real match rows, items with a real observation list each - plus the geometry
UpdateNormalAndDepth reads: a pose per key frame, a position, a reference key frame and its octave per point, the scale factors.
insert() is the loop, key frame after key frame, entry after entry, every AddObservation and every UpdateNormalAndDepth run to
its end before the next entry.  Nothing here knows of slots, claims, adder bits or a merged walk."""
import numpy as np

import fuse_numpy as fn
from fuse_numpy import POINT, LINE

NULL, BAD, RECENT, ADDED = range(4)      # drfe_lmap_insert_call's action bytes
UPKEEP_NORMAL = 2                        # DRFE_UPKEEP_NORMAL
f32 = np.float32


class Refused(Exception):
    def __init__(self, rc, why):
        super().__init__(why)
        self.rc = rc


ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -3, -4      # DRFE_ERR_INVALID, DRFE_ERR_CAPACITY, DRFE_ERR_STATE


def camera_centre(Tcw):
    """KeyFrame::GetCameraCenter as SetPose leaves it: the float dot of a column of Rcw with tcw, times -1"""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    return np.array([f32(np.float64(f32(f32(f32(T[0, i] * T[0, 3]) + f32(T[1, i] * T[1, 3])) + f32(T[2, i] * T[2, 3]))) * -1.0)
                     for i in range(3)], f32)


def norm3(v):
    """cv::norm of a float 3-vector: the double sum of squares in order, then sqrt"""
    s = np.float64(0.0)
    for k in range(3):
        s = s + np.float64(v[k]) * np.float64(v[k])
    return np.sqrt(s)


class Store(fn.World):
    def __init__(self):
        super().__init__()
        self.scales = []                 # mvScaleFactors
        self.poses = {}                  # key-frame handle -> Tcw [4, 4] float32
        self.geo = {}                    # point handle -> dict(world [3] float32, ref_kf, ref_level)
        self.cull_fit = {}               # key-frame handle -> False: its culling attributes do not fit its row

    def set_pose(self, kf, centre):
        """a pose with the identity rotation and the camera centre `centre`"""
        T = np.eye(4, dtype=f32)
        T[:3, 3] = -np.asarray(centre, f32)
        self.poses[kf] = T

    def set_geo(self, point, world, ref_kf, ref_level=0):
        self.geo[point] = dict(world=np.asarray(world, f32), ref_kf=ref_kf, ref_level=ref_level)

    def clone(self):
        w = Store()
        base = super().clone()
        w.kfs, w.items = base.kfs, base.items
        w.scales = list(self.scales)
        w.poses = {k: v.copy() for k, v in self.poses.items()}
        w.geo = {k: dict(world=v["world"].copy(), ref_kf=v["ref_kf"], ref_level=v["ref_level"]) for k, v in self.geo.items()}
        w.cull_fit = dict(self.cull_fit)
        return w

    # ---- MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:370-417) ----

    def update_normal_and_depth(self, point):
        it = self.items[POINT][point]
        if not self.scales:
            raise Refused(ERR_STATE, "no scales")
        if point not in self.geo:
            raise Refused(ERR_STATE, "no position")
        g = self.geo[point]
        if g["ref_kf"] not in self.kfs or g["ref_kf"] not in self.poses:
            raise Refused(ERR_STATE, "no reference key frame, or it has no pose")
        if not 0 <= g["ref_level"] < len(self.scales):
            raise Refused(ERR_STATE, "ref_level out of range")
        for kf, _ in it["obs"]:
            if kf not in self.poses:
                raise Refused(ERR_STATE, "an observer has no pose")
        X = g["world"]
        normal = np.zeros(3, f32)
        n = 0
        with np.errstate(divide="ignore", invalid="ignore"):
            for kf, _ in it["obs"]:                                   # the stored order stands for the map's pointer order
                normali = (X - camera_centre(self.poses[kf])).astype(f32)
                a = f32(1.0 / norm3(normali))
                normal = (normali * a).astype(f32) + normal           # scaleAdd: normali * scale + normal, in float
                n += 1
            PC = (X - camera_centre(self.poses[g["ref_kf"]])).astype(f32)
            dist = f32(norm3(PC))
            max_d = f32(dist * f32(self.scales[g["ref_level"]]))
            min_d = f32(max_d / f32(self.scales[-1]))
            normal = (normal * f32(1.0 / np.float64(n))).astype(f32)
        return normal, max_d, min_d

    # ---- a call ----

    def insert(self, handles, normals=True):
        """changes nothing when it raises Refused"""
        handles = [int(h) for h in handles]
        if any(h not in self.kfs for h in handles) or len(set(handles)) != len(handles):
            raise Refused(ERR_INVALID, "an unknown or repeated key frame")
        trial = self.clone()
        out = trial._insert(handles, normals)
        self.kfs, self.items = trial.kfs, trial.items
        return out

    def _insert(self, handles, normals):
        out = dict(point_action=[], line_action=[], added_points=[], added_lines=[], recent_points=[], recent_lines=[],
                   normal=[], max_distance=[], min_distance=[], status=[])
        for kf in handles:
            # :124-157: the map points of the key frame
            action = []
            for i, p in enumerate(self.kfs[kf]["rows"][POINT]):
                if p < 0:
                    action.append(NULL)
                    continue
                it = self.items[POINT][p]
                if it["bad"]:
                    action.append(BAD)
                    continue
                if it.get("no_cull"):
                    raise Refused(ERR_STATE, "a point without culling attributes that fit")
                if not self._in_kf(POINT, p, kf):
                    if self.cull_fit.get(kf) is False:
                        raise Refused(ERR_STATE, "a key frame without culling attributes that fit its row")
                    self._add_observation(POINT, p, kf, i)
                    out["added_points"].append((p, kf, i))
                    if normals:
                        nrm, mx, mn = self.update_normal_and_depth(p)
                        out["normal"].append(nrm)
                        out["max_distance"].append(mx)
                        out["min_distance"].append(mn)
                        out["status"].append(UPKEEP_NORMAL)
                    action.append(ADDED)                               # ComputeDistinctiveDescriptors stays with the caller
                else:
                    out["recent_points"].append(p)                     # mlpRecentAddedMapPoints.push_back
                    action.append(RECENT)
            out["point_action"].append(action)
            action = []
            for i, l in enumerate(self.kfs[kf]["rows"][LINE]):
                if l < 0:
                    action.append(NULL)
                    continue
                it = self.items[LINE][l]
                if it["bad"]:
                    action.append(BAD)
                    continue
                if it.get("no_state"):
                    raise Refused(ERR_STATE, "a line without recent-list state")
                if not self._in_kf(LINE, l, kf):
                    self._add_observation(LINE, l, kf, i)
                    out["added_lines"].append((l, kf, i))
                    action.append(ADDED)                               # UpdateAverageDir stays with the caller
                else:
                    out["recent_lines"].append(l)
                    action.append(RECENT)
            out["line_action"].append(action)
        return out
