"""Map-point and map-line creation restated on objects, from the reference's lines: the tail of
LocalMapping::CreateNewMapPoints and CreateNewMapLines2 (src/LocalMapping.cc:522-535, :1019-1031), MapPoint::AddObservation and
UpdateNormalAndDepth (src/MapPoint.cc:124-138, :376-417), MapLine::AddObservation (src/MapLine.cpp:91-100), KeyFrame::AddMapPoint
and AddMapLine (src/KeyFrame.cc:287-291, :849-853).

create() works on an insert_numpy.Store, one creation after another, every AddObservation, every row write and every
UpdateNormalAndDepth run to its end before the next creation.  A key frame may carry "octave", the octaves of its keypoints
(default 0 each), which UpdateNormalAndDepth reads at the reference key frame.  Nothing here knows of slots, appends or blocks."""
import numpy as np

import insert_numpy as inp
from insert_numpy import POINT, LINE, Refused, ERR_INVALID, ERR_CAPACITY, ERR_STATE, UPKEEP_NORMAL     # noqa: F401


def octave(w, kf, idx):
    return w.kfs[kf].get("octave", [0] * len(w.kfs[kf]["rows"][POINT]))[idx]


def create(w, points=(), lines=(), normals=True):
    """changes nothing when it raises Refused"""
    trial = w.clone()
    out = _create(trial, list(points), list(lines), normals)
    w.kfs, w.items = trial.kfs, trial.items
    w.geo.update({h: g for h, g in trial.geo.items() if h not in w.geo})      # the stored points keep what they carry
    return out


def _create(w, points, lines, normals):
    out = dict(point_displaced=[], line_displaced=[], normal=[], max_distance=[], min_distance=[], status=[])
    for kind, creations in ((POINT, points), (LINE, lines)):
        for c in creations:
            h, obs, ref = int(c["handle"]), [(int(k), int(i)) for k, i in c["obs"]], int(c["ref_kf"])
            if h < 0 or h in w.items[kind]:
                raise Refused(ERR_INVALID, "a handle the store holds, or holds since an earlier creation of the call")
            if not 1 <= len(obs) <= 2:
                raise Refused(ERR_INVALID, "0 or more than 2 observations")
            for k, i in obs:
                if k not in w.kfs:
                    raise Refused(ERR_INVALID, "an unknown key frame")
                if not 0 <= i < len(w.kfs[k]["rows"][kind]):
                    raise Refused(ERR_INVALID, "an index outside the row")
            if ref not in [k for k, _ in obs]:
                raise Refused(ERR_INVALID, "the reference key frame is not among the observations")
            if kind == POINT:
                for k, _ in obs:
                    if w.cull_fit.get(k) is False:
                        raise Refused(ERR_STATE, "a key frame without culling attributes that fit its row")
            # new MapPoint(x3D, mpCurrentKeyFrame, mpMap) / new MapLine(...): nObs 0, mnFound 1, mnVisible 1
            w.add_item(kind, h, obs=[], n_obs=0, found=1, visible=1, first_kf=int(c.get("first_kf", 0)), place=False)
            for k, i in obs:
                w._add_observation(kind, h, k, i)
            displaced = [-1, -1]
            for o, (k, i) in enumerate(obs):
                row = w.kfs[k]["rows"][kind]
                displaced[o] = row[i]                                   # AddMapPoint does not tell the item that stood there
                row[i] = h
            out["point_displaced" if kind == POINT else "line_displaced"].append(displaced)
            if kind == LINE:
                continue
            idx = dict((k, i) for k, i in reversed(w.items[POINT][h]["obs"]))   # mObservations[pRefKF]
            w.set_geo(h, np.asarray(c["world"], np.float32), ref, octave(w, ref, idx[ref]))
            if normals:
                if w.geo[h]["ref_level"] < 0 or w.geo[h]["ref_level"] >= len(w.scales) > 0:
                    raise Refused(ERR_STATE, "an octave outside the scales")
                nrm, mx, mn = w.update_normal_and_depth(h)
                out["normal"].append(nrm)
                out["max_distance"].append(mx)
                out["min_distance"].append(mn)
                out["status"].append(UPKEEP_NORMAL)
    return out
