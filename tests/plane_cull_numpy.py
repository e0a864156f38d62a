"""An independent numpy restatement of LocalMapping::MapPlaneCulling (reference src/LocalMapping.cc:233-307) with
Map::PointDistanceFromPlane (src/Map.cc:433-448) and MapPlane::Replace (src/MapPlane.cc:197-271) for the host tests
(DESIGN.md section 30), in explicit float32 and float64 steps: the walk as the reference writes it, Replace rebuilding the
survivor's cloud at once (map_plane_numpy.rebuild).  It also reports which paths a scene took (paths()).

A scene is a dict: coefs [P, 4] f32, bad [P], clouds (list of P [n, 3] f32), found / visible / n_obs / first_kf_id [P],
obs (per plane a list of (key frame, plane in it), key frames ascending: std::map<KeyFrame*> order), kf_clouds (per key frame a
list of [n, 3] clouds), Twc [K, 4, 4] f32, dTh, aTh (floats: doubles in the reference), current_kf_id, recent (plane indices,
-1 = a plane that has left the map)."""
import numpy as np

import map_plane_numpy as mpn

f32, f64 = np.float32, np.float64
KEPT, ERASED_BAD, BAD_BY_RATIO, BAD_BY_OBSERVATIONS, ERASED_BY_AGE = range(5)


def angle_of(c1, c2):
    """three float products summed left to right"""
    c1, c2 = np.asarray(c1, f32), np.asarray(c2, f32)
    return f32(f32(f32(c1[0] * c2[0]) + f32(c1[1] * c2[1])) + f32(c1[2] * c2[2]))


def gate(angle, aTh):
    """angle > aTh || angle < -aTh with the float widened: the compare happens in double"""
    a, t = f64(f32(angle)), f64(aTh)
    return bool(a > t or a < -t)


def point_distance_from_plane(coef, cloud):
    """Map::PointDistanceFromPlane: res = 100; per point the float abs(a x + b y + c z + d) widened; no z skip; NaN never wins"""
    c = np.asarray(coef, f32)
    p = np.asarray(cloud, f32).reshape(-1, 3)
    res = f64(100)
    if len(p):
        with np.errstate(all="ignore"):
            d = np.abs(f32(f32(f32(c[0] * p[:, 0]) + f32(c[1] * p[:, 1])) + f32(c[2] * p[:, 2])) + c[3]).astype(f32)
        for v in d.astype(f64):
            if v < res:
                res = v
    return res


def found_ratio(found, visible):
    with np.errstate(all="ignore"):
        return f32(f32(int(found)) / f32(int(visible)))


def cull(scene):
    P = len(scene["coefs"])
    coefs = np.asarray(scene["coefs"], f32).reshape(P, 4)
    bad = [bool(b) for b in scene["bad"]]
    clouds = [np.asarray(c, f32).reshape(-1, 3) for c in scene["clouds"]]
    found = [int(v) for v in scene["found"]]
    visible = [int(v) for v in scene["visible"]]
    n_obs = [int(v) for v in scene["n_obs"]]
    obs = [dict(o) for o in scene["obs"]]                   # key frame -> plane index in it
    Twc = np.asarray(scene["Twc"], f32).reshape(-1, 4, 4)
    dTh, aTh = f64(scene["dTh"]), f64(scene["aTh"])
    events, rebuilt = [], set()
    unread = set()                                          # rebuilt clouds nobody has read since
    cnt = dict(gated_pairs=0, pair_points=0, rebuilds=0, stale_columns=0)
    path = dict(events=0, replaced_first=0, replaced_second=0, shared_keyframe=0, chain=0, dead_row=0, dead_column=0,
                stale_grew=0, stale_shrank=0, unread_rebuilds=0, rebuilt_twice=0, empty_cloud_scans=0, negative_gate=0,
                verdicts=[0] * 5)
    times_rebuilt = {}

    def replace(dead, surv):
        """dead->Replace(surv)"""
        if dead in unread:                                  # the cloud it keeps was built before its set is cleared
            unread.discard(dead)
            cnt["rebuilds"] += 1
        bad[dead] = True
        mine, obs[dead] = obs[dead], {}
        for kf in sorted(mine):
            if kf not in obs[surv]:
                obs[surv][kf] = mine[kf]
                n_obs[surv] += 1
            else:
                path["shared_keyframe"] += 1
        found[surv] += found[dead]
        visible[surv] += visible[dead]
        before = len(clouds[surv])
        kfs = sorted(obs[surv])
        clouds[surv] = mpn.rebuild([Twc[k] for k in kfs], [scene["kf_clouds"][k][obs[surv][k]] for k in kfs])
        path["stale_grew" if len(clouds[surv]) > before else "stale_shrank"] += len(clouds[surv]) != before
        rebuilt.add(surv)
        unread.add(surv)
        times_rebuilt[surv] = times_rebuilt.get(surv, 0) + 1
        if any(e[1] == dead for e in events):                # the replaced plane had survived an earlier row
            path["chain"] += 1
        events.append((dead, surv))

    for i in range(P):
        best = -1
        ldTh = f32(dTh)                                     # float ldTh = dTh
        if bad[i]:
            path["dead_row"] += any(e[0] == i for e in events)
        for j in range(i + 1, P):
            if bad[i] or bad[j]:
                path["dead_column"] += (not bad[i]) and any(e[0] == j for e in events)
                continue
            a = angle_of(coefs[i], coefs[j])
            if not gate(a, aTh):
                continue
            path["negative_gate"] += bool(a < 0)
            if j in unread:
                unread.discard(j)
                cnt["rebuilds"] += 1
                cnt["stale_columns"] += 1
                path["rebuilt_twice"] += times_rebuilt.get(j, 0) > 1
            cnt["gated_pairs"] += 1
            cnt["pair_points"] += len(clouds[j])
            path["empty_cloud_scans"] += len(clouds[j]) == 0
            dis = point_distance_from_plane(coefs[i], clouds[j])
            if dis < f64(ldTh):
                ldTh = f32(dis)
                best = j
        if best != -1:
            if n_obs[i] > n_obs[best]:
                path["replaced_second"] += 1
                replace(best, i)
            else:
                path["replaced_first"] += 1
                replace(i, best)
    cnt["rebuilds"] += len(unread)
    path["unread_rebuilds"] = len(unread)
    path["events"] = len(events)

    verdicts = []
    cur = int(scene["current_kf_id"])
    for p in scene["recent"]:
        p = int(p)
        if p < 0 or bad[p]:
            v = ERASED_BAD
        elif found_ratio(found[p], visible[p]) < f32(0.25):
            v = BAD_BY_RATIO
        elif cur - int(scene["first_kf_id"][p]) >= 2 and n_obs[p] <= 2:
            v = BAD_BY_OBSERVATIONS
        elif cur - int(scene["first_kf_id"][p]) >= 3:
            v = ERASED_BY_AGE
        else:
            v = KEPT
        if v in (BAD_BY_RATIO, BAD_BY_OBSERVATIONS):
            bad[p] = True
        verdicts.append(v)
        path["verdicts"][v] += 1
    return dict(events=np.array(events, np.int32).reshape(-1, 2), bad=np.array(bad, np.uint8), n_obs=np.array(n_obs, np.int32),
                found=np.array(found, np.int32), visible=np.array(visible, np.int32), rebuilt=sorted(rebuilt),
                clouds={j: clouds[j] for j in sorted(rebuilt)}, verdicts=np.array(verdicts, np.uint8), counters=cnt,
                all_clouds=clouds, paths=path)


def paths(scene):
    return cull(scene)["paths"]
