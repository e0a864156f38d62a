/* plane_cull_core.h — the arithmetic and the integer bookkeeping of LocalMapping::MapPlaneCulling (reference
 * src/LocalMapping.cc:233-307) with Map::PointDistanceFromPlane (src/Map.cc:433-448) and MapPlane::Replace
 * (src/MapPlane.cc:197-271), shared by the host entry (plane_cull.cpp) and the device batch (plane_cull_kernels.hip) so that
 * both produce the same bits.  Plain IEEE mul / add / compare, compiled with -ffp-contract=off on both sides; DESIGN.md
 * section 30. */
#ifndef DRFE_PLANE_CULL_CORE_H
#define DRFE_PLANE_CULL_CORE_H

#include "plane_match_core.h"

/* the gate (:255): angle is a float, aTh a double (Config::Get<double>), so both compares happen in double.  PlaneMatcher's
 * aTh is a float (pm_gate); with 0.985 the two differ at angle == (float)0.985, which is above 0.985. */
DRFE_HD bool pc_gate(float angle, double aTh) { return (double)angle > aTh || (double)angle < -aTh; }

/* Map::PointDistanceFromPlane's per-point term as an unsigned key: the bits of abs(a x + b y + c z + d) in float.  Unlike
 * PlaneMatcher::PointDistanceFromPlane (pm_point_key) there is no z != 0 skip.  Ordering, NaN and the cap at the start value
 * 100 are those of pm_point_key / pm_key_distance. */
DRFE_HD uint32_t pc_point_key(const float p[4], float x, float y, float z)
{
    const float d = pm_point_dis(p, x, y, z);
    uint32_t u;
    memcpy(&u, &d, 4);
    return u;
}

/* The j loop of row i (:241-263) over angle[j] and key[j] (the min-reduced pc_point_key of plane j's cloud at that moment,
 * read only where both planes are alive and the gate passes): float ldTh = dTh narrows once, `dis < ldTh` compares a double
 * with a widened float, strictly, so the first of equal distances wins.  Returns bestIdx or -1. */
DRFE_HD int pc_decide_row(double dTh, double aTh, const float* angle, const uint32_t* key, const uint8_t* bad, int i, int n)
{
    int best = -1;
    float ldTh = (float)dTh;
    if (bad[i]) return -1;
    for (int j = i + 1; j < n; j++) {
        if (bad[j] || !pc_gate(angle[j], aTh)) continue;
        const double dis = pm_key_distance(key[j]);
        if (dis < (double)ldTh) {
            ldTh = (float)dis;
            best = j;
        }
    }
    return best;
}

/* which of the pair is replaced (:271-274): pMP2 when pMP1 has strictly more observations, else pMP1 */
DRFE_HD bool pc_first_survives(int n_obs1, int n_obs2) { return n_obs1 > n_obs2; }

/* Replace's walk over the replaced plane's mObservations (:218-234), both sets in key-frame rank order (std::map<KeyFrame*>):
 * the survivor takes an observation unless it is already in that key frame (IsInKeyFrame), in which case the key frame's
 * match is erased.  Writes the merged set (rank order, at most nd + ns entries) and returns its size; *added = the
 * AddObservation calls that counted (nObs += *added). */
DRFE_HD int pc_merge_observations(const int32_t* dkf, const int32_t* didx, int nd, const int32_t* skf, const int32_t* sidx, int ns,
                                  int32_t* okf, int32_t* oidx, int* added)
{
    int a = 0, b = 0, n = 0, add = 0;
    while (a < nd || b < ns) {
        if (b >= ns || (a < nd && dkf[a] < skf[b])) {
            okf[n] = dkf[a]; oidx[n] = didx[a]; n++; a++; add++;
        } else {
            if (a < nd && dkf[a] == skf[b]) a++;           /* a shared key frame: the survivor keeps its own match */
            okf[n] = skf[b]; oidx[n] = sidx[b]; n++; b++;
        }
    }
    *added = add;
    return n;
}

/* MapPlane::GetFoundRatio (src/MapPlane.cc:292-296): static_cast<float>(mnFound) / mnVisible, the int converted to float */
DRFE_HD float pc_found_ratio(int found, int visible) { return (float)found / (float)visible; }

/* the verdict of one entry of mlpRecentAddedMapPlanes (:289-306); nThObs is 2 on both branches */
DRFE_HD int pc_recent_verdict(bool bad, int found, int visible, int n_obs, int first_kf_id, int current_kf_id)
{
    if (bad) return DRFE_PLANE_CULL_ERASED_BAD;
    if (pc_found_ratio(found, visible) < 0.25f) return DRFE_PLANE_CULL_BAD_BY_RATIO;
    const long long age = (long long)current_kf_id - (long long)first_kf_id;
    if (age >= 2 && n_obs <= 2) return DRFE_PLANE_CULL_BAD_BY_OBSERVATIONS;
    if (age >= 3) return DRFE_PLANE_CULL_ERASED_BY_AGE;
    return DRFE_PLANE_CULL_KEPT;
}

/* the key arrays of the device pass hold pair (i, j), i < j, column-major: column j's j entries are contiguous */
DRFE_HD int pc_pair_index(int i, int j) { return j * (j - 1) / 2 + i; }

#endif
