/* create_core.h — the rules of map-point and map-line creation (the tail of LocalMapping::CreateNewMapPoints and
 * CreateNewMapLines2, reference src/LocalMapping.cc:522-535, :1019-1031, with MapPoint::AddObservation and UpdateNormalAndDepth,
 * src/MapPoint.cc:124-138, :376-417), once, for lmap_create.cpp.  DESIGN.md section 34.
 *
 * A new item has no stored observers, so its observer list is the call's own 1 or 2 observations: a second one on the key frame of
 * the first is no observer, and two of them stand in ascending slot, which is rank order.  The arithmetic of UpdateNormalAndDepth
 * is map_upkeep_core.h's, as insert_core.h uses it. */
#ifndef DRFE_CREATE_CORE_H
#define DRFE_CREATE_CORE_H

#include "correct_core.h"
#include "fuse_core.h"

/* The observers a creation keeps, in list order: kf and idx are the call's 2 entries in slots, n its count.  Writes oKf, oIdx and
 * returns how many there are. */
DRFE_HD int32_t create_observers(int32_t n, const int32_t kf[2], const int32_t idx[2], int32_t oKf[2], int32_t oIdx[2])
{
    oKf[0] = kf[0];
    oIdx[0] = idx[0];
    if (n < 2 || kf[1] == kf[0]) return 1;
    const int first = kf[1] < kf[0] ? 1 : 0;   /* in front of the first listed observer of greater slot */
    oKf[0] = kf[first];
    oIdx[0] = idx[first];
    oKf[1] = kf[1 - first];
    oIdx[1] = idx[1 - first];
    return 2;
}

/* the index a creation observes key frame `ref` with, among its m kept observers, or -1 */
DRFE_HD int32_t create_ref_index(int32_t m, const int32_t oKf[2], const int32_t oIdx[2], int32_t ref)
{
    for (int32_t t = 0; t < m; t++)
        if (oKf[t] == ref) return oIdx[t];
    return -1;
}

/* UpdateNormalAndDepth of a created point at X over its m kept observers in list order; kfOw and scale as CorrImage holds them */
DRFE_HD uint8_t create_point_normal(const float* kfOw, const float* scale, int32_t nLevels, const float X[3], int32_t m,
                                    const int32_t oKf[2], int32_t ref, int32_t level, float nrm[3], float* maxD, float* minD)
{
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
    for (int32_t t = 0; t < m; t++) mu_point_obs(nrm, X, kfOw + 3 * (size_t)oKf[t]);
    mu_point_finish(nrm, m, X, kfOw + 3 * (size_t)ref, scale[level], scale[nLevels - 1], maxD, minD);
    return DRFE_UPKEEP_NORMAL;
}

#endif
