/* recent_core.h — the rules of LocalMapping::MapPointCulling and MapLineCulling (reference src/LocalMapping.cc:175-231) on the
 * local-map store, stated once for the host walk (lmap_recent.cpp) and the kernels (recent_kernels.hip).  DESIGN.md section 31.
 *
 * Three facts carry the device entry:
 *   1. The verdict of a list entry reads its own item only (bad flag, mnFound, mnVisible, mnFirstKFid, nObs), and SetBadFlag of
 *      another item writes none of those.  So every verdict can be taken from the state the call found, all at once.
 *   2. The one coupling inside a list is a handle that stands in it twice: the first occurrence of a culled item carries the
 *      verdict, every later one finds it bad.  The lowest list position of a culled item is an atomicMin on a claim word.
 *   3. SetBadFlag stores null at (observer, index) for every observation it holds, whatever stands there.  The stores of distinct
 *      culled items are all the same value, so their order does not show. */
#ifndef DRFE_RECENT_CORE_H
#define DRFE_RECENT_CORE_H

#include "../../include/drfe_math.h"
#include <stdint.h>

/* what became of a list entry */
enum { RECENT_KEPT = 0, RECENT_WAS_BAD = 1, RECENT_RATIO = 2, RECENT_OBS = 3, RECENT_AGED = 4 };
/* the two kinds of a call, and of an entry of the flat entry space: the point list first, then the line list */
enum { RECENT_POINT = 0, RECENT_LINE = 1 };

/* MapPoint::GetFoundRatio() < 0.25f: static_cast<float>(mnFound) / mnVisible, one correctly rounded float division.  visible == 0
 * gives inf or NaN, and NaN is not less. */
DRFE_HD bool recent_point_ratio(int32_t found, int32_t visible)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn((float)found, (float)visible) < 0.25f;
#else
    return (float)found / (float)visible < 0.25f;
#endif
}

/* MapLine::GetFoundRatio() divides the integers; these are the two cases in which that division is not defined */
DRFE_HD bool recent_line_undefined(int32_t found, int32_t visible) { return visible == 0 || (found == INT32_MIN && visible == -1); }

/* static_cast<float>(mnFound / mnVisible) < 0.25f, for a line that is not recent_line_undefined */
DRFE_HD bool recent_line_ratio(int32_t found, int32_t visible) { return (float)(found / visible) < 0.25f; }

/* (int)mpCurrentKeyFrame->mnId - (int)mnFirstKFid: both truncated to int as written, the difference in 64 bits */
DRFE_HD int64_t recent_age(int64_t current, int64_t first)
{
    return (int64_t)(int32_t)(uint32_t)(uint64_t)current - (int64_t)(int32_t)(uint32_t)(uint64_t)first;
}

/* the verdict of an item that is not bad, from the values the call found: RECENT_KEPT, _RATIO, _OBS or _AGED */
DRFE_HD int recent_verdict(int kind, int32_t found, int32_t visible, int64_t first, int32_t nObs, int64_t current, int monocular)
{
    if (kind == RECENT_POINT ? recent_point_ratio(found, visible) : recent_line_ratio(found, visible)) return RECENT_RATIO;
    const int64_t age = recent_age(current, first);
    if (age >= 2 && nObs <= (monocular ? 2 : 3)) return RECENT_OBS;
    if (age >= 3) return RECENT_AGED;
    return RECENT_KEPT;
}

DRFE_HD bool recent_culls(int action) { return action == RECENT_RATIO || action == RECENT_OBS; }

#endif
