/* plane_match_core.h — the arithmetic of PlaneMatcher::SearchMapByCoefficients / bMatchStatus (reference
 * src/PlaneMatcher.cpp:11-201, PointDistanceFromPlane :206-226) and Map::FlagMatchedPlanePoints (src/Map.cc:406-431), shared
 * by the host entries (plane_match.cpp) and the device batch (plane_match_kernels.hip) so that both produce the same bits.
 * Plain IEEE add / mul / compare in float, compiled with -ffp-contract=off on both sides; DESIGN.md section 12.
 *
 * Matrices are row-major: Tcw is 4x4 (16 floats), Rwc_MF 3x3. */
#ifndef DRFE_PLANE_MATCH_CORE_H
#define DRFE_PLANE_MATCH_CORE_H

#include "../../include/drfe.h"
#include "../../include/drfe_math.h"

/* the bits of PointDistanceFromPlane's start value 100 (exact in float): the result of an empty or all-skipped cloud */
#define PM_NO_DISTANCE_BITS 0x42C80000u

/* Frame::ComputePlaneWorldCoeff (src/Frame.cc:1311-1317): cv::transpose(mTcw, temp), then temp * coef.  temp is a plain
 * matrix, so the product carries no transpose flag and takes gemm's small-matrix float path as restated in manhattan_core.h
 * (float dot products in order, then (float)(t * 1 + 0 * 0), i.e. + 0.0f); unpinned. */
DRFE_HD void pm_world_coef(const float Tcw[16], const float c[4], float o[4])
{
    for (int r = 0; r < 4; r++) {
        const float d = Tcw[0 * 4 + r] * c[0] + Tcw[1 * 4 + r] * c[1] + Tcw[2 * 4 + r] * c[2] + Tcw[3 * 4 + r] * c[3];
        o[r] = d + 0.0f;
    }
}

/* Frame::ComputePlaneWorldCoeff_MF (src/Frame.cc:1318-1328): the same with the top-left 3x3 of temp replaced by Rwc_MF */
DRFE_HD void pm_world_coef_mf(const float Tcw[16], const float Rwc[9], const float c[4], float o[4])
{
    float T[16];
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) T[r * 4 + k] = (r < 3 && k < 3) ? Rwc[r * 3 + k] : Tcw[k * 4 + r];
    for (int r = 0; r < 4; r++) {
        const float d = T[r * 4 + 0] * c[0] + T[r * 4 + 1] * c[1] + T[r * 4 + 2] * c[2] + T[r * 4 + 3] * c[3];
        o[r] = d + 0.0f;
    }
}

/* angle = pM0 * pW0 + pM1 * pW1 + pM2 * pW2 in float, left to right */
DRFE_HD float pm_angle(const float pM[4], const float pW[4]) { return pM[0] * pW[0] + pM[1] * pW[1] + pM[2] * pW[2]; }

/* abs(a x + b y + c z + d) in float (std::abs(float): the reference files have `using namespace std`) */
DRFE_HD float pm_point_dis(const float p[4], float x, float y, float z) { return fabsf(p[0] * x + p[1] * y + p[2] * z + p[3]); }

/* PointDistanceFromPlane's per-point term as an unsigned key: the bits of the float distance for a point with z != 0 (NaN z
 * included), else the start value.  The distance is never negative, so its bits order like its value; a NaN distance has the
 * sign bit clear (fabsf) and bits above +inf, so `dis < res` rejecting NaN is the same as a u32 min ignoring it.  The
 * minimum over any order, capped at PM_NO_DISTANCE_BITS, is therefore the reference's result in float bits. */
DRFE_HD uint32_t pm_point_key(const float p[4], float x, float y, float z)
{
    if (z == 0.0f) return PM_NO_DISTANCE_BITS;
    const float d = pm_point_dis(p, x, y, z);
    uint32_t u;
    memcpy(&u, &d, 4);
    return u;
}

/* the key of a min-reduction back to PointDistanceFromPlane's double result */
DRFE_HD double pm_key_distance(uint32_t key)
{
    if (key > PM_NO_DISTANCE_BITS) key = PM_NO_DISTANCE_BITS;
    float d;
    memcpy(&d, &key, 4);
    return (double)d;
}

/* the association gate: (angle > aTh || angle < -aTh) */
DRFE_HD bool pm_gate(float angle, float aTh) { return angle > aTh || angle < -aTh; }

/* The decision for one frame plane over the map planes in vpMapPlanes order, from angle[j] (pm_angle) and key[j] (the
 * min-reduced pm_point_key of plane j's cloud, read only where pm_gate passes and the plane is not bad).  map / par / ver hold
 * the prior pointers on entry and are only overwritten on assignment.  Returns `found`. */
DRFE_HD bool pm_decide(const drfe_plane_match_params& P, const float* angle, const uint32_t* key, const uint8_t* bad, int n_map,
                       int32_t* map, int32_t* par, int32_t* ver)
{
    float ldTh = P.dTh, lverTh = P.verTh, lparTh = P.parTh;
    bool found = false;
    for (int j = 0; j < n_map; j++) {
        if (bad[j]) continue;
        const float a = angle[j];
        if (pm_gate(a, P.aTh)) {
            const double d = pm_key_distance(key[j]);
            if (d < (double)ldTh) {
                ldTh = (float)d;
                *map = j;
                found = true;
                continue;
            }
        }
        if (a > lparTh || a < -lparTh) {
            lparTh = fabsf(a);
            *par = j;
            continue;
        }
        if (a < lverTh && a > -lverTh) {
            lverTh = fabsf(a);
            *ver = j;
            continue;
        }
    }
    return found;
}

/* FlagMatchedPlanePoints' test of one map point: dis < 0.5 with dis the float distance widened to double */
DRFE_HD bool pm_flag_point(const float pM[4], float x, float y, float z) { return (double)pm_point_dis(pM, x, y, z) < 0.5; }

/* bMatchStatus' test of one matched plane: true when it makes the call return false.  fabs(float) is the float overload;
 * fabs(angle_MF) - 0.0005 is a double. */
DRFE_HD bool pm_status_fails(float angle, float angle_MF)
{
    const double a = (double)fabsf(angle), m = (double)fabsf(angle_MF);
    return a < m - 0.0005 && a > m - 0.05;
}

#endif
