/* gba_core.h — the arithmetic of the map update after a global bundle adjustment (reference src/LoopClosing.cc:722-783), once, for
 * lmap_gba.cpp and gba_kernels.hip.  DESIGN.md section 29.  The float 4x4 product is correct_core.h's corr_gemm4, the inverse
 * SetPose keeps is kf_pose_core.h's pose_inverse_kf and the 3x4 map with a C term is triangulate_core.h's tr_twc_apply: plain IEEE
 * mul / add, compiled with -ffp-contract=off on both sides.  Parity with a build of the reference's LoopClosing.cc is not pinned. */
#ifndef DRFE_GBA_CORE_H
#define DRFE_GBA_CORE_H

#include "correct_core.h"
#include "triangulate_core.h"

/* what a point does in :749-783 */
enum { GBA_POINT_STAYS = 0, GBA_POINT_POS = 1, GBA_POINT_REF = 2 };

/* the state of section 29 by slot, next to LmapImage and CorrImage; the commit writes into it */
struct GbaImage {
    float* kfTcwGBA;               /* nK x 16: mTcwGBA */
    float* kfBef;                  /* nK x 16: mTcwBefGBA */
    int32_t* kfStamp;              /* nK: mnBAGlobalForKF as a handle */
    uint8_t* kfHasBef;             /* nK */
    const float* mpPosGBA;         /* nP x 3 */
    const int32_t* mpStamp;        /* nP */
};

/* :735-736 of one child whose stamp is not nLoopKF: Twc = pKF->GetPoseInverse() of the parent's pose before its SetPose,
 * Tchildc = pChild->GetPose() * Twc, mTcwGBA = Tchildc * pKF->mTcwGBA */
DRFE_HD void gba_compose(const float childTcw[16], const float parentTcw[16], const float parentGBA[16], float out[16])
{
    float Twc[16], Tchildc[16];
    pose_inverse_kf(parentTcw, Twc);
    corr_gemm4(childTcw, Twc, Tchildc);
    corr_gemm4(Tchildc, parentGBA, out);
}

/* :755-769 without the arithmetic: refStamp is the reference key frame's mnBAGlobalForKF after the walk over the key frames
 * (read only when the point's own stamp differs from loop) */
DRFE_HD int gba_point_kind(uint8_t bad, int32_t stamp, int32_t refStamp, int32_t loop)
{
    if (bad) return GBA_POINT_STAYS;
    if (stamp == loop) return GBA_POINT_POS;
    return refStamp == loop ? GBA_POINT_REF : GBA_POINT_STAYS;
}

/* :772-781: Xc = Rcw * X + tcw with mTcwBefGBA, then Rwc * Xc + twc with the inverse of the pose SetPose received */
DRFE_HD void gba_through_ref(const float bef[16], const float refTcw[16], const float X[3], float out[3])
{
    float Twc[16], Xc[3];
    tr_twc_apply(bef, X, Xc);
    pose_inverse_kf(refTcw, Twc);
    tr_twc_apply(Twc, Xc, out);
}

/* the point rule: the kind, and the new position when it is not GBA_POINT_STAYS.  bef and refTcw are read for kind 2 only. */
DRFE_HD int gba_point(uint8_t bad, int32_t stamp, int32_t refStamp, int32_t loop, const float posGBA[3], const float X[3],
                      const float* bef, const float* refTcw, float out[3])
{
    const int kind = gba_point_kind(bad, stamp, refStamp, loop);
    if (kind == GBA_POINT_POS) {
        out[0] = posGBA[0]; out[1] = posGBA[1]; out[2] = posGBA[2];
    } else if (kind == GBA_POINT_REF) {
        gba_through_ref(bef, refTcw, X, out);
    }
    return kind;
}

#endif
