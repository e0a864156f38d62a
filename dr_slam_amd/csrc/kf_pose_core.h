/* kf_pose_core.h — what KeyFrame::SetPose (reference src/KeyFrame.cc:147-167) derives from Tcw, once, for the matchers' host
 * side (capi_match.cpp), the map store (lmap_correct.cpp, lmap_gba.cpp) and its kernels (correct_kernels.hip, gba_kernels.hip).  Plain IEEE float
 * mul / add, compiled with -ffp-contract=off on both sides. */
#ifndef DRFE_KF_POSE_CORE_H
#define DRFE_KF_POSE_CORE_H

#include "../../include/drfe_math.h"

/* KeyFrame::GetCameraCenter(): Ow = -Rwc*tcw with Rwc = Rcw.t() stored first (KeyFrame::SetPose, src/KeyFrame.cc:153-154), so
 * the product has no transpose flag and cv::gemm takes its small-matrix float path: float dot, then * alpha = -1 */
DRFE_HD void camera_centre_kf(const float* Tcw, float Ow[3])
{
    for (int i = 0; i < 3; i++) {
        const float d = Tcw[0 * 4 + i] * Tcw[3] + Tcw[1 * 4 + i] * Tcw[7] + Tcw[2 * 4 + i] * Tcw[11];
        Ow[i] = (float)((double)d * -1.0);
    }
}

/* Twc as SetPose leaves it: Rwc and Ow copied into eye(4) */
DRFE_HD void pose_inverse_kf(const float* Tcw, float Twc[16])
{
    float Ow[3];
    camera_centre_kf(Tcw, Ow);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Twc[r * 4 + c] = Tcw[c * 4 + r];
        Twc[r * 4 + 3] = Ow[r];
    }
    Twc[12] = 0.0f; Twc[13] = 0.0f; Twc[14] = 0.0f; Twc[15] = 1.0f;
}

#endif
