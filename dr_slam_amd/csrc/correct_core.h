/* correct_core.h — the arithmetic of LoopClosing::CorrectLoop's Sim3 propagation (reference src/LoopClosing.cc:480-562), once,
 * for lmap_correct.cpp and correct_kernels.hip.  DESIGN.md section 27.  g2o::Sim3 is sim3_opt_core.h's restatement, the quaternion
 * pieces are map_plane_core.h's, UpdateNormalAndDepth is map_upkeep_core.h's and SetPose's centre is kf_pose_core.h's: plain IEEE
 * add / mul / div / sqrt, compiled with -ffp-contract=off on both sides; no sin, cos or exp.
 *
 * Key frames are slots in rank order and a call's key frames are positions 0 .. n in rank order (the iteration order of
 * map<KeyFrame*, g2o::Sim3>); points are slots of their own. */
#ifndef DRFE_CORRECT_CORE_H
#define DRFE_CORRECT_CORE_H

#include "sim3_opt_core.h"
#include "map_upkeep_core.h"
#include "kf_pose_core.h"

/* the geometry of the store's image, next to LmapImage; the commit writes into it */
struct CorrImage {
    int32_t nLevels;
    const float* scale;            /* nLevels: mvScaleFactors */
    float* kfTcw;                  /* nK x 16: what SetPose last received */
    float* kfOw;                   /* nK x 3: camera_centre_kf of it */
    float* mpWorld;                /* nP x 3 */
    const int32_t* mpRef;          /* nP: slot of the reference key frame */
    const int32_t* mpLevel;        /* nP */
    int32_t* mpBy;                 /* nP: mnCorrectedByKF as a handle */
    int32_t* mpByRef;              /* nP: mnCorrectedReference as a handle */
};

/* what one called key frame gets: CorrectedSim3, NonCorrectedSim3, the inverse the points use, the new pose and its centre */
struct CorrKf {
    SoSim3 corrected, nonCorrected, swi;
    float Tiw[16];
    float Ow[3];
    int32_t pad;
};

/* g2o::Sim3 from double[8]: coeffs x y z w, t, s */
DRFE_HD void corr_sim3_from8(const double v[8], SoSim3& S)
{
    for (int k = 0; k < 4; k++) S.q[k] = v[k];
    for (int k = 0; k < 3; k++) S.t[k] = v[4 + k];
    S.s = v[7];
}
DRFE_HD void corr_sim3_to8(const SoSim3& S, double v[8])
{
    for (int k = 0; k < 4; k++) v[k] = S.q[k];
    for (int k = 0; k < 3; k++) v[4 + k] = S.t[k];
    v[7] = S.s;
}

/* cv::Mat Tic = Tiw * Twc of two float 4x4: gemm's small-matrix path, four float products summed left to right, then
 * (float)(t * alpha) with alpha = 1 */
DRFE_HD void corr_gemm4(const float A[16], const float B[16], float D[16])
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            const float t = A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c] + A[r * 4 + 2] * B[8 + c] + A[r * 4 + 3] * B[12 + c];
            D[r * 4 + c] = (float)((double)t * 1.0);
        }
}

/* g2o::Sim3(toMatrix3d(T.rowRange(0,3).colRange(0,3)), toVector3d(T.rowRange(0,3).col(3)), 1.0) */
DRFE_HD void corr_sim3_of_pose(const float T[16], SoSim3& S)
{
    const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    const float t[3] = {T[3], T[7], T[11]};
    so_from_pose(R, t, S);
}

/* :497-514 and :521-558 of one key frame: Tiw as stored, TwcCur = mpCurrentKF->GetPoseInverse() before the call */
DRFE_HD void corr_keyframe(const float Tiw[16], bool isCur, const float TwcCur[16], const SoSim3& Scw, CorrKf& K)
{
    corr_sim3_of_pose(Tiw, K.nonCorrected);
    if (isCur) {
        K.corrected = Scw;
    } else {
        float Tic[16];
        SoSim3 Sic;
        corr_gemm4(Tiw, TwcCur, Tic);
        corr_sim3_of_pose(Tic, Sic);
        so_mul(Sic, Scw, K.corrected);
    }
    so_inverse(K.corrected, K.swi);
    /* toCvSE3(r.toRotationMatrix(), t * (1. / s)): doubles cast to float */
    double R[3][3];
    mp_quat_to_matrix(K.corrected.q, R);
    const double inv = 1.0 / K.corrected.s;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) K.Tiw[r * 4 + c] = (float)R[r][c];
        K.Tiw[r * 4 + 3] = (float)(K.corrected.t[r] * inv);
    }
    K.Tiw[12] = 0.0f; K.Tiw[13] = 0.0f; K.Tiw[14] = 0.0f; K.Tiw[15] = 1.0f;
    camera_centre_kf(K.Tiw, K.Ow);
    K.pad = 0;
}

/* toCvMat(g2oCorrectedSwi.map(g2oSiw.map(toVector3d(P3Dw)))) */
DRFE_HD void corr_point(const SoSim3& Siw, const SoSim3& Swi, const float X[3], float Xn[3])
{
    const double v[3] = {(double)X[0], (double)X[1], (double)X[2]};
    double a[3], b[3];
    so_map(Siw, v, a);
    so_map(Swi, a, b);
    for (int k = 0; k < 3; k++) Xn[k] = (float)b[k];
}

/* the test of the walk (:530-535) */
DRFE_HD bool corr_entry_moves(int32_t p, const uint8_t* mpBad, const int32_t* mpBy, int32_t cur)
{
    return p >= 0 && !mpBad[p] && mpBy[p] != cur;
}

/* A key frame read by the UpdateNormalAndDepth of a point that position j claims has had its SetPose exactly when it is a called
 * key frame strictly before j; the claimant's own SetPose comes after its points. */
DRFE_HD bool corr_centre_is_new(int32_t posOfKf, int32_t j) { return posOfKf >= 0 && posOfKf < j; }

/* UpdateNormalAndDepth of a point that position j moved to Xn.  pos: nK, position in the call or -1; kfs: the call's CorrKf by
 * position.  Returns DRFE_UPKEEP_NORMAL, or 0 when the point has no observations and nothing is computed. */
DRFE_HD uint8_t corr_normal(const CorrImage& G, const int32_t* obsOff, const int32_t* obs, const int32_t* pos, const CorrKf* kfs,
                            int32_t p, int32_t j, const float Xn[3], float nrm[3], float* maxD, float* minD)
{
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
    *maxD = *minD = 0.0f;
    const int32_t o0 = obsOff[p], o1 = obsOff[p + 1];
    if (o1 == o0) return 0;
    for (int32_t o = o0; o < o1; o++) {
        const int32_t s = obs[o], q = pos[s];
        mu_point_obs(nrm, Xn, corr_centre_is_new(q, j) ? kfs[q].Ow : G.kfOw + 3 * (size_t)s);
    }
    const int32_t r = G.mpRef[p], q = pos[r];
    mu_point_finish(nrm, o1 - o0, Xn, corr_centre_is_new(q, j) ? kfs[q].Ow : G.kfOw + 3 * (size_t)r, G.scale[G.mpLevel[p]],
                    G.scale[G.nLevels - 1], maxD, minD);
    return DRFE_UPKEEP_NORMAL;
}

#endif
