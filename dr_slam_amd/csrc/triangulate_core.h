/* triangulate_core.h — the per-match arithmetic of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:383-538)
 * and CreateNewMapLines2 (:875-1026), RGB-D / stereo branch, with KeyFrame::UnprojectStereo and obtain3DLine
 * (src/KeyFrame.cc:788-815).  Shared by the host entries (triangulate.cpp) and the device kernels (triangulate_kernels.hip) so
 * that both produce the same bits; plain IEEE add / mul / div / sqrt, compiled with -ffp-contract=off on both sides.  The
 * SVD is the shared drfe_jacobi_svd<4>; cos and atan2 are drfe_math.h's correctly rounded drfe_cosf / drfe_atan2f.  The
 * OpenCV readings are DESIGN.md section 15 (unpinned, as sections 11 and 14). */
#ifndef DRFE_TRIANGULATE_CORE_H
#define DRFE_TRIANGULATE_CORE_H

#include "../../include/drfe.h"
#include "../../include/drfe_math.h"
#include "jacobi_svd_core.h"

#include <stdint.h>

/* The inputs of one call as flat arrays (host pointers or their staged device copies). */
struct TriView {
    const drfe_tri_keyframe* kf;
    const float *scale, *sigma2;       /* n_keyframes x nLevels */
    int nLevels;
    const int32_t* off;                /* n_keyframes + 1 feature offsets */
    /* points */
    const float *un, *raw, *uRight, *depth;
    /* lines */
    const float *ends, *depthLine;
    const double* lines3d;
    const int32_t* octave;
};

/* Mat::dot of two float 3-vectors: double products summed in order */
DRFE_HD double tr_dotd(const float* a, const float* b)
{
    double s = 0.0;
    s += (double)a[0] * (double)b[0];
    s += (double)a[1] * (double)b[1];
    s += (double)a[2] * (double)b[2];
    return s;
}

/* (float)cv::norm(a - b) of two float 3-vectors: the float difference, the double sum of squares in order, sqrt */
DRFE_HD float tr_dist(const float* a, const float* b)
{
    const float d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
    return (float)sqrt(tr_dotd(d, d));
}

/* Rwc * x with Rwc = Rcw.t() materialised, through gemm's small-matrix path: float dots, then (float)(t * 1 + 0 * 0) */
DRFE_HD void tr_rwc_mul(const float Tcw[12], const float x[3], float o[3])
{
    for (int r = 0; r < 3; r++) {
        const float t = Tcw[0 * 4 + r] * x[0] + Tcw[1 * 4 + r] * x[1] + Tcw[2 * 4 + r] * x[2];
        o[r] = (float)((double)t * 1.0 + 0.0 * 0.0);
    }
}

/* Twc.rowRange(0,3).colRange(0,3) * x + Twc.rowRange(0,3).col(3): one gemm with a C term, float dots, then
 * (float)(t * 1 + c * 1) */
DRFE_HD void tr_twc_apply(const float Twc[12], const float x[3], float o[3])
{
    for (int r = 0; r < 3; r++) {
        const float t = Twc[r * 4 + 0] * x[0] + Twc[r * 4 + 1] * x[1] + Twc[r * 4 + 2] * x[2];
        o[r] = (float)((double)t * 1.0 + (double)Twc[r * 4 + 3] * 1.0);
    }
}

/* Rcw.row(r).dot(X) + tcw.at<float>(r), stored to float */
DRFE_HD float tr_row(const float Tcw[12], int r, const float X[3])
{
    return (float)(tr_dotd(Tcw + r * 4, X) + (double)Tcw[r * 4 + 3]);
}

/* A.row(q) = s * Tcw.row(a) - Tcw.row(b): MatExpr's AddEx(alpha = s, beta = -1) assigned through cv::addWeighted in double
 * (per element (float)(a * s + b * -1 + 0)), or cv::subtract in float when s == 1 exactly */
DRFE_HD void tr_arow(float s, const float* ra, const float* rb, float* o)
{
    for (int k = 0; k < 4; k++)
        o[k] = s == 1.0f ? ra[k] - rb[k] : (float)((double)ra[k] * (double)s + (double)rb[k] * -1.0 + 0.0);
}

/* (x * x + y * y [+ r * r]) in float against c * sigma2 in double */
DRFE_HD bool tr_reproj_bad(const drfe_tri_keyframe& K, const float* Tcw, const float X[3], float z, float kx, float ky, float sigma2,
                           bool stereo, float mbf, float ur)
{
    const float x = tr_row(Tcw, 0, X), y = tr_row(Tcw, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = K.fx * x * invz + K.cx;
    const float v = K.fy * y * invz + K.cy;
    const float ex = u - kx, ey = v - ky;
    if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    const float u_r = u - mbf * invz;
    const float er = u_r - ur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

/* cv::norm(Ow2 - Ow1) < pKF2->mb: the pair is skipped */
DRFE_HD bool tr_pair_skipped(const drfe_tri_keyframe& K1, const drfe_tri_keyframe& K2)
{
    return tr_dist(K2.Ow, K1.Ow) < K2.mb;
}

/* KeyFrame::UnprojectStereo(i) (mvDepth[i] > 0: the entries reject a stereo keypoint without depth) */
DRFE_HD void tr_unproject(const TriView& V, const drfe_tri_keyframe& K, int g, float X[3])
{
    const float z = V.depth[g];
    const float u = V.raw[2 * (size_t)g], v = V.raw[2 * (size_t)g + 1];
    const float xc[3] = {(u - K.cx) * z * K.invfx, (v - K.cy) * z * K.invfy, z};
    tr_twc_apply(K.Twc, xc, X);
}

/* The parallax test and the branch of a point match (keypoints g1 of kf1, g2 of kf2, global indices): DRFE_TRI_BRANCH_*; 0
 * when neither triangulation nor stereo applies */
DRFE_HD int tr_point_branch(const TriView& V, int f1, int f2, int g1, int g2)
{
    const drfe_tri_keyframe &K1 = V.kf[f1], &K2 = V.kf[f2];
    const bool st1 = V.uRight[g1] >= 0, st2 = V.uRight[g2] >= 0;
    const float xn1[3] = {(V.un[2 * (size_t)g1] - K1.cx) * K1.invfx, (V.un[2 * (size_t)g1 + 1] - K1.cy) * K1.invfy, 1.0f};
    const float xn2[3] = {(V.un[2 * (size_t)g2] - K2.cx) * K2.invfx, (V.un[2 * (size_t)g2 + 1] - K2.cy) * K2.invfy, 1.0f};
    float ray1[3], ray2[3];
    tr_rwc_mul(K1.Tcw, xn1, ray1);
    tr_rwc_mul(K2.Tcw, xn2, ray2);
    const float cosRays = (float)(tr_dotd(ray1, ray2) / (sqrt(tr_dotd(ray1, ray1)) * sqrt(tr_dotd(ray2, ray2))));
    const float cosStereo0 = cosRays + 1;
    float cos1 = cosStereo0, cos2 = cosStereo0;
    if (st1) cos1 = drfe_cosf(2 * drfe_atan2f(K1.mb / 2, V.depth[g1]));
    else if (st2) cos2 = drfe_cosf(2 * drfe_atan2f(K2.mb / 2, V.depth[g2]));
    const float cosStereo = cos2 < cos1 ? cos2 : cos1;             /* std::min */
    if (cosRays < cosStereo && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) return DRFE_TRI_BRANCH_SVD;
    if (st1 && cos1 < cos2) return DRFE_TRI_BRANCH_STEREO1;
    if (st2 && cos2 < cos1) return DRFE_TRI_BRANCH_STEREO2;
    return DRFE_TRI_BRANCH_NONE;
}

/* Linear triangulation: A's four rows, cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV), vt.row(3); false when x3D(3) == 0.
 * x3D.rowRange(0,3) / w is convertTo with the scale (float)(1.0 / w) and cvtScale's zero shift, or a plain copy when that
 * scale is exactly 1 (convertTo's noScale). */
DRFE_HD bool tr_point_svd(const TriView& V, int f1, int f2, int g1, int g2, float X[3])
{
    const drfe_tri_keyframe &K1 = V.kf[f1], &K2 = V.kf[f2];
    const float xn10 = (V.un[2 * (size_t)g1] - K1.cx) * K1.invfx, xn11 = (V.un[2 * (size_t)g1 + 1] - K1.cy) * K1.invfy;
    const float xn20 = (V.un[2 * (size_t)g2] - K2.cx) * K2.invfx, xn21 = (V.un[2 * (size_t)g2 + 1] - K2.cy) * K2.invfy;
    float A[16];
    tr_arow(xn10, K1.Tcw + 8, K1.Tcw + 0, A + 0);
    tr_arow(xn11, K1.Tcw + 8, K1.Tcw + 4, A + 4);
    tr_arow(xn20, K2.Tcw + 8, K2.Tcw + 0, A + 8);
    tr_arow(xn21, K2.Tcw + 8, K2.Tcw + 4, A + 12);
    float At[16], Vt[16];
    double W[4];
    for (int i = 0; i < 4; i++)
        for (int k = 0; k < 4; k++) At[i * 4 + k] = A[k * 4 + i];
    drfe_jacobi_svd<4>(At, W, Vt);
    const float w = Vt[15];
    if (w == 0) return false;
    const double sd = 1.0 / (double)w;
    const float a = (float)sd;
    for (int k = 0; k < 3; k++) X[k] = sd == 1.0 ? Vt[12 + k] : Vt[12 + k] * a + 0.0f;
    return true;
}

/* The gates after the point X (in front of both cameras, reprojection in KF1 then KF2, zero distance, scale consistency):
 * DRFE_TRI_ACCEPTED or the code of the `continue` that fired */
DRFE_HD int tr_point_gates(const TriView& V, int f1, int f2, int g1, int g2, const float X[3])
{
    const drfe_tri_keyframe &K1 = V.kf[f1], &K2 = V.kf[f2];
    const float z1 = tr_row(K1.Tcw, 2, X);
    if (z1 <= 0) return DRFE_TRI_Z1;
    const float z2 = tr_row(K2.Tcw, 2, X);
    if (z2 <= 0) return DRFE_TRI_Z2;
    const int o1 = V.octave[g1], o2 = V.octave[g2];
    const float ur1 = V.uRight[g1], ur2 = V.uRight[g2];
    if (tr_reproj_bad(K1, K1.Tcw, X, z1, V.un[2 * (size_t)g1], V.un[2 * (size_t)g1 + 1], V.sigma2[f1 * V.nLevels + o1], ur1 >= 0,
                      K1.mbf, ur1))
        return DRFE_TRI_REPROJ1;
    /* KF2's stereo residual uses KF1's mbf, as the reference */
    if (tr_reproj_bad(K2, K2.Tcw, X, z2, V.un[2 * (size_t)g2], V.un[2 * (size_t)g2 + 1], V.sigma2[f2 * V.nLevels + o2], ur2 >= 0,
                      K1.mbf, ur2))
        return DRFE_TRI_REPROJ2;
    const float dist1 = tr_dist(X, K1.Ow), dist2 = tr_dist(X, K2.Ow);
    if (dist1 == 0 || dist2 == 0) return DRFE_TRI_DIST;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = V.scale[f1 * V.nLevels + o1] / V.scale[f2 * V.nLevels + o2];
    const float ratioFactor = 1.5f * K1.scale_factor;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return DRFE_TRI_SCALE;
    return DRFE_TRI_ACCEPTED;
}

/* One point match */
DRFE_HD int tr_point(const TriView& V, int f1, int f2, int g1, int g2, float X[3], int* branch)
{
    const int br = tr_point_branch(V, f1, f2, g1, g2);
    *branch = br;
    if (br == DRFE_TRI_BRANCH_NONE) return DRFE_TRI_NO_PARALLAX;
    if (br == DRFE_TRI_BRANCH_SVD) {
        if (!tr_point_svd(V, f1, f2, g1, g2, X)) return DRFE_TRI_W_ZERO;
    } else if (br == DRFE_TRI_BRANCH_STEREO1) {
        tr_unproject(V, V.kf[f1], g1, X);
    } else {
        tr_unproject(V, V.kf[f2], g2, X);
    }
    return tr_point_gates(V, f1, f2, g1, g2, X);
}

/* KeyFrame::obtain3DLine(i): the double endpoints rounded to float, through Twc (one gemm with a C term each) */
DRFE_HD void tr_obtain_line(const TriView& V, const drfe_tri_keyframe& K, int g, float sp[3], float ep[3])
{
    const double* L = V.lines3d + 6 * (size_t)g;
    const float a[3] = {(float)L[0], (float)L[1], (float)L[2]}, b[3] = {(float)L[3], (float)L[4], (float)L[5]};
    tr_twc_apply(K.Twc, a, sp);
    tr_twc_apply(K.Twc, b, ep);
}

/* One line match (idx2 is the match's index in KF2; q2 is KF1's line idx2 as a global index, or -1 when idx2 is past KF1's
 * lines: the reference reads out of bounds there, the entries take bStereo2 = false and flag the match) */
DRFE_HD int tr_line(const TriView& V, int f1, int f2, int g1, int g2, int q2, float sp[3], float ep[3], int* branch)
{
    const drfe_tri_keyframe &K1 = V.kf[f1], &K2 = V.kf[f2];
    const int flag = q2 < 0 ? DRFE_TRI_IDX2_PAST_KF1 : 0;
    const bool st1 = V.depthLine[g1] > 0;
    const bool st2 = q2 >= 0 && V.depthLine[q2] > 0;            /* KF1's mvDepthLine[idx2], as the reference */
    *branch = DRFE_TRI_BRANCH_NONE;
    if (st1) { *branch = DRFE_TRI_BRANCH_STEREO1; tr_obtain_line(V, K1, g1, sp, ep); }
    else if (st2) { *branch = DRFE_TRI_BRANCH_STEREO2; tr_obtain_line(V, K2, g2, sp, ep); }
    else return DRFE_TRI_NO_PARALLAX | flag;
    const float zsp1 = tr_row(K1.Tcw, 2, sp);
    if (zsp1 <= 0) return DRFE_TRI_L_Z_SP1 | flag;
    const float zep1 = tr_row(K1.Tcw, 2, ep);
    if (zep1 <= 0) return DRFE_TRI_L_Z_EP1 | flag;
    const float zsp2 = tr_row(K2.Tcw, 2, sp);
    if (zsp2 <= 0) return DRFE_TRI_L_Z_SP2 | flag;
    const float zep2 = tr_row(K2.Tcw, 2, ep);
    if (zep2 <= 0) return DRFE_TRI_L_Z_EP2 | flag;
    const int o1 = V.octave[g1], o2 = V.octave[g2];
    const float s1 = V.sigma2[f1 * V.nLevels + o1], s2 = V.sigma2[f2 * V.nLevels + o2];
    const float* e1 = V.ends + 4 * (size_t)g1;
    const float* e2 = V.ends + 4 * (size_t)g2;
    if (tr_reproj_bad(K1, K1.Tcw, sp, zsp1, e1[0], e1[1], s1, false, 0.f, 0.f)) return DRFE_TRI_L_REPROJ_SP1 | flag;
    if (tr_reproj_bad(K1, K1.Tcw, ep, zep1, e1[2], e1[3], s1, false, 0.f, 0.f)) return DRFE_TRI_L_REPROJ_EP1 | flag;
    if (tr_reproj_bad(K2, K2.Tcw, sp, zsp2, e2[0], e2[1], s2, false, 0.f, 0.f)) return DRFE_TRI_L_REPROJ_SP2 | flag;
    if (tr_reproj_bad(K2, K2.Tcw, ep, zep2, e2[2], e2[3], s2, false, 0.f, 0.f)) return DRFE_TRI_L_REPROJ_EP2 | flag;
    const float dsp1 = tr_dist(sp, K1.Ow), dep1 = tr_dist(ep, K1.Ow), dsp2 = tr_dist(sp, K2.Ow), dep2 = tr_dist(ep, K2.Ow);
    if (dsp1 == 0 || dep1 == 0 || dsp2 == 0 || dep2 == 0) return DRFE_TRI_L_DIST | flag;
    const float rsp = dsp2 / dsp1, rep = dep2 / dep1;
    const float ratioOctave = V.scale[f1 * V.nLevels + o1] / V.scale[f2 * V.nLevels + o2];
    const float ratioFactor = 1.5f * K1.scale_factor;
    if (rsp * ratioFactor < ratioOctave || rsp > ratioOctave * ratioFactor || rep * ratioFactor < ratioOctave ||
        rep > ratioOctave * ratioFactor)
        return DRFE_TRI_L_SCALE | flag;
    return DRFE_TRI_ACCEPTED | flag;
}

#endif
