/* manhattan_core.h — the arithmetic of Tracking::TrackManhattanFrame (reference src/Tracking.cc:1055-1266, 1336-1546),
 * shared by the host entry (manhattan.cpp) and the device batch entry (manhattan_kernels.hip) so that both produce the
 * same bits.  Plain IEEE add / mul / div / sqrt, compiled with -ffp-contract=off on both sides; asin, exp and tan(float)
 * are the canonical drfe_asin / drfe_exp / drfe_tanf of drfe_math.h.  The semantics and the OpenCV pieces restated here
 * (cv::SVD of a 3x3 CV_32F, determinant, Mat::cross, small-matrix gemm, Mat / double, cv::norm, cv::sum) are written down
 * in DESIGN.md section 11; the OpenCV pieces are unpinned.
 *
 * Matrices are row-major float[9].  "M" is the reference's R_mc_new of axis a (1..3): the transpose of R_cm with its
 * columns permuted to ((a+3)%3, (a+4)%3, (a+5)%3), so row k of M is column c_k of R_cm. */
#ifndef DRFE_MANHATTAN_CORE_H
#define DRFE_MANHATTAN_CORE_H

#include "../../include/drfe_math.h"
#include "jacobi_svd_core.h"

DRFE_HD void mf_axis_rows(const float R[9], int a, float M[9])
{
    const int c[3] = {(a + 3) % 3, (a + 4) % 3, (a + 5) % 3};
    for (int k = 0; k < 3; k++)
        for (int r = 0; r < 3; r++) M[k * 3 + r] = R[r * 3 + c[k]];
}

/* n_ini of a SurfaceNormal: cv::Point3f from float products and float sums (src/Tracking.cc:1232-1240) */
DRFE_HD void mf_nini_normal(const float M[9], const float n[3], float o[3])
{
    for (int k = 0; k < 3; k++) o[k] = M[k * 3] * n[0] + M[k * 3 + 1] * n[1] + M[k * 3 + 2] * n[2];
}

/* n_ini of a FrameLine direction (cv::Point3d): float * double products, double sums, stored to float (:1254-1262) */
DRFE_HD void mf_nini_line(const float M[9], const double d[3], float o[3])
{
    for (int k = 0; k < 3; k++)
        o[k] = (float)((double)M[k * 3] * d[0] + (double)M[k * 3 + 1] * d[1] + (double)M[k * 3 + 2] * d[2]);
}

/* lambda = sqrt(float) (the float overload: `using namespace std`), widened to double */
DRFE_HD double mf_lambda(const float o[3]) { return (double)sqrtf(o[0] * o[0] + o[1] * o[1]); }

/* m_j of ProjectSN2MF (:1101-1108) for a point whose lambda passed the mean-shift cone; false when m_j is NaN (the point
 * is then not selected, but it was still pushed to the frame's axis list).  lambda == 0 gives 0 / 0: dropped. */
DRFE_HD bool mf_mj(double lambda, const float o[3], double* mx, double* my)
{
    const double tan_alfa = lambda / (double)fabsf(o[2]);
    const double alfa = drfe_asin(lambda);
    *mx = alfa / tan_alfa * (double)o[0] / (double)o[2];
    *my = alfa / tan_alfa * (double)o[1] / (double)o[2];
    return !(*mx != *mx) && !(*my != *my);
}

/* MeanShift's per-point terms (:1536-1541): k = exp(-20 * |m| * |m|), then k * x and k * y */
DRFE_HD void mf_weight(double mx, double my, double w[3])
{
    const double nm = sqrt(mx * mx + my * my);
    const double k = drfe_exp(-20.0 * nm * nm);
    w[0] = k * mx;
    w[1] = k * my;
    w[2] = k;
}

/* The end of ProjectSN2MF once m_j_selected.size() > numOfSN (:1143-1164), from MeanShift's three sequential sums:
 * s_j = nominator / denominator, density = float(denominator / n), alfa = float(norm(s_j)), ma = float(tanf(alfa) / alfa *
 * s_j), R_cm_Rec = R_mc.t() * [ma_x, ma_y, 1]^T (small-matrix gemm: float dots, then (float)(t * 1 + 0 * 0)), divided by its
 * cv::norm (double sum of squares; Mat / double scales by (float)(1.0 / norm) through convertTo).  Returns whether
 * sum(R_cm_Rec)[0] != 0 (a double sum), the reference's test for "axis found". */
DRFE_HD bool mf_axis_tail(const float M[9], double sx, double sy, double sk, int n, float col[3], float* density)
{
    const double cx = sx / sk, cy = sy / sk;
    *density = (float)(sk / (double)n);
    const float alfa = (float)sqrt(cx * cx + cy * cy);
    const float ta = drfe_tanf(alfa) / alfa;
    const float ma_x = (float)((double)ta * cx), ma_y = (float)((double)ta * cy);
    float v[3];
    for (int r = 0; r < 3; r++) {            /* rtemp = M^T: rtemp[r][k] = M[k][r] */
        const float d = M[0 * 3 + r] * ma_x + M[1 * 3 + r] * ma_y + M[2 * 3 + r] * 1.0f;
        v[r] = d + 0.0f;
    }
    double s2 = 0.0;
    for (int r = 0; r < 3; r++) s2 += (double)v[r] * (double)v[r];
    const float inv = (float)(1.0 / sqrt(s2));
    for (int r = 0; r < 3; r++) col[r] = v[r] * inv;
    double sum = 0.0;
    for (int r = 0; r < 3; r++) sum += (double)col[r];
    return sum != 0.0;
}

/* cv::determinant of a 3x3 CV_32F: the det3 macro in float, returned as double */
DRFE_HD float mf_det3(const float m[9])
{
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

/* cv::Mat::cross of two CV_32F 3-vectors */
DRFE_HD void mf_cross(const float a[3], const float b[3], float c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

/* cv::SVD::compute(A, W, U, VT) of a 3x3 CV_32F (JacobiSVDImpl_<float>, m = n = n1 = 3, minval = FLT_MIN,
 * eps = 2 * FLT_EPSILON, at most 30 sweeps; At = A^T: the shared drfe_jacobi_svd<3>), then U * VT through the small-matrix
 * gemm (float dots, + 0). */
DRFE_HD void mf_svd_polar(float R[9])
{
    const float eps = 2.0f * 1.1920928955078125e-07f;
    const double minval = 1.17549435082228750797e-38;
    float At[9], Vt[9];
    double W[3];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) At[i * 3 + k] = R[k * 3 + i];
    drfe_jacobi_svd<3>(At, W, Vt);
    /* left singular vectors; a singular value <= FLT_MIN gets cv::RNG(0x12345678)'s random vector, orthogonalised */
    uint64_t rng = 0x12345678u;
    for (int i = 0; i < 3; i++) {
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / 3);
            for (int k = 0; k < 3; k++) {
                rng = (uint64_t)(unsigned)rng * 4164903690u + (unsigned)(rng >> 32);
                At[i * 3 + k] = (((unsigned)rng) & 256) != 0 ? val0 : -val0;
            }
            for (int it = 0; it < 2; it++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < 3; k++) sd += At[i * 3 + k] * At[j * 3 + k];
                    float asum = 0;
                    for (int k = 0; k < 3; k++) {
                        const float t = (float)(At[i * 3 + k] - sd * At[j * 3 + k]);
                        At[i * 3 + k] = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < 3; k++) At[i * 3 + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < 3; k++) { const float t = At[i * 3 + k]; sd += (double)t * t; }
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
        for (int k = 0; k < 3; k++) At[i * 3 + k] *= s;
    }
    /* U = At^T; R = U * VT */
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const float d = At[0 * 3 + r] * Vt[0 * 3 + c] + At[1 * 3 + r] * Vt[1 * 3 + c] + At[2 * 3 + r] * Vt[2 * 3 + c];
            R[r * 3 + c] = d + 0.0f;
        }
}

/* The end of TrackManhattanFrame's single pass (:1443-1516) on R, which already holds the columns of the axes found
 * (R_cm and R_cm_update share one buffer: `cv::Mat R_cm = R_cm_update` copies the header).  Fewer than 2 axes: R is
 * returned as it stands, no SVD.  Exactly 2: the third column is their cross product in the reference's operand order,
 * negated when |det + 1| < 0.5.  Then R = U * VT.  The acos(...) < 0.001 test (:1511) sits inside a loop that runs once
 * and only decides whether to leave it early, so it changes nothing and is not computed.  Returns whether the SVD ran. */
DRFE_HD bool mf_assemble(float R[9], int found)
{
    const int nf = (found & 1) + ((found >> 1) & 1) + ((found >> 2) & 1);
    if (nf < 2) return false;
    if (nf == 2) {
        int ia, ib, ic;                     /* third column ic = col(ia) x col(ib) */
        if ((found & 3) == 3) { ia = 0; ib = 1; ic = 2; }
        else if ((found & 6) == 6) { ia = 2; ib = 1; ic = 0; }
        else { ia = 0; ib = 2; ic = 1; }
        const float va[3] = {R[ia], R[3 + ia], R[6 + ia]}, vb[3] = {R[ib], R[3 + ib], R[6 + ib]};
        float vc[3];
        mf_cross(va, vb, vc);
        for (int r = 0; r < 3; r++) R[r * 3 + ic] = vc[r];
        if (fabs((double)mf_det3(R) + 1) < 0.5)
            for (int r = 0; r < 3; r++) R[r * 3 + ic] = -vc[r];
    }
    mf_svd_polar(R);
    return true;
}

#endif
