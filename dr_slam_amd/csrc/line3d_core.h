/* line3d_core.h — the arithmetic of Frame::isLineGood (reference src/Frame.cc:481-558) and of the 3-D line lifting it calls
 * (src/LineExtractor.cpp: depthStdDev :1180, compPt3dCov :1196, extract3dline_mahdist :1266, verify3dLine :1362,
 * mah_dist3d_pt_line :1419, computeLine3d_svd :1157, projectPt3d2Ln3d :278).  Shared by the host entry (lines_3d.cpp) and the
 * device kernels (lines_3d_kernels.hip) so that both produce the same bits: plain IEEE add / mul / div / sqrt / floor in double,
 * compiled with -ffp-contract=off on both sides.  What the reference really computes, the two k_as_f64 modes and the eigen-solve
 * that stands for cv::SVD are described in lines_3d.cpp; the device side is DESIGN.md section 18.
 *
 * The loops of the reference are order-defined only where they add (computeLine3d_svd's sums) or pick a first index (the
 * extremes); those are stated here as steps - a term, a strict comparison - that the host walks over a vector and the device
 * over a wavefront's inlier mask. */
#ifndef DRFE_LINE3D_CORE_H
#define DRFE_LINE3D_CORE_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/drfe.h"
#include "../../include/drfe_math.h"
#include "ahc_math.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define L3_MAX_SAMPLES 51          /* j = 0 .. numSmp, numSmp <= 50 */
#define L3_MIN_POINTS 10           /* fewer lifted samples: the line is skipped and draws nothing */
#define L3_MAX_ITERATIONS 10       /* extract3dline_mahdist's maxIterNo: two rand() draws each */
#define L3_EPS 1e-10
#define L3_DIST_THRESH 1.5

struct L3P { double x, y, z; };
DRFE_HD L3P operator-(const L3P& a, const L3P& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
DRFE_HD L3P operator+(const L3P& a, const L3P& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
DRFE_HD L3P operator*(const L3P& a, double s) { return {a.x * s, a.y * s, a.z * s}; }
DRFE_HD double l3_dot(const L3P& a, const L3P& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
DRFE_HD double l3_norm(const L3P& a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }

/* RandomPoint3d: the position and DU = diag(1 / sqrt(w)) * U^T of its covariance */
struct L3Point {
    L3P pos;
    double DU[9];
};

/* cv::norm(Point2f) of start - end, and numSmp = min((int)len, 50); below 1 the reference divides 0 by 0: no sample.  The int
 * conversion as cvttsd2si: a length that is NaN or does not fit gives INT_MIN, no sample */
DRFE_HD int l3_num_samples(const drfe_keyline& kl, double* len)
{
    const float dxs = kl.start_point_x - kl.end_point_x, dys = kl.start_point_y - kl.end_point_y;
    *len = sqrt((double)dxs * dxs + (double)dys * dys);
    const int n = *len < 2147483648.0 ? (int)*len : (-2147483647 - 1);
    const double numSmp = (double)(n < 50 ? n : 50);
    return numSmp >= 1 ? (int)numSmp : 0;
}

/* sample j of numSmp along the key line, lifted: Point2f * double -> Point2f (saturate_cast<float> of the double product),
 * Point2f + Point2f, the bounds test, the integer-coordinate rule, the nearest-pixel depth and its d <= 0.01 skip */
DRFE_HD bool l3_sample(const drfe_keyline& kl, int j, int numSmp, const float* depth, int w, int h, size_t stride, float cx, float cy,
                       float invfx, float invfy, L3P* p)
{
    const double t = j / (double)numSmp;
    const float px = (float)((double)kl.start_point_x * (1 - t)) + (float)((double)kl.end_point_x * t);
    const float py = (float)((double)kl.start_point_y * (1 - t)) + (float)((double)kl.end_point_y * t);
    const double x = px, y = py;
    if (x < 0 || y < 0 || x >= w || y >= h) return false;
    int row, col;
    if (floor(x) == x && floor(y) == y) {
        col = (int)(x - 1); if (col < 0) col = 0;
        row = (int)(y - 1); if (row < 0) row = 0;
    } else { col = (int)x; row = (int)y; }
    const float d = depth[(size_t)row * stride + col];
    if ((double)d <= 0.01) return false;
    p->z = d;
    p->x = (double)((float)col - cx) * p->z * (double)invfx;
    p->y = (double)((float)row - cy) * p->z * (double)invfy;
    return true;
}

/* the focal length compPt3dCov reads: K.at<double>(0,0) on CV_32F storage is the bytes of (K[0], K[1]) */
DRFE_HD double l3_focal(const float* K, int k_as_f64)
{
    if (k_as_f64) return (double)K[0];
    union { float f[2]; double d; } u;
    u.f[0] = K[0]; u.f[1] = K[1];
    return u.d;
}

DRFE_HD double l3_depth_std_dev(double d) { return 0.00273 * d * d + 0.00074 * d + (-0.00058); }

/* compPt3dCov: cov0 = J0 * diag(1, 1, sigma^2) * J0^T as two plain 3x3 products (every term kept, so inf * 0 is NaN exactly
 * where OpenCV's gemm makes it), then DU = diag(1/sqrt(w)) * U^T from the decomposition of cov0 */
DRFE_HD L3Point l3_comp_pt3d_cov(const L3P& pt, double f)
{
    L3Point rp;
    rp.pos = pt;
    const double J[3][3] = {{pt.z / f, 0, pt.x / pt.z}, {0, pt.z / f, pt.y / pt.z}, {0, 0, 1}};
    const double s = l3_depth_std_dev(pt.z) * l3_depth_std_dev(pt.z);
    const double C[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, s}};
    double M[3][3], cov[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[i][j] = J[i][0] * C[0][j] + J[i][1] * C[1][j] + J[i][2] * C[2][j];
    bool finite = true;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            cov[i][j] = M[i][0] * J[j][0] + M[i][1] * J[j][1] + M[i][2] * J[j][2];
            finite = finite && __builtin_isfinite(cov[i][j]);
        }
    if (!finite) {   /* Jacobi SVD of a matrix with a NaN in every column: all singular values NaN -> DU all NaN */
        for (int i = 0; i < 9; i++) rp.DU[i] = __builtin_nan("");
        return rp;
    }
    double ev[3], Q[9];
    ahc_eig3(cov[0][0], cov[1][0], cov[2][0], cov[1][1], cov[2][1], cov[2][2], ev, Q);
    for (int i = 0; i < 3; i++) {            /* singular values descending = eigenvalues descending */
        const int e = 2 - i;
        const double ws = sqrt(ev[e]);
        for (int c = 0; c < 3; c++) rp.DU[i * 3 + c] = (1 / ws) * Q[e * 3 + c];
    }
    return rp;
}

/* mah_dist3d_pt_line, src/LineExtractor.cpp:1419-1470, term by term */
DRFE_HD double l3_mah_dist(const L3Point& pt, const L3P& q1, const L3P& q2)
{
    const double xa = q1.x, ya = q1.y, za = q1.z, xb = q2.x, yb = q2.y, zb = q2.z;
    const double c1 = pt.DU[0], c2 = pt.DU[1], c3 = pt.DU[2], c4 = pt.DU[3], c5 = pt.DU[4], c6 = pt.DU[5], c7 = pt.DU[6],
                 c8 = pt.DU[7], c9 = pt.DU[8];
    const double x1 = pt.pos.x, x2 = pt.pos.y, x3 = pt.pos.z;
    const double a1 = c1 * (x1 - xa) + c2 * (x2 - ya) + c3 * (x3 - za), b1 = c1 * (x1 - xb) + c2 * (x2 - yb) + c3 * (x3 - zb);
    const double a2 = c4 * (x1 - xa) + c5 * (x2 - ya) + c6 * (x3 - za), b2 = c4 * (x1 - xb) + c5 * (x2 - yb) + c6 * (x3 - zb);
    const double a3 = c7 * (x1 - xa) + c8 * (x2 - ya) + c9 * (x3 - za), b3 = c7 * (x1 - xb) + c8 * (x2 - yb) + c9 * (x3 - zb);
    const double term1 = a1 * b2 - a2 * b1, term2 = a1 * b3 - a3 * b1, term3 = a2 * b3 - a3 * b2;
    const double term4 = c1 * (x1 - xa) - c1 * (x1 - xb) + c2 * (x2 - ya) - c2 * (x2 - yb) + c3 * (x3 - za) - c3 * (x3 - zb);
    const double term5 = c4 * (x1 - xa) - c4 * (x1 - xb) + c5 * (x2 - ya) - c5 * (x2 - yb) + c6 * (x3 - za) - c6 * (x3 - zb);
    const double term6 = c7 * (x1 - xa) - c7 * (x1 - xb) + c8 * (x2 - ya) - c8 * (x2 - yb) + c9 * (x3 - za) - c9 * (x3 - zb);
    return sqrt((term1 * term1 + term2 * term2 + term3 * term3) / (term4 * term4 + term5 * term5 + term6 * term6));
}

DRFE_HD bool l3_is_inlier(const L3Point& pt, const L3P& q1, const L3P& q2) { return l3_mah_dist(pt, q1, q2) < L3_DIST_THRESH; }

/* random_unique's step k (include/LSDextractor.h:241-251) swaps indexes[k] with indexes[k + draw % (n - k)] */
DRFE_HD int l3_swap_with(int k, int draw, int n) { return k + (int)((size_t)draw % (size_t)(n - k)); }

/* extract3dline_mahdist's iteration bound and its early exit */
DRFE_HD int l3_max_iterations(int n)
{
    const int m = (int)(n * (n - 1) * 0.5);
    return m < L3_MAX_ITERATIONS ? m : L3_MAX_ITERATIONS;
}
DRFE_HD bool l3_enough(int inliers, int n) { return (double)(size_t)inliers > n * 0.6; }

DRFE_HD L3P l3_project_pt_to_line(const L3P& P, const L3P& mid, const L3P& drct)
{
    const L3P A = mid, B = mid + drct, AB = B - A, AP = P - A;
    return A + AB * (l3_dot(AB, AP) / l3_dot(AB, AB));
}

/* The two extremes of a walk in index order: `if (v < minv)` / `if (v > maxv)` from minv = 100, maxv = -100 and index 0, so the
 * first index of an extreme wins and a value that beats neither bound (or a NaN) leaves the first element chosen. */
struct L3Extremes {
    double minv = 100, maxv = -100;
    int lo = 0, hi = 0;
};
DRFE_HD void l3_extremes_step(L3Extremes& e, int i, double v)
{
    if (v < e.minv) { e.minv = v; e.lo = i; }
    if (v > e.maxv) { e.maxv = v; e.hi = i; }
}

/* verify3dLine, :1362-1417, after its extremes: C and D are the projections of the extreme inliers on the line AB; every inlier
 * falls into one of ten cells between them, and more than 7 cells must be populated */
struct L3Cells {
    L3P C, D;
    double cd;
};
DRFE_HD bool l3_cells_begin(const L3P& lo, const L3P& hi, const L3P& A, const L3P& B, L3Cells* g)
{
    g->C = l3_project_pt_to_line(lo, (A + B) * 0.5, B - A);
    g->D = l3_project_pt_to_line(hi, (A + B) * 0.5, B - A);
    g->cd = l3_norm(g->D - g->C);
    return !(g->cd < L3_EPS);
}
DRFE_HD unsigned l3_cell_of(const L3Cells& g, const L3P& p)
{
    const double lambda = fabs(l3_dot(p - g.C, g.D - g.C) / g.cd / g.cd);
    if (lambda >= 1) return 9;
    const unsigned c = (unsigned)floor(lambda * 10);
    return c < 9 ? c : 9;             /* lambda < 1: at most 9 already */
}
DRFE_HD bool l3_cells_pass(int populated) { return (double)populated / 10 > 0.7; }

/* computeLine3d_svd, :1157-1178: the mean from the ordered sum of the positions, the six scatter sums of the ordered
 * differences, the principal direction.  Host and device add the terms in inlier order. */
DRFE_HD L3P l3_mean(const L3P& sum, int n) { return sum * (1.0 / n); }
DRFE_HD void l3_scatter_add(double s[6], const L3P& d)
{
    s[0] += d.x * d.x; s[1] += d.y * d.x; s[2] += d.z * d.x; s[3] += d.y * d.y; s[4] += d.z * d.y; s[5] += d.z * d.z;
}
DRFE_HD L3P l3_direction(const double s[6])
{
    double ev[3], Q[9];
    ahc_eig3(s[0], s[1], s[2], s[3], s[4], s[5], ev, Q);
    return {Q[6], Q[7], Q[8]};      /* eigenvector of the largest eigenvalue = first right singular vector */
}

/* isLineGood's gates and the depth it stores: the smaller end-point depth (std::min(end, start)), -1 with an end point outside */
DRFE_HD bool l3_accept(int nInliers, double len, const L3P& A, const L3P& B) { return nInliers / len > 0.4 && l3_norm(A - B) > 0.02; }
DRFE_HD float l3_end_point_depth(const drfe_keyline& kl, const float* depth, int w, int h, size_t stride)
{
    const int ex = (int)kl.end_point_x, ey = (int)kl.end_point_y, sx = (int)kl.start_point_x, sy = (int)kl.start_point_y;
    const bool in = ex >= 0 && ex < w && ey >= 0 && ey < h && sx >= 0 && sx < w && sy >= 0 && sy < h;
    if (!in) return -1.0f;
    const float a = depth[(size_t)ey * stride + ex], b = depth[(size_t)sy * stride + sx];
    return b < a ? b : a;
}

#endif
