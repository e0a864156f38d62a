/* pose_opt_core.h — the arithmetic of Optimizer::PoseOptimization (reference src/Optimizer.cc:601-1338) and of what g2o runs
 * under it, restated statement by statement: the unary edges, Huber's kernel, the 6x6 normal equations and
 * VertexSE3Expmap::oplusImpl; Eigen's LDLT and the Levenberg step control are lm_core.h's.  Shared by the host entry (pose_opt.cpp) and the device kernel
 * (pose_opt_kernels.hip) so that both produce the same bits: plain IEEE add / mul / div / sqrt in double, compiled with
 * -ffp-contract=off on both sides; sin, cos and the two cubes through cr_sincos.h / cr_cube.h.  DESIGN.md section 20 states the
 * evaluation order of every expression; where Eigen leaves an association open it is read left to right.
 *
 * An edge is evaluated by one lane (the twelve perturbations of a plane edge's numeric Jacobian by up to twelve).  What is summed over edges (H, b, the robust chi2) is summed by the caller, edge after edge in
 * active-edge order; po_edge_terms gives the 27 terms of one edge.  The step control (PoLM) runs in one lane. */
#ifndef DRFE_POSE_OPT_CORE_H
#define DRFE_POSE_OPT_CORE_H

#include <float.h>
#include <math.h>
#include <stdint.h>
#include "map_plane_core.h"
#include "lm_core.h"
#include "cr_atan2.h"

enum { PO_MONO = 0, PO_STEREO = 1, PO_LINE = 2, PO_PLANE = 3, PO_PAR_PLANE = 4, PO_VER_PLANE = 5 };
enum { PO_H_TERMS = 21, PO_TERMS = 27 };        /* the lower triangle of H, row by row, then b */

/* one edge as staged:
 *   a point      obs = u, v, uRight; X = the map point, floats widened; info = invSigma2 widened, three times
 *   a line end   obs = the line function; X = the end point; info = 1
 *   a plane      obs = the measured Plane3D (Converter::toPlane3D of mvPlaneCoefficients[i]); X = the map plane's Plane3D;
 *                info = angleInfo, angleInfo, disInfo (matched) or parInfo / verInfo twice
 * delta is Huber's delta, a float widened by setDelta(double); th the classification's threshold widened to double (a float
 * for points and line ends, the double Plane.Chi / Plane.VPChi for planes). */
struct PoEdge {
    double obs[4];
    double X[4];
    double info[3];
    double delta, th;
    int32_t kind, pad;
};

/* a frame's camera: fx fy cx cy bf, floats widened as the reference's `e->fx = pFrame->fx` does */
struct PoCam { double fx, fy, cx, cy, bf; };

DRFE_HD int po_dim(int kind) { return (kind == PO_MONO || kind == PO_PAR_PLANE || kind == PO_VER_PLANE) ? 2 : 3; }
DRFE_HD int po_is_plane(int kind) { return kind >= PO_PLANE; }

/* the point and line constants of src/Optimizer.cc:634-635, 1049-1050, 1160 */
DRFE_HD double po_delta_mono() { return (double)(float)sqrt(5.991); }
DRFE_HD double po_delta_stereo() { return (double)(float)sqrt(7.815); }
DRFE_HD double po_th_mono() { return (double)5.991f; }
DRFE_HD double po_th_stereo() { return (double)7.815f; }
DRFE_HD double po_th_line() { return (double)(2 * 5.991f); }

/* the transcendentals (the cube is lm_core.h's): correctly rounded, or the host's libm where the certificate fails, or ctx.fail.
 * sin and cos of any |x| < 64: sin is odd, cos even, exactly */
DRFE_HD void po_sincos(LmCtx& ctx, double x, double* sn, double* cs)
{
    const double ax = fabs(x);
    double s = 0.0, c = 1.0;
    if (!(ax <= DBL_MAX)) { *sn = NAN; *cs = NAN; return; }   /* NaN and the infinities, as sin / cos */
    if (!drfe_cr_sincos(ax, &s, &c)) {
#if !defined(__HIP_DEVICE_COMPILE__)
        if (ctx.libm) { s = sin(ax); c = cos(ax); }
        else
#endif
            ctx.fail = 1;
    }
    *sn = x < 0.0 ? -s : s;
    *cs = c;
}

/* atan2 of any y: odd in y, exactly (atan2(-0, x) = -atan2(+0, x)) */
DRFE_HD double po_atan2(LmCtx& ctx, double y, double x)
{
    const int neg = y == y && signbit(y);
    double r;
    if (!drfe_cr_atan2(neg ? -y : y, x, &r)) {
#if !defined(__HIP_DEVICE_COMPILE__)
        if (ctx.libm) r = atan2(neg ? -y : y, x);
        else
#endif
            ctx.fail = 1;
    }
    return neg ? -r : r;
}

/* Eigen 3.3.7 Quaternion::_transformVector, then SE3Quat::map's `+ _t`: uv = 2 (q.vec x v); (v + w uv) + q.vec x uv; + t */
DRFE_HD void po_map(const double q[4], const double t[3], const double v[3], double o[3])
{
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int k = 0; k < 3; k++) o[k] = ((v[k] + q[3] * uv[k]) + c[k]) + t[k];
}

/* ---- Plane3D (g2oAddition/Plane3D.h) ---- */

/* Plane3D::normalize: coeffs * (1 / |n|), then the four negated when d < 0 */
DRFE_HD void po_plane_normalize(double c[4])
{
    const double n = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    const double inv = 1.0 / n;
    for (int k = 0; k < 4; k++) c[k] = c[k] * inv;
    if (c[3] < 0.0)
        for (int k = 0; k < 4; k++) c[k] = -c[k];
}

/* Converter::toPlane3D (src/Converter.cc:182-191): the floats widened, negated when the float d < 0, Plane3D(V) */
DRFE_HD void po_to_plane3d(const float coe[4], double c[4])
{
    for (int k = 0; k < 4; k++) c[k] = (double)coe[k];
    if (coe[3] < 0.0f)
        for (int k = 0; k < 4; k++) c[k] = -c[k];
    po_plane_normalize(c);
}

/* Plane3D::rotation(v): (AngleAxisd(azimuth, Z) * AngleAxisd(-elevation, Y)).toRotationMatrix().  AngleAxis * AngleAxis is the
 * product of their quaternions (w = cos(angle / 2), vec = sin(angle / 2) * axis, the zeros of the axes multiplied through),
 * Eigen's generic quat_product, not normalised */
DRFE_HD void po_plane_rotation(LmCtx& ctx, const double v[3], double R[3][3])
{
    const double az = po_atan2(ctx, v[1], v[0]);
    const double el = po_atan2(ctx, v[2], sqrt(v[0] * v[0] + v[1] * v[1]));
    double s1, c1, s2, c2;
    po_sincos(ctx, 0.5 * az, &s1, &c1);
    po_sincos(ctx, 0.5 * (-el), &s2, &c2);
    const double ax = s1 * 0.0, ay = s1 * 0.0, az_ = s1 * 1.0, aw = c1;
    const double bx = s2 * 0.0, by = s2 * 1.0, bz = s2 * 0.0, bw = c2;
    double q[4];
    q[3] = ((aw * bw - ax * bx) - ay * by) - az_ * bz;
    q[0] = ((aw * bx + ax * bw) + ay * bz) - az_ * by;
    q[1] = ((aw * by + ay * bw) + az_ * bx) - ax * bz;
    q[2] = ((aw * bz + az_ * bw) + ax * by) - ay * bx;
    mp_quat_to_matrix(q, R);
}

/* R^T m, then (azimuth, elevation) of it: the tail of ominus, ominus_par and ominus_ver */
DRFE_HD void po_plane_angles(LmCtx& ctx, const double nor[3], const double m[3], double e[2])
{
    double R[3][3], n[3];
    po_plane_rotation(ctx, nor, R);
    for (int i = 0; i < 3; i++) n[i] = (R[0][i] * m[0] + R[1][i] * m[1]) + R[2][i] * m[2];
    e[0] = po_atan2(ctx, n[1], n[0]);
    e[1] = po_atan2(ctx, n[2], sqrt(n[0] * n[0] + n[1] * n[1]));
}

/* computeError of EdgePlaneOnlyPose / EdgeParallelPlaneOnlyPose / EdgeVerticalPlaneOnlyPose: localPlane = Isometry3D(estimate) *
 * Xw (operator*, Plane3D.h:189-202; rotation() of an isometry is its linear part), then ominus / ominus_par / ominus_ver of the
 * measurement */
DRFE_HD void po_plane_ominus(LmCtx& ctx, const PoEdge& E, double l[4], const double t[3], double e[3]);
DRFE_HD void po_plane_error(LmCtx& ctx, const PoEdge& E, const double q[4], const double t[3], double e[3])
{
    double R[3][3], l[4];
    mp_quat_to_matrix(q, R);
    for (int i = 0; i < 3; i++) l[i] = (R[i][0] * E.X[0] + R[i][1] * E.X[1]) + R[i][2] * E.X[2];
    po_plane_ominus(ctx, E, l, t, e);
}

/* what follows the normal l[0..2] of the local plane, shared with the translation-only plane edges (trans_opt_core.h, whose
 * operator+ leaves the normal as it is): d - t . n, the four negated below zero, the Plane3D constructor, then the edge's ominus */
DRFE_HD void po_plane_ominus(LmCtx& ctx, const PoEdge& E, double l[4], const double t[3], double e[3])
{
    l[3] = E.X[3] - ((t[0] * l[0] + t[1] * l[1]) + t[2] * l[2]);
    if (l[3] < 0.0)
        for (int k = 0; k < 4; k++) l[k] = -l[k];
    po_plane_normalize(l);
    const double* m = E.obs;
    e[2] = 0.0;
    if (E.kind == PO_PLANE) {
        po_plane_angles(ctx, l, m, e);
        e[2] = (-l[3]) - (-m[3]);
    } else if (E.kind == PO_PAR_PLANE) {
        double nor[3] = {l[0], l[1], l[2]};
        if ((m[0] * nor[0] + m[1] * nor[1]) + m[2] * nor[2] < 0.0)
            for (int k = 0; k < 3; k++) nor[k] = -nor[k];
        po_plane_angles(ctx, nor, m, e);
    } else {
        /* v = n x m; AngleAxisd(M_PI / 2, v / |v|) * n is AngleAxis::toRotationMatrix() * n; sin(M_PI / 2) rounds to 1 and
         * cos(M_PI / 2) to 0x1.1a62633145c07p-54 */
        const double v[3] = {l[1] * m[2] - l[2] * m[1], l[2] * m[0] - l[0] * m[2], l[0] * m[1] - l[1] * m[0]};
        const double nv = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        const double ax[3] = {v[0] / nv, v[1] / nv, v[2] / nv};
        const double sn = 1.0, c = 0x1.1a62633145c07p-54;
        const double sa[3] = {sn * ax[0], sn * ax[1], sn * ax[2]};
        const double ca[3] = {(1.0 - c) * ax[0], (1.0 - c) * ax[1], (1.0 - c) * ax[2]};
        double A[3][3], tmp;
        tmp = ca[0] * ax[1]; A[0][1] = tmp - sa[2]; A[1][0] = tmp + sa[2];
        tmp = ca[0] * ax[2]; A[0][2] = tmp + sa[1]; A[2][0] = tmp - sa[1];
        tmp = ca[1] * ax[2]; A[1][2] = tmp - sa[0]; A[2][1] = tmp + sa[0];
        for (int k = 0; k < 3; k++) A[k][k] = ca[k] * ax[k] + c;
        double b[3];
        for (int i = 0; i < 3; i++) b[i] = (A[i][0] * l[0] + A[i][1] * l[1]) + A[i][2] * l[2];
        po_plane_angles(ctx, b, m, e);
    }
}

/* computeError of the edge under the estimate (q, t); e[2] of a mono edge is not read and set to 0 */
DRFE_HD void po_project_error(const PoEdge& E, const PoCam& C, const double p[3], double e[3]);
DRFE_HD void po_edge_error(LmCtx& ctx, const PoEdge& E, const PoCam& C, const double q[4], const double t[3], double e[3])
{
    if (po_is_plane(E.kind)) { po_plane_error(ctx, E, q, t, e); return; }
    double p[3];
    po_map(q, t, E.X, p);
    po_project_error(E, C, p, e);
}

/* the measurement less cam_project of the camera point p, of a point or line edge: shared with the translation-only edges */
DRFE_HD void po_project_error(const PoEdge& E, const PoCam& C, const double p[3], double e[3])
{
    if (E.kind == PO_STEREO) {
        /* EdgeStereoSE3ProjectXYZOnlyPose::cam_project: `const float invz = 1.0f / trans_xyz[2]` divides in double, rounds to float */
        const double invz = (double)(float)(1.0 / p[2]);
        const double r0 = (p[0] * invz) * C.fx + C.cx;
        const double r1 = (p[1] * invz) * C.fy + C.cy;
        const double r2 = r0 - C.bf * invz;
        e[0] = E.obs[0] - r0; e[1] = E.obs[1] - r1; e[2] = E.obs[2] - r2;
        return;
    }
    const double r0 = (p[0] / p[2]) * C.fx + C.cx;
    const double r1 = (p[1] / p[2]) * C.fy + C.cy;
    if (E.kind == PO_MONO) {
        e[0] = E.obs[0] - r0; e[1] = E.obs[1] - r1; e[2] = 0.0;
    } else {                                       /* EdgeLineProjectXYZOnlyPose (include/EdgeLine.h:161-168) */
        e[0] = (E.obs[0] * r0 + E.obs[1] * r1) + E.obs[2];
        e[1] = 0.0; e[2] = 0.0;
    }
}

/* BaseEdge::chi2: _error.dot(information() * _error), the information the D x D diag(info) with its zeros multiplied through */
DRFE_HD double po_chi2(const PoEdge& E, const double e[3])
{
    const int D = po_dim(E.kind);
    const double* info = E.info;
    double s = 0.0;
    for (int i = 0; i < D; i++) {
        double w = 0.0;
        for (int j = 0; j < D; j++) {
            const double term = (i == j ? info[i] : 0.0) * e[j];
            w = j == 0 ? term : w + term;
        }
        const double term = e[i] * w;
        s = i == 0 ? term : s + term;
    }
    return s;
}

/* RobustKernelHuber::robustify; `float dsqr = delta * delta` (robust_kernel_impl.h:84) */
DRFE_HD void po_huber(double chi2, double delta, double* rho0, double* rho1)
{
    const float dsqr = (float)(delta * delta);
    if (chi2 <= (double)dsqr) {
        *rho0 = chi2; *rho1 = 1.0;
    } else {
        const double sqrte = sqrt(chi2);
        *rho0 = (2.0 * sqrte) * delta - (double)dsqr;
        *rho1 = delta / sqrte;
    }
}

/* an edge's term of activeRobustChi2 */
DRFE_HD double po_chi_term(const PoEdge& E, const double e[3], int robust)
{
    const double chi2 = po_chi2(E, e);
    if (!robust) return chi2;
    double r0, r1;
    po_huber(chi2, E.delta, &r0, &r1);
    return r0;
}

/* linearizeOplus of the three analytic edges at the estimate (q, t): J is D x 6, rows past D unused */
DRFE_HD void po_edge_jacobian(const PoEdge& E, const PoCam& C, const double q[4], const double t[3], double J[3][6])
{
    double p[3];
    po_map(q, t, E.X, p);
    const double x = p[0], y = p[1];
    const double invz = 1.0 / p[2];
    const double invz_2 = invz * invz;
    const double fx = C.fx, fy = C.fy;
    if (E.kind == PO_LINE) {
        const double lx = E.obs[0], ly = E.obs[1];
        J[0][0] = ((-fy) * ly - (((fx * lx) * x) * y) * invz_2) - (((fy * ly) * y) * y) * invz_2;
        J[0][1] = (fx * lx + (((fx * lx) * x) * x) * invz_2) + (((fy * ly) * x) * y) * invz_2;
        J[0][2] = (((-fx) * lx) * y) * invz + ((fy * ly) * x) * invz;
        J[0][3] = (fx * lx) * invz;
        J[0][4] = (fy * ly) * invz;
        J[0][5] = (-(((fx * lx) * x) + ((fy * ly) * y))) * invz_2;
        for (int c = 0; c < 6; c++) { J[1][c] = 0.0; J[2][c] = 0.0; }
        return;
    }
    J[0][0] = ((x * y) * invz_2) * fx;
    J[0][1] = (-(1.0 + ((x * x) * invz_2))) * fx;
    J[0][2] = (y * invz) * fx;
    J[0][3] = (-invz) * fx;
    J[0][4] = 0.0;
    J[0][5] = (x * invz_2) * fx;
    J[1][0] = (1.0 + (y * y) * invz_2) * fy;
    J[1][1] = (((-x) * y) * invz_2) * fy;
    J[1][2] = ((-x) * invz) * fy;
    J[1][3] = 0.0;
    J[1][4] = (-invz) * fy;
    J[1][5] = (y * invz_2) * fy;
    if (E.kind == PO_STEREO) {
        const double bf = C.bf;
        J[2][0] = J[0][0] - (bf * y) * invz_2;
        J[2][1] = J[0][1] + (bf * x) * invz_2;
        J[2][2] = J[0][2];
        J[2][3] = J[0][3];
        J[2][4] = 0.0;
        J[2][5] = J[0][5] - bf * invz_2;
    } else {
        for (int c = 0; c < 6; c++) J[2][c] = 0.0;
    }
}

/* BaseUnaryEdge::constructQuadraticForm of one edge: term[r (r + 1) / 2 + c] is what the edge adds to H(r, c), c <= r (the
 * triangle Eigen's LDLT reads), term[21 + r] what it takes from b(r).
 *   with a kernel: W = rho1 Omega; b -= ((rho1 A^T) Omega) e; H += (A^T W) A
 *   without:       b -= (A^T Omega) e;                        H += (A^T Omega) A
 * each product a temporary, each element a sum over the inner index from 0 up. */
DRFE_HD void po_edge_terms(const PoEdge& E, const double J[3][6], const double e[3], int robust, double term[PO_TERMS])
{
    const int D = po_dim(E.kind);
    double rho1 = 1.0;
    if (robust) {
        double r0;
        po_huber(po_chi2(E, e), E.delta, &r0, &rho1);
    }
    double T[6][3], Tb[6][3];
    for (int i = 0; i < 6; i++)
        for (int k = 0; k < D; k++) {
            double s = 0.0, sb = 0.0;
            for (int m = 0; m < D; m++) {
                const double om = m == k ? E.info[m] : 0.0;
                const double w = robust ? rho1 * om : om;
                const double a = J[m][i] * w;
                const double ab = robust ? (rho1 * J[m][i]) * om : J[m][i] * om;
                s = m == 0 ? a : s + a;
                sb = m == 0 ? ab : sb + ab;
            }
            T[i][k] = s;
            Tb[i][k] = sb;
        }
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j <= i; j++) {
            double s = 0.0;
            for (int k = 0; k < D; k++) {
                const double a = T[i][k] * J[k][j];
                s = k == 0 ? a : s + a;
            }
            term[i * (i + 1) / 2 + j] = s;
        }
        double s = 0.0;
        for (int k = 0; k < D; k++) {
            const double a = Tb[i][k] * e[k];
            s = k == 0 ? a : s + a;
        }
        term[PO_H_TERMS + i] = s;
    }
}

/* VertexSE3Expmap::oplusImpl: estimate = SE3Quat::exp(u) * estimate (types/se3quat.h:227-261, :104-110) */
DRFE_HD int po_oplus(LmCtx& ctx, double q[4], double t[3], const double u[6])
{
    const double o0 = u[0], o1 = u[1], o2 = u[2];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double Om[3][3] = {{0.0, -o2, o1}, {o2, 0.0, -o0}, {-o1, o0, 0.0}};
    double Om2[3][3], R[3][3], V[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Om2[r][c] = (Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c];
    const int small = theta < 0.00001;
    if (small) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                R[r][c] = ((r == c ? 1.0 : 0.0) + Om[r][c]) + Om2[r][c];
                V[r][c] = R[r][c];
            }
    } else {
        double sn, cs;
        po_sincos(ctx, theta, &sn, &cs);
        const double a = sn / theta;
        const double bq = (1.0 - cs) / (theta * theta);
        const double cq = (theta - sn) / lm_cube(ctx, theta);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                const double id = r == c ? 1.0 : 0.0;
                R[r][c] = (id + a * Om[r][c]) + bq * Om2[r][c];
                V[r][c] = (id + bq * Om[r][c]) + cq * Om2[r][c];
            }
    }
    double eq[4], et[3];
    mp_quat_from_matrix(R, eq);
    mp_quat_normalize_rotation(eq);
    for (int r = 0; r < 3; r++) et[r] = (V[r][0] * u[3] + V[r][1] * u[4]) + V[r][2] * u[5];
    /* SE3Quat::operator*: t = et + eq * t (no `+ t` inside the rotation), r = eq * r (Eigen's generic quat_product), normalizeRotation */
    {
        const double* v = t;
        double uv[3] = {eq[1] * v[2] - eq[2] * v[1], eq[2] * v[0] - eq[0] * v[2], eq[0] * v[1] - eq[1] * v[0]};
        for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
        const double c[3] = {eq[1] * uv[2] - eq[2] * uv[1], eq[2] * uv[0] - eq[0] * uv[2], eq[0] * uv[1] - eq[1] * uv[0]};
        double nt[3];
        for (int k = 0; k < 3; k++) nt[k] = et[k] + ((v[k] + eq[3] * uv[k]) + c[k]);
        for (int k = 0; k < 3; k++) t[k] = nt[k];
    }
    {
        const double ax = eq[0], ay = eq[1], az = eq[2], aw = eq[3];
        const double bx = q[0], by = q[1], bz = q[2], bw = q[3];
        double nq[4];
        nq[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
        nq[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
        nq[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
        nq[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
        mp_quat_normalize_rotation(nq);
        for (int k = 0; k < 4; k++) q[k] = nq[k];
    }
    return small;
}

/* BaseUnaryEdge::linearizeOplus, the numeric Jacobian of the plane edges (core/base_unary_edge.hpp:82-123): perturbation
 * (d, side) is computeError at exp(+-1e-9 e_d) * estimate, side 0 the plus step; column d = (1 / 2e-9) * (plus - minus).  The
 * estimate is pushed and popped around every step and _error restored afterwards, so nothing but J leaves. */
DRFE_HD void po_plane_perturbed(LmCtx& ctx, const PoEdge& E, const double q[4], const double t[3], int d, int side, double e[3])
{
    double u[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, pq[4], pt[3];
    u[d] = side ? -1e-9 : 1e-9;
    for (int k = 0; k < 4; k++) pq[k] = q[k];
    for (int k = 0; k < 3; k++) pt[k] = t[k];
    (void)po_oplus(ctx, pq, pt, u);
    po_plane_error(ctx, E, pq, pt, e);
}
DRFE_HD void po_plane_jacobian(LmCtx& ctx, const PoEdge& E, const double q[4], const double t[3], double J[3][6])
{
    const double scalar = lm_numeric_scalar();
    for (int d = 0; d < 6; d++) {
        double e1[3], e2[3];
        po_plane_perturbed(ctx, E, q, t, d, 0, e1);
        po_plane_perturbed(ctx, E, q, t, d, 1, e2);
        for (int r = 0; r < 3; r++) J[r][d] = scalar * (e1[r] - e2[r]);
    }
}

/* ---- the vertex under lm_core.h's step control: one lane ---- */

struct PoLM {
    double q[4], t[3];             /* the estimate: quaternion x y z w, translation */
    double qs[4], ts[3];           /* what push() saved */
    LmControl<6> lm;               /* x is kept over rounds */
};

/* push, solve, update */
DRFE_HD void lm_step(PoLM& S)
{
    for (int k = 0; k < 4; k++) S.qs[k] = S.q[k];
    for (int k = 0; k < 3; k++) S.ts[k] = S.t[k];
    lm_solve(S.lm);
    lm_count_theta(S.lm, po_oplus(S.lm.ctx, S.q, S.t, S.lm.x));
}

/* the rho test, pop after a rejected trial */
DRFE_HD int lm_judge(PoLM& S, double tempChi)
{
    int accepted;
    const int more = lm_judge(S.lm, tempChi, accepted);
    if (!accepted) {
        for (int k = 0; k < 4; k++) S.q[k] = S.qs[k];
        for (int k = 0; k < 3; k++) S.t[k] = S.ts[k];
    }
    return more;
}

/* the classification of one edge after a round (src/Optimizer.cc:1067-1326): 1 for an outlier.  `const float chi2 = e->chi2()`
 * against the float threshold of a point or the double one of a plane; a line end's `const float chi2_s = e1->chiline()` =
 * e0 * e0 against the float 2 * chi2Mono.  A NaN is no outlier. */
DRFE_HD int po_outlier(const PoEdge& E, const double e[3])
{
    const float chi2 = (float)(E.kind == PO_LINE ? e[0] * e[0] : po_chi2(E, e));
    return (double)chi2 > E.th;
}

/* Converter::toCvMat(SE3Quat): to_homogeneous_matrix narrowed to float */
DRFE_HD void po_pose_out(const double q[4], const double t[3], float T[16])
{
    double R[3][3];
    mp_quat_to_matrix(q, R);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)R[r][c];
        T[r * 4 + 3] = (float)t[r];
    }
    T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

#endif
