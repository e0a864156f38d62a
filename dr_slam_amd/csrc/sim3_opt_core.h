/* sim3_opt_core.h — the arithmetic of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:3982-4177) and of what g2o runs under
 * it, restated statement by statement: g2o::Sim3 (types/sim3.h: the exponential with its four branches, map, inverse, operator*),
 * the two projection edges of types_seven_dof_expmap.h, BaseBinaryEdge's numeric Jacobian and quadratic form for the one free
 * vertex, Huber's kernel, the 7x7 normal equations and VertexSim3Expmap::oplusImpl; the LDLT and the step control are lm_core.h's.
 * Shared by the host entry (sim3_opt.cpp) and the device kernel (sim3_opt_kernels.hip) so that both produce the same bits: plain
 * IEEE add / mul / div / sqrt in double, compiled with -ffp-contract=off on both sides; sin and cos through cr_sincos.h.  exp has
 * no certified form here: a problem with a free scale runs on the host with the host's libm, also inside the device entry.
 * DESIGN.md section 22 states the evaluation order of every expression; where Eigen leaves an association open it is read left
 * to right, as in section 20, whose kernel and quaternion pieces (pose_opt_core.h) this header reuses.
 *
 * Parity with a g2o / Eigen 3.3.7 build is not pinned: Eigen is not available to the tests.
 *
 * The 14 perturbed estimates of an iteration's numeric Jacobians (so_perturbed) are the same for every edge, so they are formed
 * once per iteration; an edge (so_edge_error, so_edge_terms) is evaluated by one lane.  What is summed over edges (H, b, the
 * robust chi2) is summed by the caller, edge after edge in active-edge order.  The step control (SoLM) runs in one lane. */
#ifndef DRFE_SIM3_OPT_CORE_H
#define DRFE_SIM3_OPT_CORE_H

#include "pose_opt_core.h"
#include "sim3_core.h"

enum { SO_H_TERMS = 28, SO_TERMS = 35 };         /* the lower triangle of H, row by row, then what is added to b */

/* g2o::Sim3: r (x y z w, Eigen's coeffs() order), t, s */
struct SoSim3 { double q[4], t[3], s; };

/* a problem's two cameras (floats widened, as `vSim3->_focal_length1[0] = K1.at<float>(0,0)`), Huber's delta (`const float
 * deltaHuber = sqrt(th2)`, the float sqrt, widened by setDelta(double)) and th2 widened for the comparisons */
struct SoCam { double K1[4], K2[4], delta, th2; };

/* one kept match as staged: the two fixed vertices, the two measurements, the two informations (a float widened, times I) */
struct SoMatch {
    double P1c[3], P2c[3];
    double obs1[2], obs2[2];
    double info1, info2;
};

/* cv::Mat P3Dc = Rcw * P3Dw + tcw: one gemm with a C term on floats (the small-matrix path), then Converter::toVector3d */
DRFE_HD void so_camera_point(const float R[9], const float t[3], const float Xw[3], double Pc[3])
{
    for (int r = 0; r < 3; r++) Pc[r] = (double)s3_gemm_row(R[r * 3], R[r * 3 + 1], R[r * 3 + 2], Xw, 1.0, t[r], 1.0);
}

/* Eigen 3.3.7 Quaternion::_transformVector: uv = 2 (q.vec x v); (v + w uv) + q.vec x uv */
DRFE_HD void so_rotate(const double q[4], const double v[3], double o[3])
{
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int k = 0; k < 3; k++) o[k] = (v[k] + q[3] * uv[k]) + c[k];
}

/* Sim3::map: s * (r * xyz) + t */
DRFE_HD void so_map(const SoSim3& S, const double v[3], double o[3])
{
    double r[3];
    so_rotate(S.q, v, r);
    for (int k = 0; k < 3; k++) o[k] = S.s * r[k] + S.t[k];
}

/* Sim3::inverse: Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s) */
DRFE_HD void so_inverse(const SoSim3& S, SoSim3& I)
{
    const double m = -1.0 / S.s;
    const double v[3] = {m * S.t[0], m * S.t[1], m * S.t[2]};
    I.q[0] = -S.q[0]; I.q[1] = -S.q[1]; I.q[2] = -S.q[2]; I.q[3] = S.q[3];
    so_rotate(I.q, v, I.t);
    I.s = 1.0 / S.s;
}

/* Sim3::operator*: r = a.r * b.r (Eigen's generic quat_product, nothing normalised), t = a.s * (a.r * b.t) + a.t, s = a.s * b.s */
DRFE_HD void so_mul(const SoSim3& A, const SoSim3& B, SoSim3& R)
{
    const double ax = A.q[0], ay = A.q[1], az = A.q[2], aw = A.q[3];
    const double bx = B.q[0], by = B.q[1], bz = B.q[2], bw = B.q[3];
    SoSim3 o;
    o.q[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
    o.q[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
    o.q[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
    o.q[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
    so_map(A, B.t, o.t);
    o.s = A.s * B.s;
    R = o;
}

/* std::exp(sigma): exp(0) is 1; anything else is the host's libm (no certified exp exists here yet, so a last-place difference
 * from a correctly rounded exp is possible), or ctx.fail on the device */
DRFE_HD double so_exp(LmCtx& ctx, double sigma)
{
    if (sigma == 0.0) return 1.0;
#if !defined(__HIP_DEVICE_COMPILE__)
    if (ctx.libm) return exp(sigma);
#endif
    ctx.fail = 1;
    return 1.0;
}

/* Sim3(const Vector7d& update) (types/sim3.h:70-142): omega, upsilon, sigma.  Returns theta < eps.  R is ((I + a Omega) + b
 * Omega2) element by element, W = ((A Omega) + (B Omega2)) + C I; Quaterniond(R) is not normalised. */
DRFE_HD int so_exp_map(LmCtx& ctx, const double u[7], SoSim3& S)
{
    const double o0 = u[0], o1 = u[1], o2 = u[2];
    const double sigma = u[6];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double Om[3][3] = {{0.0, -o2, o1}, {o2, 0.0, -o0}, {-o1, o0, 0.0}};
    double Om2[3][3], R[3][3];
    const double s = so_exp(ctx, sigma);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Om2[r][c] = (Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c];
    const double eps = 0.00001;
    const int small = theta < eps;
    double A, B, C;
    double sn = 0.0, cs = 1.0;
    if (!small) po_sincos(ctx, theta, &sn, &cs);
    if (small) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R[r][c] = ((r == c ? 1.0 : 0.0) + Om[r][c]) + Om2[r][c];
    } else {
        const double a = sn / theta;
        const double b = (1.0 - cs) / (theta * theta);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R[r][c] = ((r == c ? 1.0 : 0.0) + a * Om[r][c]) + b * Om2[r][c];
    }
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (small) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1.0 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn;
            const double b = s * cs;
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2;
        }
    }
    mp_quat_from_matrix(R, S.q);
    for (int r = 0; r < 3; r++) {
        double W[3];
        for (int c = 0; c < 3; c++) W[c] = (A * Om[r][c] + B * Om2[r][c]) + C * (r == c ? 1.0 : 0.0);
        S.t[r] = (W[0] * u[3] + W[1] * u[4]) + W[2] * u[5];
    }
    S.s = s;
    return small;
}

/* VertexSim3Expmap::oplusImpl: `update[6] = 0` through the caller's array when the scale is fixed, then estimate = Sim3(update)
 * * estimate.  Returns theta < eps. */
DRFE_HD int so_oplus(LmCtx& ctx, SoSim3& S, double u[7], int fixScale)
{
    if (fixScale) u[6] = 0.0;
    SoSim3 E;
    const int small = so_exp_map(ctx, u, E);
    so_mul(E, S, S);
    return small;
}

/* the perturbed estimates of BaseBinaryEdge::linearizeOplus for vertex 1 (core/base_binary_edge.hpp:176-198): perturbation
 * j = 2 d + side is oplus(+-1e-9 e_d) of the estimate (side 0 the plus step), P[j] what EdgeSim3ProjectXYZ maps with and Pinv[j]
 * its inverse(), which EdgeInverseSim3ProjectXYZ maps with.  The estimate is pushed and popped around every step. */
DRFE_HD void so_perturbed(LmCtx& ctx, const SoSim3& S, int fixScale, int j, SoSim3& P, SoSim3& Pinv)
{
    double u[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    u[j >> 1] = (j & 1) ? -1e-9 : 1e-9;
    P = S;
    (void)so_oplus(ctx, P, u, fixScale);
    so_inverse(P, Pinv);
}

/* obs - cam_map(project(p)): project is (p0 / p2, p1 / p2), cam_map v * focal + principal */
DRFE_HD void so_project_error(const double obs[2], const double K[4], const double p[3], double e[2])
{
    e[0] = obs[0] - ((p[0] / p[2]) * K[0] + K[2]);
    e[1] = obs[1] - ((p[1] / p[2]) * K[1] + K[3]);
}

/* computeError of edge `kind` (0: EdgeSim3ProjectXYZ e12, 1: EdgeInverseSim3ProjectXYZ e21) of a match under the estimate S, whose
 * inverse() is Sinv */
DRFE_HD void so_edge_error(const SoMatch& M, const SoCam& C, int kind, const SoSim3& S, const SoSim3& Sinv, double e[2])
{
    double p[3];
    if (kind == 0) {
        so_map(S, M.P2c, p);
        so_project_error(M.obs1, C.K1, p, e);
    } else {
        so_map(Sinv, M.P1c, p);
        so_project_error(M.obs2, C.K2, p, e);
    }
}

/* BaseEdge::chi2: _error.dot(information() * _error), the information the 2x2 diag(info, info) with its zeros multiplied through */
DRFE_HD double so_chi2(double info, const double e[2])
{
    const double w0 = info * e[0] + 0.0 * e[1];
    const double w1 = 0.0 * e[0] + info * e[1];
    return e[0] * w0 + e[1] * w1;
}

/* an edge's term of activeRobustChi2 */
DRFE_HD double so_chi_term(double info, double delta, const double e[2])
{
    double r0, r1;
    po_huber(so_chi2(info, e), delta, &r0, &r1);
    return r0;
}

/* BaseBinaryEdge::constructQuadraticForm of one edge with its kernel, vertex 1's part (vertex 0 is fixed): term[r (r + 1) / 2 + c]
 * is what the edge adds to H(r, c), c <= r, term[28 + r] what it adds to b(r).
 *   omega_r = -(Omega e); omega_r *= rho1; b += B^T omega_r; H += (B^T (rho1 Omega)) B
 * each product a temporary, each element a sum over the inner index from 0 up.  J is 2 x 7: column d = scalar * (e(+) - e(-)). */
DRFE_HD void so_edge_terms(double info, double delta, const double J[2][7], const double e[2], double term[SO_TERMS])
{
    double r0, rho1;
    po_huber(so_chi2(info, e), delta, &r0, &rho1);
    const double Om[2][2] = {{info, 0.0}, {0.0, info}};
    double omr[2], W[2][2];
    for (int k = 0; k < 2; k++) {
        omr[k] = -(Om[k][0] * e[0] + Om[k][1] * e[1]);
        omr[k] = omr[k] * rho1;
        for (int m = 0; m < 2; m++) W[k][m] = rho1 * Om[k][m];
    }
    for (int i = 0; i < 7; i++) {
        double T[2];
        for (int k = 0; k < 2; k++) T[k] = J[0][i] * W[0][k] + J[1][i] * W[1][k];
        for (int j = 0; j <= i; j++) term[i * (i + 1) / 2 + j] = T[0] * J[0][j] + T[1] * J[1][j];
        term[SO_H_TERMS + i] = J[0][i] * omr[0] + J[1][i] * omr[1];
    }
}

/* ---- the vertex under lm_core.h's step control: one lane ---- */

struct SoLM {
    SoSim3 S, saved;               /* the estimate and what push() saved */
    int32_t fixScale;
    LmControl<7> lm;               /* x is kept over the two phases */
};

DRFE_HD void so_lm_init(SoLM& L, const double S12[8], int fixScale, int libm)
{
    for (int k = 0; k < 4; k++) L.S.q[k] = S12[k];
    for (int k = 0; k < 3; k++) L.S.t[k] = S12[4 + k];
    L.S.s = S12[7];
    L.saved = L.S;
    L.fixScale = fixScale;
    lm_init(L.lm, libm);
}

/* update(): oplusImpl zeroes x[6] in the solver's own array when the scale is fixed */
DRFE_HD void so_lm_update(SoLM& L) { lm_count_theta(L.lm, so_oplus(L.lm.ctx, L.S, L.lm.x, L.fixScale)); }

/* push, solve, update: the update before lm_judge's computeScale reads x */
DRFE_HD void lm_step(SoLM& L)
{
    L.saved = L.S;
    lm_solve(L.lm);
    so_lm_update(L);
}

/* the rho test, pop after a rejected trial */
DRFE_HD int lm_judge(SoLM& L, double tempChi)
{
    int accepted;
    const int more = lm_judge(L.lm, tempChi, accepted);
    if (!accepted) L.S = L.saved;
    return more;
}

/* `e12->chi2() > th2 || e21->chi2() > th2`: doubles against the widened float; a NaN is no outlier.  e = e12's error, then e21's */
DRFE_HD int so_outlier(const SoMatch& M, double th2, const double e[4])
{
    return so_chi2(M.info1, e) > th2 || so_chi2(M.info2, e + 2) > th2;
}

/* Converter::toCvMat(g2o::Sim3): toCvSE3(s * r.toRotationMatrix(), t) */
DRFE_HD void so_to_cvmat(const SoSim3& S, float T[16])
{
    double R[3][3];
    mp_quat_to_matrix(S.q, R);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)(S.s * R[r][c]);
        T[r * 4 + 3] = (float)S.t[r];
    }
    T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

/* g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0): the floats widened, Quaterniond(R) as it is */
DRFE_HD void so_from_pose(const float R[9], const float t[3], SoSim3& S)
{
    double m[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[r][c] = (double)R[r * 3 + c];
    mp_quat_from_matrix(m, S.q);
    for (int k = 0; k < 3; k++) S.t[k] = (double)t[k];
    S.s = 1.0;
}

#endif
