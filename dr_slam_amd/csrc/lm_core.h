/* lm_core.h — what the g2o-style optimisers (pose_opt_core.h, trans_opt_core.h, sim3_opt_core.h) share below their vertices:
 * the context a lane carries through the transcendentals, the certified cube, Eigen's LDLT of an N x N system and
 * OptimizationAlgorithmLevenberg::solve's step control, restated statement by statement once for every dimension.  Shared by the
 * host entries and the device kernels so that both produce the same bits: plain IEEE arithmetic in double, -ffp-contract=off on
 * both sides.  A vertex (PoLM, SoLM) holds its estimate, what push() saved and an LmControl<N>; its lm_step and lm_judge add the
 * three vertex lines (push, oplus, pop) to lm_solve and lm_judge here.  The step control runs in one lane.  DESIGN.md section 24. */
#ifndef DRFE_LM_CORE_H
#define DRFE_LM_CORE_H

#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/drfe_math.h"
#include "cr_cube.h"

/* what a lane carries through the transcendentals: fail = one could not be certified and no libm stood in (device: the frame goes
 * back to the host); libm = the host's libm stands in */
struct LmCtx { int32_t fail, libm; };

/* the cube: correctly rounded, or the host's libm where the certificate fails, or ctx.fail */
DRFE_HD double lm_cube(LmCtx& ctx, double v)
{
    double r;
    if (!(fabs(v) <= DBL_MAX)) return v * v * v;          /* NaN and the infinities, as pow(v, 3) */
    if (drfe_cr_cube(v, &r)) return r;
#if !defined(__HIP_DEVICE_COMPILE__)
    if (ctx.libm) return pow(v, 3);
#endif
    ctx.fail = 1;
    return r;
}

/* the factor of BaseUnaryEdge / BaseBinaryEdge::linearizeOplus's numeric Jacobians: 1 / (2 delta), delta = 1e-9 */
DRFE_HD double lm_numeric_scalar() { return 1.0 / (2 * 1e-9); }

/* Eigen::LDLT<MatrixXd>::compute of the N x N whose lower triangle is A (full storage, row-major; the upper triangle is not
 * read), in place (ldlt_inplace<Lower>::unblocked, Eigen 3.3.7), then solve(b) into x when isPositive().  Returns isPositive().
 * Dot products and the rank update's products are summed over the inner index from 0 up. */
template <int N>
DRFE_HD int lm_ldlt_solve(double A[N][N], const double b[N], double x[N])
{
    const int n = N;
    int tr[N];
    double temp[N];
    int sign = 0;                                  /* 0 ZeroSign, 1 PositiveSemiDef, -1 NegativeSemiDef, 2 Indefinite */
    bool early = false;                            /* (found_zero_pivot only decides info(), which g2o does not read) */
    for (int k = 0; k < n && !early; k++) {
        int big = k;
        double best = fabs(A[k][k]);
        for (int i = k + 1; i < n; i++) {
            const double v = fabs(A[i][i]);
            if (v > best) { best = v; big = i; }
        }
        tr[k] = big;
        if (k != big) {
            for (int j = 0; j < k; j++) { const double s = A[k][j]; A[k][j] = A[big][j]; A[big][j] = s; }
            for (int i = big + 1; i < n; i++) { const double s = A[i][k]; A[i][k] = A[i][big]; A[i][big] = s; }
            { const double s = A[k][k]; A[k][k] = A[big][big]; A[big][big] = s; }
            for (int i = k + 1; i < big; i++) { const double s = A[i][k]; A[i][k] = A[big][i]; A[big][i] = s; }
        }
        const int rs = n - k - 1;
        if (k > 0) {
            for (int j = 0; j < k; j++) temp[j] = A[j][j] * A[k][j];
            double s = 0.0;
            for (int j = 0; j < k; j++) { const double a = A[k][j] * temp[j]; s = j == 0 ? a : s + a; }
            A[k][k] -= s;
            for (int i = k + 1; i < n; i++) {
                double u = 0.0;
                for (int j = 0; j < k; j++) { const double a = A[i][j] * temp[j]; u = j == 0 ? a : u + a; }
                A[i][k] -= u;
            }
        }
        const double realAkk = A[k][k];
        const bool pivot_is_valid = fabs(realAkk) > 0.0;
        if (k == 0 && !pivot_is_valid) {
            sign = 0;
            for (int j = 0; j < n; j++) tr[j] = j;
            early = true;
            break;
        }
        if (rs > 0 && pivot_is_valid)
            for (int i = k + 1; i < n; i++) A[i][k] /= realAkk;
        if (sign == 1) {
            if (realAkk < 0.0) sign = 2;
        } else if (sign == -1) {
            if (realAkk > 0.0) sign = 2;
        } else if (sign == 0) {
            if (realAkk > 0.0) sign = 1;
            else if (realAkk < 0.0) sign = -1;
        }
    }
    if (!(sign == 1 || sign == 0)) return 0;
    /* LDLT::_solve_impl: P b; L^-1 (column by column); D^-1 with the tolerance 1 / highest(); L^-T (row by row); P^T */
    double d[N];
    for (int i = 0; i < n; i++) d[i] = b[i];
    for (int k = 0; k < n; k++) { const double s = d[k]; d[k] = d[tr[k]]; d[tr[k]] = s; }
    for (int i = 0; i < n; i++)
        if (d[i] != 0.0)                           /* triangular_solve_vector skips a zero right-hand side element */
            for (int j = i + 1; j < n; j++) d[j] -= d[i] * A[j][i];
    const double tolerance = 1.0 / DBL_MAX;
    for (int i = 0; i < n; i++) {
        if (fabs(A[i][i]) > tolerance) d[i] /= A[i][i];
        else d[i] = 0.0;
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = 0.0;
        for (int j = i + 1; j < n; j++) { const double a = A[j][i] * d[j]; s = j == i + 1 ? a : s + a; }
        if (i + 1 < n) d[i] -= s;
    }
    for (int k = n - 1; k >= 0; k--) { const double s = d[k]; d[k] = d[tr[k]]; d[tr[k]] = s; }
    for (int i = 0; i < n; i++) x[i] = d[i];
    return 1;
}

/* the solver's side of an optimize() call for a vertex of N dimensions */
template <int N>
struct LmControl {
    double H[N * (N + 1) / 2], b[N];   /* the system of the current iteration: H's lower triangle, row by row */
    double x[N];                       /* the solver's x: kept over a failed solve and over optimize() calls, zero at the start */
    double lambda, ni, currentChi, iniChi, rho;
    int32_t nBad, qmax;
    int32_t solved;                    /* the last trial's LDLT was isPositive() and wrote x (Levenberg's ok2) */
    LmCtx ctx;
    int32_t iterations, trials, rejected, lastRejected, nBadStops, smallTheta, bigTheta;   /* diagnostics of the call */
};

template <int N>
DRFE_HD void lm_init(LmControl<N>& C, int libm)
{
    for (int k = 0; k < N; k++) C.x[k] = 0.0;
    C.ctx.fail = 0; C.ctx.libm = libm;
    C.iterations = 0; C.trials = 0; C.rejected = 0; C.lastRejected = 0; C.nBadStops = 0; C.smallTheta = 0; C.bigTheta = 0;
    C.lambda = -1.0; C.ni = 2.0; C.nBad = 0; C.qmax = 0; C.solved = 0; C.rho = 0.0; C.currentChi = 0.0; C.iniChi = 0.0;
}

/* OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:61-164) cut at its calls into the graph:
 *   lm_begin(C, iteration, chi)      after computeActiveErrors / activeRobustChi2 / buildSystem (C.H, C.b filled)
 *   the vertex's lm_step(V)          push, lm_solve (setLambda, solve, restoreDiagonal), update: oplus on C.x, counted by lm_count_theta;
 *                                    then the caller recomputes the errors
 *   the vertex's lm_judge(V, chi)    lm_judge(C, chi, accepted), pop when the trial is not accepted; returns 1 when the do-while goes on
 *   lm_end(C)                        returns 1 for OK, 0 for Terminate */
template <int N>
DRFE_HD void lm_begin(LmControl<N>& C, int iteration, double chi)
{
    C.currentChi = chi;
    C.iniChi = chi;
    if (iteration == 0) {
        /* computeLambdaInit: std::max(fabs(h), maxDiagonal) is (fabs(h) < maxDiagonal) ? maxDiagonal : fabs(h) */
        double maxDiagonal = 0.0;
        for (int j = 0; j < N; j++) {
            const double a = fabs(C.H[j * (j + 1) / 2 + j]);
            maxDiagonal = a < maxDiagonal ? maxDiagonal : a;
        }
        C.lambda = 1e-5 * maxDiagonal;
        C.ni = 2.0;
        C.nBad = 0;
    }
    C.rho = 0.0;
    C.qmax = 0;
    C.iterations++;
}

/* A = H + lambda I, then the LDLT into C.x */
template <int N>
DRFE_HD void lm_solve(LmControl<N>& C)
{
    double A[N][N];
    for (int i = 0; i < N; i++)
        for (int j = 0; j <= i; j++) {
            const double h = C.H[i * (i + 1) / 2 + j];
            A[i][j] = i == j ? h + C.lambda : h;
            A[j][i] = A[i][j];
        }
    C.solved = lm_ldlt_solve<N>(A, C.b, C.x);
    C.trials++;
}

/* what oplusImpl returned for the trial's update: theta below its threshold or not */
template <int N>
DRFE_HD void lm_count_theta(LmControl<N>& C, int small)
{
    if (small) C.smallTheta++;
    else C.bigTheta++;
}

/* computeScale: reads the solver's x after update() has run (Sim3's oplusImpl zeroes x[6] there when the scale is fixed) */
template <int N>
DRFE_HD double lm_scale(const LmControl<N>& C)
{
    double scale = 0.0;
    for (int j = 0; j < N; j++) scale += C.x[j] * (C.lambda * C.x[j] + C.b[j]);
    scale += 1e-3;
    return scale;
}

/* the rho test.  accepted = the trial stays; otherwise the caller restores the vertex (pop).  Returns 1 when the do-while goes on */
template <int N>
DRFE_HD int lm_judge(LmControl<N>& C, double tempChi, int& accepted)
{
    if (!C.solved) tempChi = DBL_MAX;
    double rho = C.currentChi - tempChi;
    rho /= lm_scale(C);
    accepted = rho > 0.0 && isfinite(tempChi);
    if (accepted) {
        double alpha = 1.0 - lm_cube(C.ctx, 2.0 * rho - 1.0);
        const double up = 2.0 / 3.0, lo = 1.0 / 3.0;
        alpha = up < alpha ? up : alpha;                       /* std::min(alpha, up) */
        const double scaleFactor = lo < alpha ? alpha : lo;    /* std::max(lo, alpha) */
        C.lambda *= scaleFactor;
        C.ni = 2.0;
        C.currentChi = tempChi;
        C.lastRejected = 0;
    } else {
        C.lambda *= C.ni;
        C.ni *= 2.0;
        C.rejected++;
        C.lastRejected = 1;
    }
    C.rho = rho;
    C.qmax++;
    return rho < 0.0 && C.qmax < 10;
}

template <int N>
DRFE_HD int lm_end(LmControl<N>& C)
{
    if (C.qmax == 10 || C.rho == 0.0) return 0;
    if ((C.iniChi - C.currentChi) * 1e3 < C.iniChi) C.nBad++;
    else C.nBad = 0;
    if (C.nBad >= 3) { C.nBadStops++; return 0; }
    return 1;
}

#endif
