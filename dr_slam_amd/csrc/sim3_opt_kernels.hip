/* sim3_opt_kernels.hip — Optimizer::OptimizeSim3 (reference src/Optimizer.cc:3982-4177) on gfx950, every fixed-scale problem of
 * a call, driven by sim3_opt.cpp.  DESIGN.md section 22.
 *   k_sim3_opt   one workgroup of 256 lanes per problem runs both optimize() calls and both classifications in one launch.
 *                At the start of an iteration lanes 0..13 form the 14 perturbed estimates of the numeric Jacobians and their
 *                inverses in LDS; they are the same for every edge.  An edge (e12 or e21 of a match) is evaluated by one lane, 256
 *                edges (128 matches, a chunk) at a time: its error, its term of the robust chi2 and, when the system is built, its
 *                14 perturbed errors, its Jacobian and its 35 terms of H and b, written to LDS.  Lanes 0..34 each own one entry of
 *                H / b and add the chunk's terms edge after edge; lane 35 owns the robust chi2 the same way.  An edge that is not
 *                active (its match nulled by the first classification, or past the end) contributes +0.0, which changes no bit of
 *                a sum that started at +0.0.  Lane 0 runs the step control, the 7x7 LDLT and the update (SoLM) and keeps it in
 *                LDS, where every lane reads the estimate; every decision the workgroup branches on goes through LDS behind a
 *                barrier.  Every loop is bounded by the reference's limits (5 or 10 iterations, 10 trials, the chunk count).
 *                A problem with a free scale returns at once: the host core runs it (exp has no certified form here).
 * No float or double atomics; a sum is never split across lanes.  -ffp-contract=off, as the host entry. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sim3_opt_internal.h"
#include "lm_device.h"

namespace {

struct SoShared {
    double term[SO_ROWS * SO_TERM_STRIDE];   /* rows 0..34 the terms of H and b, row 35 the chi2 terms */
    SoSim3 pert[14], pinv[14];
    SoSim3 Sinv;
    SoLM L;
    double chi;
    int32_t ctl;                   /* the decision of the step control every lane branches on */
    int32_t count, count2;         /* nActive, then the outliers of a classification; what the stale errors decided differently */
    int32_t fail;                  /* a lane could not certify a transcendental */
};

/* computeActiveErrors and activeRobustChi2; with `build` also linearizeOplus and constructQuadraticForm into L.lm.H / L.lm.b.
 * Returns the robust chi2 in every lane.  Every lane of the workgroup calls it.  Kept out of line, as the compiler had it while the
 * trial loop called it from two places: inlined, the kernel takes 107 AGPRs instead of the 32 of DESIGN.md section 22. */
__device__ __noinline__ double so_pass(SoShared& sh, const SoProbRec& P, const SoMatch* match, double* err, const uint8_t* flag, bool build)
{
    const int tid = threadIdx.x;
    LmCtx ctx = {0, 0};
    if (tid == 0) so_inverse(sh.L.S, sh.Sinv);
    if (build && tid < 14) so_perturbed(ctx, sh.L.S, P.fixScale, tid, sh.pert[tid], sh.pinv[tid]);
    __syncthreads();
    const SoSim3 S = sh.L.S, Sinv = sh.Sinv;
    const int nEdges = 2 * lm_uniform(P.nMatches);
    double acc = 0.0;
    for (int base = 0; base < nEdges; base += SO_THREADS) {
        const int k = base + tid;
        const int m = k >> 1, kind = k & 1;
        const bool act = k < nEdges && !flag[m];
        double c = 0.0;
        if (act) {
            const SoMatch M = match[m];
            const double info = kind ? M.info2 : M.info1;
            double e[2];
            so_edge_error(M, P.cam, kind, S, Sinv, e);
            err[2 * (size_t)k] = e[0];
            err[2 * (size_t)k + 1] = e[1];
            c = so_chi_term(info, P.cam.delta, e);
            if (build) {
                double J[2][7], term[SO_TERMS];
                const double scalar = lm_numeric_scalar();
                for (int d = 0; d < 7; d++) {
                    double e1[2], e2[2];
                    so_edge_error(M, P.cam, kind, sh.pert[2 * d], sh.pinv[2 * d], e1);
                    so_edge_error(M, P.cam, kind, sh.pert[2 * d + 1], sh.pinv[2 * d + 1], e2);
                    for (int r = 0; r < 2; r++) J[r][d] = scalar * (e1[r] - e2[r]);
                }
                so_edge_terms(info, P.cam.delta, J, e, term);
                for (int r = 0; r < SO_TERMS; r++) sh.term[r * SO_TERM_STRIDE + tid] = term[r];
            }
        } else if (build) {
            for (int r = 0; r < SO_TERMS; r++) sh.term[r * SO_TERM_STRIDE + tid] = 0.0;
        }
        sh.term[SO_TERMS * SO_TERM_STRIDE + tid] = c;
        __syncthreads();
        const int cnt = nEdges - base < SO_THREADS ? nEdges - base : SO_THREADS;
        if (tid == SO_TERMS || (build && tid < SO_TERMS)) {
            const double* row = sh.term + tid * SO_TERM_STRIDE;
            for (int j = 0; j < cnt; j++) acc += row[j];
        }
        __syncthreads();
    }
    if (ctx.fail) sh.fail = 1;
    if (build) {
        if (tid < SO_H_TERMS) sh.L.lm.H[tid] = acc;
        else if (tid < SO_TERMS) sh.L.lm.b[tid - SO_H_TERMS] = acc;
    }
    if (tid == SO_TERMS) sh.chi = acc;
    __syncthreads();
    return sh.chi;
}

}  // namespace

__global__ __launch_bounds__(SO_THREADS) void k_sim3_opt(const SoLaunch L)
{
    __shared__ SoShared sh;
    const int tid = threadIdx.x;
    const SoProbRec& P = L.prob[blockIdx.x];
    if (!lm_uniform(P.fixScale)) return;                            /* uniform: the host core runs the problem */
    SoProbOut& O = L.out[blockIdx.x];
    const SoMatch* match = L.match + P.match0;
    double* err = L.err + 4 * (size_t)P.match0;
    uint8_t* flag = L.flag + P.match0;
    const int nM = lm_uniform(P.nMatches);
    int nBad = 0, early = 0, ret = 0, lastRejectedPhases = 0, stale = 0;
    int iterations[2] = {0, 0}, trials[2] = {0, 0};
    if (tid == 0) {
        so_lm_init(sh.L, P.S12, 1, 0);
        sh.fail = 0;
    }
    for (int phase = 0; phase < 2; phase++) {
        const int iters = phase == 0 ? 5 : (nBad > 0 ? 10 : 5);
        if (tid == 0) {
            sh.L.lm.lastRejected = 0;
            sh.count = 0;
            sh.count2 = 0;
        }
        __syncthreads();
        const int it0 = lm_uniform(sh.L.lm.iterations), tr0 = lm_uniform(sh.L.lm.trials);
        {
            int mine = 0;
            for (int m = tid; m < nM; m += SO_THREADS) mine += flag[m] ? 0 : 1;
            if (mine) atomicAdd(&sh.count, mine);
        }
        __syncthreads();
        const int nActive = lm_uniform(sh.count);
        __syncthreads();
        if (nActive > 0) lm_iterations(sh.L, sh.ctl, iters, [&](bool build) { return so_pass(sh, P, match, err, flag, build); });
        /* the classification on _error as the last trial left it; after a rejected one also on the errors at the kept estimate,
         * to count what the stale ones decided differently */
        if (tid == 0) {
            so_inverse(sh.L.S, sh.Sinv);
            sh.count = 0;
        }
        __syncthreads();
        const int rejected = lm_uniform(sh.L.lm.lastRejected);
        iterations[phase] = lm_uniform(sh.L.lm.iterations) - it0;
        trials[phase] = lm_uniform(sh.L.lm.trials) - tr0;
        lastRejectedPhases += rejected ? 1 : 0;
        {
            int mine = 0, mine2 = 0;
            for (int m = tid; m < nM; m += SO_THREADS) {
                if (flag[m]) continue;
                const SoMatch M = match[m];
                double e[4];
                for (int r = 0; r < 4; r++) e[r] = err[4 * (size_t)m + r];
                const int out = so_outlier(M, P.cam.th2, e);
                if (rejected) {
                    so_edge_error(M, P.cam, 0, sh.L.S, sh.Sinv, e);
                    so_edge_error(M, P.cam, 1, sh.L.S, sh.Sinv, e + 2);
                    if (so_outlier(M, P.cam.th2, e) != out) mine2++;
                }
                flag[m] = (uint8_t)out;
                mine += out;
            }
            if (mine) atomicAdd(&sh.count, mine);
            if (mine2) atomicAdd(&sh.count2, mine2);
        }
        __syncthreads();
        const int count = lm_uniform(sh.count);
        stale += lm_uniform(sh.count2);
        __syncthreads();
        if (phase == 0) {
            nBad = count;
            if (nM - nBad < 10) { early = 1; break; }
        } else {
            ret = nActive - count;
        }
    }
    if (tid == 0) {
        SoProbOut R;
        R.ret = ret;
        R.nBad = nBad;
        for (int k = 0; k < 2; k++) { R.iterations[k] = iterations[k]; R.trials[k] = trials[k]; }
        for (int k = 0; k < SO_DIAG_N; k++) R.diag[k] = 0;
        R.diag[SO_DIAG_REJECTED] = sh.L.lm.rejected;
        R.diag[SO_DIAG_LAST_REJECTED] = lastRejectedPhases;
        R.diag[SO_DIAG_NBAD_STOPS] = sh.L.lm.nBadStops;
        R.diag[SO_DIAG_SMALL_THETA] = sh.L.lm.smallTheta;
        R.diag[SO_DIAG_BIG_THETA] = sh.L.lm.bigTheta;
        R.diag[SO_DIAG_EARLY_RETURN] = early;
        R.diag[SO_DIAG_STALE_DECIDED] = stale;
        R.handBack = (sh.L.lm.ctx.fail || sh.fail) ? 1 : 0;
        R.pad = 0;
        SoSim3 S = sh.L.S;
        if (early) {
            for (int k = 0; k < 4; k++) S.q[k] = P.S12[k];
            for (int k = 0; k < 3; k++) S.t[k] = P.S12[4 + k];
            S.s = P.S12[7];
        }
        so_finish(P, S, R);
        O = R;
    }
}

hipError_t drfe_launch_sim3_opt(const SoLaunch& L, hipStream_t s)
{
    if (L.nProblems <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sim3_opt, dim3(L.nProblems), dim3(SO_THREADS), 0, s, L);
    return hipGetLastError();
}
