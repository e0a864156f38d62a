/* pose_opt_kernels.hip — Optimizer::PoseOptimization (reference src/Optimizer.cc:601-1338) on gfx950, every frame of a call,
 * driven by pose_opt.cpp.  DESIGN.md section 20.
 *   k_pose_opt   one workgroup of 256 lanes per frame runs the frame's four rounds, classification included, in one launch.
 *                A point or line edge is evaluated by one lane, 256 edges (a chunk) at a time: its error, its term of the robust
 *                chi2 and, when the system is built, its Jacobian and its 27 terms of H and b, written to LDS.  Plane edges come
 *                16 at a time: the twelve perturbed errors of each edge's numeric Jacobian in twelve lanes (192 of the 256), the
 *                edge's own error in a lane of the fourth wavefront, which then forms the Jacobian and the 27 terms.
 *                Lanes 0..26 each own one entry of H / b and add the chunk's terms edge after edge; lane 0 owns the robust chi2
 *                the same way.  An edge that is not active (an outlier of an earlier round, or past the end) contributes +0.0,
 *                which changes no bit of a sum that started at +0.0.  Lane 0 runs the step control, the 6x6 LDLT and the update
 *                (PoLM) and keeps it in LDS, where every lane reads the estimate; every decision the workgroup branches on goes
 *                through LDS behind a barrier.
 * No float or double atomics; a sum is never split across lanes.  -ffp-contract=off, as the host entry. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "pose_opt_internal.h"
#include "lm_device.h"

namespace {

struct PoShared {
    double term[PO_TERMS * PO_TERM_STRIDE];
    double chi[PO_THREADS];
    double pert[PO_PLANE_GROUP * 12 * 3];
    PoLM S;
    int32_t ctl;                   /* the decision of the step control every lane branches on */
    int32_t count;                 /* nActive, then nBad */
    int32_t fail;                  /* a lane could not certify a transcendental */
};

/* what lanes 0..26 and lane 0 add after a chunk's terms are in LDS */
using PoSums = LmSums<PO_TERMS, PO_H_TERMS, PO_TERM_STRIDE>;

/* computeActiveErrors and activeRobustChi2; with `build` also linearizeOplus and constructQuadraticForm into S.lm.H / S.lm.b.
 * Returns the robust chi2 in lane 0.  Every lane of the workgroup calls it. */
__device__ double po_pass(PoShared& sh, const PoFrameRec& F, const PoEdge* edge, double* err, const uint8_t* flag, int robust,
                          bool build)
{
    const int tid = threadIdx.x;
    LmCtx ctx = {0, 0};
    double q[4], t[3];
    for (int k = 0; k < 4; k++) q[k] = sh.S.q[k];
    for (int k = 0; k < 3; k++) t[k] = sh.S.t[k];
    PoSums sums = {0.0, 0.0};
    const int plane0 = F.nPoints + 2 * F.nLines;
    for (int base = 0; base < plane0; base += PO_THREADS) {
        const int k = base + tid;
        const bool act = k < plane0 && !flag[k];
        double c = 0.0;
        if (act) {
            const PoEdge E = edge[k];
            double e[3];
            po_edge_error(ctx, E, F.cam, q, t, e);
            for (int r = 0; r < 3; r++) err[3 * (size_t)k + r] = e[r];
            c = po_chi_term(E, e, robust);
            if (build) {
                double J[3][6], term[PO_TERMS];
                po_edge_jacobian(E, F.cam, q, t, J);
                po_edge_terms(E, J, e, robust, term);
                for (int r = 0; r < PO_TERMS; r++) sh.term[r * PO_TERM_STRIDE + tid] = term[r];
            }
        } else if (build) {
            for (int r = 0; r < PO_TERMS; r++) sh.term[r * PO_TERM_STRIDE + tid] = 0.0;
        }
        sh.chi[tid] = c;
        __syncthreads();
        sums.add(sh.term, sh.chi, plane0 - base < PO_THREADS ? plane0 - base : PO_THREADS, build);
        __syncthreads();
    }
    for (int base = plane0; base < F.nEdges; base += PO_PLANE_GROUP) {
        const int cnt = F.nEdges - base < PO_PLANE_GROUP ? F.nEdges - base : PO_PLANE_GROUP;
        const int own = tid - 12 * PO_PLANE_GROUP;                 /* lanes 192..207: the edge's own error, then its terms */
        double e[3] = {0.0, 0.0, 0.0};
        bool act = false;
        if (tid < 12 * PO_PLANE_GROUP) {
            const int g = tid / 12, pr = tid % 12;
            if (build && g < cnt && !flag[base + g]) {
                double pe[3];
                po_plane_perturbed(ctx, edge[base + g], q, t, pr >> 1, pr & 1, pe);
                for (int r = 0; r < 3; r++) sh.pert[tid * 3 + r] = pe[r];
            }
        } else if (own < PO_PLANE_GROUP) {
            act = own < cnt && !flag[base + own];
            double c = 0.0;
            if (act) {
                const int k = base + own;
                po_plane_error(ctx, edge[k], q, t, e);
                for (int r = 0; r < 3; r++) err[3 * (size_t)k + r] = e[r];
                c = po_chi_term(edge[k], e, robust);
            }
            sh.chi[own] = c;
        }
        __syncthreads();
        if (build && own >= 0 && own < PO_PLANE_GROUP) {
            double term[PO_TERMS];
            if (act) {
                double J[3][6];
                const double scalar = lm_numeric_scalar();
                for (int d = 0; d < 6; d++)
                    for (int r = 0; r < 3; r++)
                        J[r][d] = scalar * (sh.pert[((own * 12 + 2 * d) * 3) + r] - sh.pert[((own * 12 + 2 * d + 1) * 3) + r]);
                po_edge_terms(edge[base + own], J, e, robust, term);
            } else {
                for (int r = 0; r < PO_TERMS; r++) term[r] = 0.0;
            }
            for (int r = 0; r < PO_TERMS; r++) sh.term[r * PO_TERM_STRIDE + own] = term[r];
        }
        __syncthreads();
        sums.add(sh.term, sh.chi, cnt, build);
        __syncthreads();
    }
    if (ctx.fail) sh.fail = 1;
    if (build) {
        if (tid < PO_H_TERMS) sh.S.lm.H[tid] = sums.acc;
        else if (tid < PO_TERMS) sh.S.lm.b[tid - PO_H_TERMS] = sums.acc;
        __syncthreads();
    }
    return sums.chi;
}

}  // namespace

__global__ __launch_bounds__(PO_THREADS) void k_pose_opt(const PoLaunch L)
{
    __shared__ PoShared sh;
    const int tid = threadIdx.x;
    const PoFrameRec& F = L.frame[blockIdx.x];
    PoFrameOut& O = L.out[blockIdx.x];
    const PoEdge* edge = L.edge + F.edge0;
    double* err = L.err + 3 * (size_t)F.edge0;
    uint8_t* flag = L.flag + F.edge0;
    const int nInitial = lm_uniform(F.nPoints + F.nLines + F.nPlaneEdges), nEdges = lm_uniform(F.nEdges);
    if (nInitial < 3) {                                 /* uniform: the pose untouched, the flags false (zero before the launch) */
        if (tid < 16) O.Tcw[tid] = F.Tcw[tid];
        return;
    }
    int robust = 1, rounds = 0, lastRejectedRounds = 0, emptyRounds = 0, nBad = 0;
    if (tid == 0) {
        lm_init(sh.S.lm, 0);
        sh.fail = 0;
    }
    for (int it = 0; it < 4; it++) {
        if (tid == 0) {
            mp_to_se3quat(F.Tcw, sh.S.q, sh.S.t);
            sh.S.lm.lastRejected = 0;
            sh.count = 0;
        }
        __syncthreads();
        {
            int mine = 0;
            for (int k = tid; k < F.nEdges; k += PO_THREADS) mine += flag[k] ? 0 : 1;
            if (mine) atomicAdd(&sh.count, mine);
        }
        __syncthreads();
        const int nActive = lm_uniform(sh.count);
        __syncthreads();
        if (nActive == 0) emptyRounds++;
        else lm_iterations(sh.S, sh.ctl, 10, [&](bool build) { return po_pass(sh, F, edge, err, flag, robust, build); });
        rounds++;
        if (tid == 0) {
            if (sh.S.lm.lastRejected) lastRejectedRounds++;
            sh.count = 0;
        }
        __syncthreads();
        /* the classification: a point or a plane by one lane (a point by the lane that owns its edge in po_pass), a line's two
         * ends by one lane */
        {
            LmCtx ctx = {0, 0};
            double q[4], t[3];
            for (int k = 0; k < 4; k++) q[k] = sh.S.q[k];
            for (int k = 0; k < 3; k++) t[k] = sh.S.t[k];
            const int line0 = F.nPoints, plane0 = F.nPoints + 2 * F.nLines;
            int mine = 0;
            for (int j = tid; j < F.nPoints + F.nPlaneEdges; j += PO_THREADS) {
                const int k = j < F.nPoints ? j : plane0 + (j - F.nPoints);
                const PoEdge E = edge[k];
                double e[3];
                if (flag[k]) {
                    po_edge_error(ctx, E, F.cam, q, t, e);
                    for (int r = 0; r < 3; r++) err[3 * (size_t)k + r] = e[r];
                } else {
                    for (int r = 0; r < 3; r++) e[r] = err[3 * (size_t)k + r];
                }
                const int out = po_outlier(E, e);
                flag[k] = (uint8_t)out;
                mine += out;
            }
            for (int l = tid; l < F.nLines; l += PO_THREADS) {
                const int k = line0 + 2 * l;
                double e1[3], e2[3];
                po_edge_error(ctx, edge[k], F.cam, q, t, e1);
                po_edge_error(ctx, edge[k + 1], F.cam, q, t, e2);
                for (int r = 0; r < 3; r++) { err[3 * (size_t)k + r] = e1[r]; err[3 * (size_t)(k + 1) + r] = e2[r]; }
                const int out = po_outlier(edge[k], e1) || po_outlier(edge[k + 1], e2);
                flag[k] = (uint8_t)out;
                flag[k + 1] = (uint8_t)out;
                mine += out;
            }
            if (mine) atomicAdd(&sh.count, mine);
            if (ctx.fail) sh.fail = 1;
        }
        __syncthreads();
        nBad = lm_uniform(sh.count);
        __syncthreads();
        if (it == 2) robust = 0;
        if (nEdges < 10) break;
    }
    if (tid == 0) {
        float T[16];
        po_pose_out(sh.S.q, sh.S.t, T);
        for (int k = 0; k < 16; k++) O.Tcw[k] = T[k];
        O.ret = nInitial - nBad;
        O.rounds = rounds;
        O.iterations = sh.S.lm.iterations;
        O.trials = sh.S.lm.trials;
        O.diag[PO_DIAG_REJECTED] = sh.S.lm.rejected;
        O.diag[PO_DIAG_LAST_REJECTED] = lastRejectedRounds;
        O.diag[PO_DIAG_NBAD_STOPS] = sh.S.lm.nBadStops;
        O.diag[PO_DIAG_SMALL_THETA] = sh.S.lm.smallTheta;
        O.diag[PO_DIAG_BIG_THETA] = sh.S.lm.bigTheta;
        O.diag[PO_DIAG_EMPTY_ROUNDS] = emptyRounds;
        O.handBack = (sh.S.lm.ctx.fail || sh.fail) ? 1 : 0;
    }
}

hipError_t drfe_launch_pose_opt(const PoLaunch& L, hipStream_t s)
{
    if (L.nFrames <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pose_opt, dim3(L.nFrames), dim3(PO_THREADS), 0, s, L);
    return hipGetLastError();
}
