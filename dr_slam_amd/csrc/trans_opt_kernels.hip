/* trans_opt_kernels.hip — Optimizer::TranslationOptimization (reference src/Optimizer.cc:3211-3980) on gfx950, every frame of a
 * call, driven by trans_opt.cpp.  DESIGN.md section 21.
 *   k_trans_opt  one workgroup of 256 lanes per frame runs the frame's four rounds, classification included, in one launch.
 *                The caller's arrays are staged as they are: the lane that evaluates an edge forms it (R_cw * Xw in float,
 *                toPlane3D and rotateNormal, information, delta) and reads and writes its outlier flag in the caller's layout.
 *                A point or line edge is an add and a projection, 256 edges (a chunk) at a time; when the system is built the
 *                lane adds the three translation columns of the Jacobian and the edge's nine terms of H's translation block
 *                and b, written to LDS.  Plane edges come 32 at a time: the six perturbed errors of each edge's numeric
 *                Jacobian (dimensions 3..5) in six lanes (192 of the 256), the edge's own error in a lane of the fourth
 *                wavefront, which then forms the Jacobian and the nine terms.  Lanes 0..8 each own one of the nine sums and
 *                add the chunk's terms edge after edge; lane 0 owns the robust chi2 the same way.  The other 18 entries of H
 *                and b are +0.0 while every term is finite; a lane that meets one that is not says so and the frame goes back
 *                to the host, which runs the full form.  Lane 0 runs the step control, the 6x6 LDLT and the update (PoLM in
 *                LDS), exactly as k_pose_opt's does.
 * No float or double atomics; a sum is never split across lanes.  -ffp-contract=off, as the host entry. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "trans_opt_internal.h"
#include "lm_device.h"

namespace {

struct ToShared {
    double term[TO_TERMS * TO_TERM_STRIDE];
    double chi[TO_THREADS];
    double pert[TO_PLANE_GROUP * 6 * 3];
    PoLM S;
    ToFrame F;
    uint8_t planeAt[3 * DRFE_POSE_OPT_MAX_PLANES];
    int32_t ctl;                   /* the decision of the step control every lane branches on */
    int32_t count;                 /* nActive, then nBad */
    int32_t fail;                  /* a lane could not certify a transcendental, or met a term that is not finite */
};

/* what lanes 0..8 and lane 0 add after a chunk's terms are in LDS */
using ToSums = LmSums<TO_TERMS, TO_H_TERMS, TO_TERM_STRIDE>;

/* computeActiveErrors and activeRobustChi2; with `build` also linearizeOplus and constructQuadraticForm into S.lm.H / S.lm.b.
 * Returns the robust chi2 in lane 0.  Every lane of the workgroup calls it. */
__device__ double to_pass(ToShared& sh, const ToLaunch& L, int robust, bool build)
{
    const int tid = threadIdx.x;
    const ToView& V = L.view;
    const ToFrame& F = sh.F;
    LmCtx ctx = {0, 0};
    int fin = 1;
    double q[4], t[3];
    for (int k = 0; k < 4; k++) q[k] = sh.S.q[k];
    for (int k = 0; k < 3; k++) t[k] = sh.S.t[k];
    ToSums sums = {0.0, 0.0};
    const int plane0 = F.nPoints + 2 * F.nLines;
    for (int base = 0; base < plane0; base += TO_THREADS) {
        const int k = base + tid;
        const bool act = k < plane0 && !*to_flag(V, F, sh.planeAt, k);
        double c = 0.0;
        if (act) {
            PoEdge E;
            to_make_edge(V, F, sh.planeAt, k, E);
            double e[3];
            to_edge_error(ctx, E, F.cam, t, e);
            double* err = L.err + 3 * to_err_slot(F, sh.planeAt, L.lineErr0, L.planeErr0, k);
            for (int r = 0; r < 3; r++) err[r] = e[r];
            c = po_chi_term(E, e, robust);
            if (build) {
                double J[3][3], term[TO_TERMS];
                to_edge_jacobian(E, F.cam, t, J);
                fin &= to_edge_terms(E, J, e, robust, term);
                for (int r = 0; r < TO_TERMS; r++) sh.term[r * TO_TERM_STRIDE + tid] = term[r];
            }
        } else if (build) {
            for (int r = 0; r < TO_TERMS; r++) sh.term[r * TO_TERM_STRIDE + tid] = 0.0;
        }
        sh.chi[tid] = c;
        __syncthreads();
        sums.add(sh.term, sh.chi, plane0 - base < TO_THREADS ? plane0 - base : TO_THREADS, build);
        __syncthreads();
    }
    for (int base = plane0; base < F.nEdges; base += TO_PLANE_GROUP) {
        const int cnt = F.nEdges - base < TO_PLANE_GROUP ? F.nEdges - base : TO_PLANE_GROUP;
        const int own = tid - 6 * TO_PLANE_GROUP;                  /* lanes 192..223: the edge's own error, then its terms */
        double e[3] = {0.0, 0.0, 0.0};
        PoEdge E;
        bool act = false;
        if (tid < 6 * TO_PLANE_GROUP) {
            const int g = tid / 6, pr = tid % 6;
            if (build && g < cnt && !*to_flag(V, F, sh.planeAt, base + g)) {
                double pe[3];
                to_make_edge(V, F, sh.planeAt, base + g, E);
                to_plane_perturbed(ctx, E, q, t, pr >> 1, pr & 1, pe);
                for (int r = 0; r < 3; r++) sh.pert[tid * 3 + r] = pe[r];
            }
        } else if (own < TO_PLANE_GROUP) {
            act = own < cnt && !*to_flag(V, F, sh.planeAt, base + own);
            double c = 0.0;
            if (act) {
                const int k = base + own;
                to_make_edge(V, F, sh.planeAt, k, E);
                to_edge_error(ctx, E, F.cam, t, e);
                double* err = L.err + 3 * to_err_slot(F, sh.planeAt, L.lineErr0, L.planeErr0, k);
                for (int r = 0; r < 3; r++) err[r] = e[r];
                c = po_chi_term(E, e, robust);
            }
            sh.chi[own] = c;
        }
        __syncthreads();
        if (build && own >= 0 && own < TO_PLANE_GROUP) {
            double term[TO_TERMS];
            if (act) {
                double J[3][3];
                const double scalar = lm_numeric_scalar();
                for (int d = 0; d < 3; d++)
                    for (int r = 0; r < 3; r++)
                        J[r][d] = scalar * (sh.pert[((own * 6 + 2 * d) * 3) + r] - sh.pert[((own * 6 + 2 * d + 1) * 3) + r]);
                fin &= to_edge_terms(E, J, e, robust, term);
            } else {
                for (int r = 0; r < TO_TERMS; r++) term[r] = 0.0;
            }
            for (int r = 0; r < TO_TERMS; r++) sh.term[r * TO_TERM_STRIDE + own] = term[r];
        }
        __syncthreads();
        sums.add(sh.term, sh.chi, cnt, build);
        __syncthreads();
    }
    if (ctx.fail || !fin) sh.fail = 1;
    if (build) {
        if (tid < PO_H_TERMS) sh.S.lm.H[tid] = 0.0;
        if (tid < 6) sh.S.lm.b[tid] = 0.0;
        __syncthreads();
        if (tid < TO_H_TERMS) sh.S.lm.H[to_h_index(tid)] = sums.acc;
        else if (tid < TO_TERMS) sh.S.lm.b[3 + tid - TO_H_TERMS] = sums.acc;
        __syncthreads();
    }
    return sums.chi;
}

}  // namespace

__global__ __launch_bounds__(TO_THREADS) void k_trans_opt(const ToLaunch L)
{
    __shared__ ToShared sh;
    const int tid = threadIdx.x;
    const int f = blockIdx.x;
    const ToView& V = L.view;
    PoFrameOut& O = L.out[f];
    const float* Tcw = V.Tcw + 16 * (size_t)f;
    if (tid == 0) {
        to_frame(V, f, sh.F);
        lm_init(sh.S.lm, 0);
        sh.fail = 0;
    }
    __syncthreads();
    const ToFrame& F = sh.F;
    const int nInitial = lm_uniform(F.nPoints);
    if (nInitial < 3) {                                 /* uniform: the pose untouched, the flags false (zero before the launch) */
        if (tid < 16) O.Tcw[tid] = Tcw[tid];
        return;
    }
    if (tid == 0) {
        sh.F.nPlaneEdges = to_plane_table(V, f, sh.F, sh.planeAt);
        sh.F.nEdges = sh.F.nPoints + 2 * sh.F.nLines + sh.F.nPlaneEdges;
    }
    __syncthreads();
    const int nEdges = lm_uniform(F.nEdges);
    int robust = 1, rounds = 0, lastRejectedRounds = 0, emptyRounds = 0, nBad = 0;
    for (int it = 0; it < 4; it++) {
        if (tid == 0) {
            mp_to_se3quat(Tcw, sh.S.q, sh.S.t);
            sh.S.lm.lastRejected = 0;
            sh.count = 0;
        }
        __syncthreads();
        {
            int mine = 0;
            for (int k = tid; k < F.nEdges; k += TO_THREADS) mine += *to_flag(V, F, sh.planeAt, k) ? 0 : 1;
            if (mine) atomicAdd(&sh.count, mine);
        }
        __syncthreads();
        const int nActive = lm_uniform(sh.count);
        __syncthreads();
        if (nActive == 0) emptyRounds++;
        else lm_iterations(sh.S, sh.ctl, 10, [&](bool build) { return to_pass(sh, L, robust, build); });
        rounds++;
        if (tid == 0) {
            if (sh.S.lm.lastRejected) lastRejectedRounds++;
            sh.count = 0;
        }
        __syncthreads();
        /* the classification: a point or a plane edge by one lane, a line's two ends by one lane; an outlier's error is
         * computed again, an inlier's is what the last computeActiveErrors left.  nLineBad is not returned */
        {
            LmCtx ctx = {0, 0};
            double t[3];
            for (int k = 0; k < 3; k++) t[k] = sh.S.t[k];
            const int line0 = F.nPoints, plane0 = F.nPoints + 2 * F.nLines;
            int mine = 0;
            for (int j = tid; j < F.nPoints + F.nPlaneEdges; j += TO_THREADS) {
                const int k = j < F.nPoints ? j : plane0 + (j - F.nPoints);
                PoEdge E;
                to_make_edge(V, F, sh.planeAt, k, E);
                uint8_t* flag = to_flag(V, F, sh.planeAt, k);
                double* err = L.err + 3 * to_err_slot(F, sh.planeAt, L.lineErr0, L.planeErr0, k);
                double e[3];
                if (*flag) {
                    to_edge_error(ctx, E, F.cam, t, e);
                    for (int r = 0; r < 3; r++) err[r] = e[r];
                } else {
                    for (int r = 0; r < 3; r++) e[r] = err[r];
                }
                const int out = po_outlier(E, e);
                *flag = (uint8_t)out;
                mine += out;
            }
            for (int l = tid; l < F.nLines; l += TO_THREADS) {
                const int k = line0 + 2 * l;
                PoEdge E1, E2;
                to_make_edge(V, F, sh.planeAt, k, E1);
                to_make_edge(V, F, sh.planeAt, k + 1, E2);
                uint8_t* flag = to_flag(V, F, sh.planeAt, k);
                double* err = L.err + 3 * to_err_slot(F, sh.planeAt, L.lineErr0, L.planeErr0, k);   /* the end's follows */
                double e1[3], e2[3];
                if (*flag) {
                    to_edge_error(ctx, E1, F.cam, t, e1);
                    to_edge_error(ctx, E2, F.cam, t, e2);
                    for (int r = 0; r < 3; r++) { err[r] = e1[r]; err[3 + r] = e2[r]; }
                } else {
                    for (int r = 0; r < 3; r++) { e1[r] = err[r]; e2[r] = err[3 + r]; }
                }
                *flag = (uint8_t)(po_outlier(E1, e1) || po_outlier(E2, e2));
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

hipError_t drfe_launch_trans_opt(const ToLaunch& L, hipStream_t s)
{
    if (L.nFrames <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_trans_opt, dim3(L.nFrames), dim3(TO_THREADS), 0, s, L);
    return hipGetLastError();
}
