/* lm_device.h — what the optimiser kernels (k_pose_opt, k_trans_opt, k_sim3_opt) share around lm_core.h's step control: one
 * workgroup per problem, lane 0 runs the control on the vertex in LDS, every lane walks the passes over the edges.  Here are the
 * iterations of an optimize() call with their barriers (lm_iterations) and the ordered sums of a chunk's terms (LmSums).  Device
 * only.  DESIGN.md section 24 states the barrier rule this header holds for its three callers. */
#ifndef DRFE_LM_DEVICE_H
#define DRFE_LM_DEVICE_H

#include <hip/hip_runtime.h>
#include "lm_core.h"

/* a value every lane of the workgroup holds alike, as a scalar: the branches on it are scalar branches, so that no wavefront
 * walks a barrier of a loop it has left with its lanes masked off */
__device__ inline int lm_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

/* optimize(iters) of a vertex V (PoLM, SoLM) in LDS; ctl is the control word beside it.  Every lane of the workgroup calls it, and
 * pass(build) is the kernel's pass over its edges, which every lane calls: computeActiveErrors and activeRobustChi2, with `build`
 * also the system into v.lm.H / v.lm.b; it ends behind a barrier and returns the robust chi2 at least in lane 0.  Every path
 * through here crosses the same barriers in every lane: what a branch depends on is lane 0's decision, written to ctl, read
 * between two barriers and made a scalar. */
template <class V, class Pass>
__device__ void lm_iterations(V& v, int32_t& ctl, int iters, Pass pass)
{
    const int tid = threadIdx.x;
    if (tid == 0) ctl = 0;
    for (int i = 0; i < iters; i++) {
        const double chi = pass(true);
        if (tid == 0) lm_begin(v.lm, i, chi);
        /* this barrier keeps lane 0's block above apart from the trial loop: without it the compiler threads the block into
         * the loop's first trip, the other lanes walk a whole pass and the loop's barriers with lane 0 masked off, read the
         * control word of the iteration before and may leave the loop a trip early */
        __syncthreads();
        int more;
        do {
            if (tid == 0) lm_step(v);
            __syncthreads();
            const double tempChi = pass(false);
            if (tid == 0) ctl = lm_judge(v, tempChi);
            __syncthreads();
            more = lm_uniform(ctl);
            __syncthreads();
        } while (more);
        if (tid == 0) ctl = lm_end(v.lm);
        __syncthreads();
        const int ok = lm_uniform(ctl);
        __syncthreads();
        if (!ok) break;
    }
}

/* what lanes 0..TERMS-1 and lane 0 add after a chunk's terms are in LDS, edge after edge: lane r owns row r of `term` (STRIDE
 * doubles a row), the first H_TERMS rows are added (H), the others subtracted (b); lane 0 also owns the robust chi2 */
template <int TERMS, int H_TERMS, int STRIDE>
struct LmSums {
    double acc, chi;
    __device__ void add(const double* term, const double* chiTerm, int cnt, bool build)
    {
        const int tid = threadIdx.x;
        if (tid == 0)
            for (int j = 0; j < cnt; j++) chi += chiTerm[j];
        if (build && tid < TERMS) {
            const double* row = term + tid * STRIDE;
            if (tid < H_TERMS)
                for (int j = 0; j < cnt; j++) acc += row[j];
            else
                for (int j = 0; j < cnt; j++) acc -= row[j];
        }
    }
};

#endif
