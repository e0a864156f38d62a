/* manhattan_kernels.hip — Manhattan-frame tracking (Tracking::TrackManhattanFrame, reference src/Tracking.cc:1336-1527) of
 * whole sequences on gfx950, over the SurfaceNormal records drfe_surface_normals_batch left on the device.
 *
 * One workgroup of 256 lanes per sequence; frame t starts from frame t-1's result, so the frames of a sequence run in
 * order and the sequences of a batch side by side.  Per call of a frame:
 *   - conic pass: every lane takes the entries (records, then the frame's lines) e = lane + 256 j, tests all three cones
 *     and keeps a 3-bit cone mask per entry in scratch; the counts are integer, so their order does not matter;
 *   - mean-shift pass, axis by axis (axis a + 1 reads the column axis a wrote): the cone members of the axis are
 *     re-projected, and the (k x, k y, k) terms of the non-NaN ones are compacted into scratch in entry order (ballot +
 *     mbcnt inside a wavefront, per-wavefront counts through LDS, 1 024 entries per barrier pair); three lanes then take
 *     MeanShift's three sums sequentially in entry order, in double, as the reference does (the order defines the bits);
 *   - the 3x3 tail (s_j, the new column, cross product, SVD) on one lane.
 * Entry e is always owned by lane e % 256, so the per-record / per-line bit words are updated without atomics.
 * All arithmetic is manhattan_core.h, shared with the host entry (manhattan.cpp); -ffp-contract=off. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "post_internal.h"
#include "manhattan_core.h"

#define MF_THREADS 256
#define MF_WAVES (MF_THREADS / 64)
#define MF_SUB 4              /* entries per lane between two barriers of the compaction */

__global__ __launch_bounds__(MF_THREADS) void k_manhattan(const drfe_surface_normal* __restrict__ recsAll, int nrec,
                                                         const float* __restrict__ R0, int seqLen,
                                                         const double* __restrict__ dirsAll, const int32_t* __restrict__ loff,
                                                         int nCalls, uint8_t* coneAll, double* sumsAll, size_t scratch,
                                                         float* __restrict__ Rout, drfe_manhattan_info* __restrict__ infoOut,
                                                         uint16_t* __restrict__ rbAll, uint16_t* __restrict__ lbAll)
{
    const int seq = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float sR[9];
    __shared__ int sCnt[3];
    __shared__ int sWave[MF_SUB * MF_WAVES];
    __shared__ double sSum[3];
    __shared__ drfe_manhattan_info sInf;
    uint8_t* cone = coneAll + (size_t)seq * scratch;
    double* sums = sumsAll + (size_t)seq * scratch * 3;
    if (tid < 9) sR[tid] = R0[seq * 9 + tid];

    for (int t = 0; t < seqLen; t++) {
        const size_t f = (size_t)seq * seqLen + t;
        const drfe_surface_normal* recs = recsAll + f * nrec;
        const int l0 = loff[f], nl = loff[f + 1] - l0, ntot = nrec + nl;
        const double* dirs = dirsAll + 3 * (size_t)l0;
        uint16_t* rb = rbAll + f * nrec;
        uint16_t* lb = lbAll + l0;
        for (int e = tid; e < ntot; e += MF_THREADS) {
            if (e < nrec) rb[e] = 0;
            else lb[e - nrec] = 0;
        }
        if (tid == 0) {
            sInf.n_calls = nCalls; sInf.pad = 0;
            for (int k = 0; k < DRFE_MANHATTAN_MAX_CALLS; k++) {
                drfe_manhattan_call& ci = sInf.call[k];
                for (int a = 0; a < 3; a++) { ci.in_cone[a] = 0; ci.n_selected[a] = 0; ci.density[a] = 0.f; }
                ci.threshold = 0; ci.deficient = 0; ci.found = 0; ci.svd = 0; ci.pad = 0;
            }
        }
        for (int call = 0; call < nCalls; call++) {
            if (tid < 3) sCnt[tid] = 0;
            __syncthreads();                                  /* sR of the previous call / frame, sCnt */
            /* ---- conic pass (ProjectSN2Conic for a = 1..3) */
            {
                float M[3][9];
                for (int a = 0; a < 3; a++) mf_axis_rows(sR, a + 1, M[a]);
                int cnt[3] = {0, 0, 0};
                for (int e = tid; e < ntot; e += MF_THREADS) {
                    unsigned bits = 0;
                    float o[3];
                    if (e < nrec) {
                        const float n[3] = {recs[e].normal[0], recs[e].normal[1], recs[e].normal[2]};
                        for (int a = 0; a < 3; a++) {
                            mf_nini_normal(M[a], n, o);
                            if (mf_lambda(o) < DRFE_MF_SIN_NORMAL_CONE) { bits |= 1u << a; cnt[a]++; }
                        }
                        if (bits) rb[e] |= DRFE_MANHATTAN_INLINE_BIT;
                    } else {
                        const double* d = dirs + 3 * (e - nrec);
                        for (int a = 0; a < 3; a++) {
                            mf_nini_line(M[a], d, o);
                            if (mf_lambda(o) < DRFE_MF_SIN_LINE_CONE) bits |= 1u << a;
                        }
                        if (bits) lb[e - nrec] |= DRFE_MANHATTAN_INLINE_BIT;
                    }
                    cone[e] = (uint8_t)bits;
                }
                for (int a = 0; a < 3; a++) {
                    int v = cnt[a];
                    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
                    if (lane == 0 && v) atomicAdd(&sCnt[a], v);
                }
            }
            __syncthreads();
            drfe_manhattan_call& ci = sInf.call[call];
            if (tid == 0) {
                int thr = nrec / 20;
                int s0 = sCnt[0], s1 = sCnt[1], s2 = sCnt[2], tt;
                ci.in_cone[0] = s0; ci.in_cone[1] = s1; ci.in_cone[2] = s2;
                if (s0 > s1) tt = s0, s0 = s1, s1 = tt;
                if (s1 > s2) tt = s1, s1 = s2, s2 = tt;
                if (s0 > s1) tt = s0, s0 = s1, s1 = tt;
                if (s1 < thr) { thr = (s1 + s0) / 2; ci.deficient = 1; }
                ci.threshold = thr;
            }
            __syncthreads();
            const int thr = ci.threshold;
            /* ---- mean-shift pass (ProjectSN2MF + MeanShift), axis by axis on the R being updated */
            for (int a = 1; a <= 3; a++) {
                float M[9];
                mf_axis_rows(sR, a, M);
                const unsigned bit = 1u << (a - 1);
                const uint16_t pushed = (uint16_t)(1u << (3 * call + a - 1));
                int base = 0;
                for (int c0 = 0; c0 < ntot; c0 += MF_SUB * MF_THREADS) {
                    double w[MF_SUB][3];
                    bool v[MF_SUB];
                    int inWave[MF_SUB];
#pragma unroll
                    for (int u = 0; u < MF_SUB; u++) {
                        const int e = c0 + u * MF_THREADS + tid;
                        v[u] = false;
                        if (e < ntot && (cone[e] & bit)) {
                            float o[3];
                            if (e < nrec) {
                                const float n[3] = {recs[e].normal[0], recs[e].normal[1], recs[e].normal[2]};
                                mf_nini_normal(M, n, o);
                            } else {
                                mf_nini_line(M, dirs + 3 * (e - nrec), o);
                            }
                            const double lam = mf_lambda(o);
                            if (lam < DRFE_MF_SIN_MS_CONE) {
                                if (e < nrec) rb[e] |= pushed;
                                else lb[e - nrec] |= pushed;
                                double mx, my;
                                if (mf_mj(lam, o, &mx, &my)) {
                                    mf_weight(mx, my, w[u]);
                                    v[u] = true;
                                }
                            }
                        }
                        const unsigned long long bal = __ballot(v[u]);
                        inWave[u] = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                        if (lane == 0) sWave[u * MF_WAVES + wave] = __popcll(bal);
                    }
                    __syncthreads();
                    int run = base, total = 0;
#pragma unroll
                    for (int u = 0; u < MF_SUB; u++) {
                        int before = 0;
                        for (int k = 0; k < MF_WAVES; k++) {
                            const int cnt = sWave[u * MF_WAVES + k];
                            if (k < wave) before += cnt;
                            total += cnt;
                        }
                        if (v[u]) {
                            const size_t pos = (size_t)(run + before + inWave[u]);
                            sums[pos] = w[u][0];
                            sums[scratch + pos] = w[u][1];
                            sums[2 * scratch + pos] = w[u][2];
                        }
                        run = base + total;
                    }
                    base += total;
                    __syncthreads();                          /* sWave is rewritten by the next chunk */
                }
                const int n = base;
                if (tid == 0) ci.n_selected[a - 1] = n;
                if (n > thr) {
                    if (tid < 3) {                            /* nominator.x, nominator.y, denominator: in entry order */
                        const double* p = sums + (size_t)tid * scratch;
                        double s = 0.0;
                        int j = 0;
                        for (; j + 8 <= n; j += 8) {
                            double q[8];
#pragma unroll
                            for (int u = 0; u < 8; u++) q[u] = p[j + u];
#pragma unroll
                            for (int u = 0; u < 8; u++) s += q[u];
                        }
                        for (; j < n; j++) s += p[j];
                        sSum[tid] = s;
                    }
                    __syncthreads();
                    if (tid == 0) {
                        float col[3];
                        if (mf_axis_tail(M, sSum[0], sSum[1], sSum[2], n, col, &ci.density[a - 1])) {
                            ci.found |= (int)bit;
                            for (int r = 0; r < 3; r++) sR[r * 3 + a - 1] = col[r];
                        }
                    }
                }
                __syncthreads();                              /* sR for the next axis */
            }
            if (tid == 0) ci.svd = mf_assemble(sR, ci.found) ? 1 : 0;
        }
        __syncthreads();
        if (tid < 9) Rout[f * 9 + tid] = sR[tid];
        if (tid == 0) infoOut[f] = sInf;
    }
}

hipError_t drfe_launch_manhattan(const drfe_surface_normal* d_recs, int nrec, const float* d_R0, int nseq, int seq_len,
                                 const double* d_dirs, const int32_t* d_loff, int n_calls, uint8_t* d_cone, double* d_sums,
                                 size_t scratch, float* d_R, drfe_manhattan_info* d_info, uint16_t* d_rbits, uint16_t* d_lbits,
                                 hipStream_t s)
{
    hipLaunchKernelGGL(k_manhattan, dim3(nseq), dim3(MF_THREADS), 0, s, d_recs, nrec, d_R0, seq_len, d_dirs, d_loff, n_calls,
                       d_cone, d_sums, scratch, d_R, d_info, d_rbits, d_lbits);
    return hipGetLastError();
}
