/* ransac_device.h — the counting kernel the RANSAC solvers share (k_sim3_count, k_pnp_count): CheckInliers of every row of every
 * solver of a call.  Workgroups over (solver, CHUNK rows), four wavefronts of CHUNK / 4 rows each, one wavefront per row at a
 * time: the correspondences 64 at a time, the ballot of the test is the mask word, its popcount adds to the count.
 *
 * DRFE_*_LDS_CORR: the correspondences of a solver the kernel keeps in LDS, 48 KiB of records in each solver (of a workgroup's 64;
 * a CU's 160 KiB has room for three such workgroups); a larger solver is read from global memory.
 * DRFE_*_CHUNK: rows per workgroup, which is how often a solver's records are staged. */
#ifndef DRFE_RANSAC_DEVICE_H
#define DRFE_RANSAC_DEVICE_H
#ifdef __HIPCC__

#include <hip/hip_runtime.h>
#include <cstdint>
#include "ransac_table.h"

/* a solver's N records into LDS by the whole workgroup: a straight dword copy */
template <int Threads, class Rec>
__device__ __forceinline__ void ransac_stage_lds(Rec* lds, const Rec* corr, int N)
{
    static_assert(sizeof(Rec) % 4 == 0, "a record is whole dwords");
    const uint32_t* src = reinterpret_cast<const uint32_t*>(corr);
    uint32_t* dst = reinterpret_cast<uint32_t*>(lds);
    for (int k = threadIdx.x; k < N * (int)(sizeof(Rec) / 4); k += Threads) dst[k] = src[k];
    __syncthreads();
}

/* CheckInliers of one row by one wavefront: test(record) per lane, the mask words and the count by lane 0 */
template <class Rec, class Test>
__device__ __forceinline__ void ransac_sweep(const Rec* corr, int N, int lane, uint64_t* mask, int32_t* countOut, Test test)
{
    int count = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool ok = i < N && test(corr[i < N ? i : 0]);
        const unsigned long long word = __ballot(ok);
        count += __popcll(word);
        if (lane == 0) mask[base >> 6] = word;
    }
    if (lane == 0) *countOut = count;
}

/* the rows of a counting workgroup: blockIdx.x picks Chunk rows of solver S, each wavefront takes its share of them in turn and
 * calls row(records, N, h, w) — h the row within the solver, w within the compact table — with the records in lds when they
 * fit */
template <int Chunk, int Threads, class Rec, int LdsCorr, class Row>
__device__ __forceinline__ void ransac_count_rows(const RansacSolverHead& S, const Rec* corr, Rec (&lds)[LdsCorr], Row row)
{
    const int h0 = blockIdx.x * Chunk;
    if (h0 >= S.hyp) return;                         /* uniform over the workgroup */
    const int N = S.n;
    if (N <= LdsCorr) {
        ransac_stage_lds<Threads>(lds, corr, N);
        corr = lds;
    }
    const int wave = threadIdx.x >> 6, perWave = Chunk / (Threads / 64);
    for (int j = 0; j < perWave; j++) {
        const int h = h0 + wave * perWave + j;
        if (h >= S.hyp) break;                       /* uniform over the wavefront */
        row(corr, N, h, (size_t)S.hyp0 + h);
    }
}

#endif
#endif
