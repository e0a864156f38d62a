/* lmap_device.h — the two workgroup primitives that lmap_kernels.hip and conn_kernels.hip share: an order-preserving rank of set
 * flags and an exclusive prefix, both over the LMAP_THREADS threads of a workgroup in thread order.  Every thread calls them. */
#ifndef DRFE_LMAP_DEVICE_H
#define DRFE_LMAP_DEVICE_H

#include "lmap_internal.h"

/* position of this lane's set flag among the workgroup's set flags in thread order; *total their number, *ballot the wave's */
__device__ inline int block_rank(bool flag, int32_t* shWave, int* total, unsigned long long* ballot)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) shWave[w] = __popcll(b);
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < LMAP_THREADS / 64; k++) {
        const int c = shWave[k];
        if (k < w) base += c;
        tot += c;
    }
    *total = tot;
    *ballot = b;
    return base + before;
}

/* exclusive prefix of v in thread order; *total the sum */
__device__ inline int32_t block_excl_scan(int32_t v, int32_t* sh, int32_t* total)
{
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int w = 1; w < LMAP_THREADS; w <<= 1) {
        const int32_t add = tid >= w ? sh[tid - w] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    *total = sh[LMAP_THREADS - 1];
    return sh[tid] - v;
}

#endif
