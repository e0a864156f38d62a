/* lines_3d_kernels.hip — Frame::isLineGood's 3-D line lifting (reference src/Frame.cc:481-558, src/LineExtractor.cpp:1157-1470)
 * on gfx950 for every key line of every frame of a call, driven by lines_3d_batch.cpp.  DESIGN.md section 18.
 *   k_line3d_prepare  one wavefront per key line, lane j = sample j: placement, depth gather, unprojection; the ballot of the
 *                     samples that lift, compacted in order by prefix popcount; compPt3dCov per lane.
 *   k_line3d_ransac   one wavefront per frame, walking the frame's key lines in order, because line k's rand() draws start
 *                     where lines 0 .. k-1 stopped.  Lane i owns lifted sample i; a ballot of the Mahalanobis test is the
 *                     inlier set; verify3dLine runs on the mask.  Leaves the best mask and its pair.
 *   k_line3d_finish   one wavefront per key line: the refit loop (ordered sums over the mask, the same in every lane), the two
 *                     extreme inliers, isLineGood's gates, the end-point depth, the outputs.
 * Arithmetic is line3d_core.h's, as on the host.  No float or double atomics, no sum split across lanes: an extreme is a
 * minimum (exact in any order) and the first lane that holds it.  -ffp-contract=off, as the host entry. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "line3d_internal.h"

namespace {

__device__ __forceinline__ bool bit(uint64_t m, int i) { return (m >> i) & 1; }
__device__ __forceinline__ int first_of(uint64_t m) { return __ffsll((unsigned long long)m) - 1; }

/* L3Extremes over the lanes of `mask` in lane order: the first lane of the least v below 100 and of the largest above -100,
 * the mask's first lane where no v beats the bound.  mask is not empty; every lane is active. */
__device__ void wave_extremes(double v, uint64_t mask, int lane, int* lo, int* hi)
{
    const bool in = bit(mask, lane);
    const bool cl = in && v < 100.0, ch = in && v > -100.0;
    double mn = cl ? v : HUGE_VAL, mx = ch ? v : -HUGE_VAL;
    for (int o = 32; o; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o));
        mx = fmax(mx, __shfl_xor(mx, o));
    }
    const uint64_t bl = __ballot(cl && v == mn), bh = __ballot(ch && v == mx);
    *lo = first_of(bl ? bl : mask);
    *hi = first_of(bh ? bh : mask);
}

/* verify3dLine over the inliers `mask` of the pair A, B; pos: the wavefront's positions by lane (LDS) */
__device__ bool wave_verify(const L3P* pos, uint64_t mask, int lane, const L3P& A, const L3P& B)
{
    int lo, hi;
    wave_extremes(l3_dot(pos[lane] - A, B - A), mask, lane, &lo, &hi);
    L3Cells g;
    if (!l3_cells_begin(pos[lo], pos[hi], A, B, &g)) return false;
    const bool in = bit(mask, lane);
    const unsigned cell = l3_cell_of(g, pos[lane]);
    int populated = 0;
    for (unsigned c = 0; c < 10; c++) populated += __ballot(in && cell == c) != 0;
    return l3_cells_pass(populated);
}

/* lane i's lifted sample of a key line (zeros past the last) and every position in LDS */
__device__ L3Point load_points(const L3Point* pts, int n, int lane, L3P* pos)
{
    L3Point pt{};
    if (lane < n) pt = pts[lane];
    __syncthreads();               /* the previous line's readers are done */
    pos[lane] = pt.pos;
    __syncthreads();
    return pt;
}

}  // namespace

__global__ __launch_bounds__(64) void k_line3d_prepare(const Line3dLaunch L)
{
    const int f = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
    if (i >= L.nLines[f]) return;
    const size_t slot = (size_t)f * L.cap + i;
    const drfe_keyline kl = L.lines[slot];
    double len;
    const int numSmp = l3_num_samples(kl, &len);
    L3P p{0, 0, 0};
    const bool ok = numSmp && lane <= numSmp &&
                    l3_sample(kl, lane, numSmp, L.depth + (size_t)f * L.frameStride, L.w, L.h, L.stride, L.cx, L.cy, L.invfx, L.invfy, &p);
    const uint64_t m = __ballot(ok);
    const int n = __popcll(m);
    if (ok && n >= L3_MIN_POINTS)
        L.pts[slot * L3_MAX_SAMPLES + __popcll(m & ((1ull << lane) - 1))] = l3_comp_pt3d_cov(p, L.f);
    if (lane == 0) L.nPts[slot] = n;
}

__global__ __launch_bounds__(64) void k_line3d_ransac(const Line3dLaunch L)
{
    __shared__ L3P pos[64];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int nl = L.nLines[f];
    const int32_t* draws = L.draws + (size_t)f * L.cap * DRFE_LINE3D_DRAWS;
    int at = 0;                    /* draws the lines before this one consumed */
    L3FrameStats st{0, 0, 0, 0};
    for (int i = 0; i < nl; i++) {
        const size_t slot = (size_t)f * L.cap + i;
        const int n = L.nPts[slot];
        L3Best best{0, {0, 0, 0}, {0, 0, 0}};
        if (n >= L3_MIN_POINTS) {
            st.ransacLines++;
            const L3Point pt = load_points(L.pts + slot * L3_MAX_SAMPLES, n, lane, pos);
            const int32_t mine = lane < DRFE_LINE3D_DRAWS ? draws[at + lane] : 0;   /* at <= i * DRFE_LINE3D_DRAWS */
            int idx = lane;        /* indexes[lane], persistent over the line's iterations */
            int bestCount = 0, used = 0;
            const int maxIt = l3_max_iterations(n);
            for (int it = 0; it < maxIt; it++) {
                st.iterations++;
                for (int k = 0; k < 2; k++) {                      /* random_unique: swap indexes[k], indexes[o] */
                    const int o = l3_swap_with(k, __shfl(mine, used++), n);
                    const int a = __shfl(idx, k), b = __shfl(idx, o);
                    if (lane == k) idx = b;
                    if (lane == o) idx = a;
                }
                const L3P A = pos[__shfl(idx, 0)], B = pos[__shfl(idx, 1)];
                if (l3_norm(B - A) < L3_EPS) { st.coincident++; continue; }
                const uint64_t mask = __ballot(lane < n && l3_is_inlier(pt, A, B));
                const int count = __popcll(mask);
                if (count > bestCount) {
                    if (wave_verify(pos, mask, lane, A, B)) {
                        best.mask = mask; best.A = A; best.B = B;
                        bestCount = count;
                    } else st.rejected++;
                }
                if (l3_enough(bestCount, n)) break;
            }
            at += used;
        }
        if (lane == 0) L.best[slot] = best;
    }
    if (lane == 0) L.frameStats[f] = st;
}

__global__ __launch_bounds__(64) void k_line3d_finish(const Line3dLaunch L)
{
    __shared__ L3P pos[64];
    const int f = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
    if (i >= L.nLines[f]) return;
    const size_t slot = (size_t)f * L.cap + i;
    const int n = L.nPts[slot];
    float depthLine = -1.0f;
    L3P A{0, 0, 0}, B{0, 0, 0};
    int nInliers = 0;
    bool good = false;
    if (n >= L3_MIN_POINTS) {
        const L3Point pt = load_points(L.pts + slot * L3_MAX_SAMPLES, n, lane, pos);
        const L3Best best = L.best[slot];
        uint64_t cur = best.mask;
        if (__popcll(cur) >= 2) {
            L3P m = (best.A + best.B) * 0.5, d = best.B - best.A;
            while (true) {         /* refit on the inliers and reselect while the set grows */
                L3P tm{0, 0, 0};
                for (uint64_t q = cur; q; q &= q - 1) tm = tm + pos[first_of(q)];
                tm = l3_mean(tm, __popcll(cur));
                double s[6] = {0, 0, 0, 0, 0, 0};
                for (uint64_t q = cur; q; q &= q - 1) l3_scatter_add(s, pos[first_of(q)] - tm);
                const L3P td = l3_direction(s);
                const uint64_t tmp = __ballot(lane < n && l3_is_inlier(pt, tm, tm + td));
                if (__popcll(tmp) > __popcll(cur)) { cur = tmp; m = tm; d = td; }
                else break;
            }
            int lo, hi;
            wave_extremes(l3_dot(pt.pos - m, d), cur, lane, &lo, &hi);
            A = pos[lo];
            B = pos[hi];
        }
        nInliers = __popcll(cur);
        const drfe_keyline kl = L.lines[slot];
        double len;
        (void)l3_num_samples(kl, &len);
        if (l3_accept(nInliers, len, A, B)) {
            depthLine = l3_end_point_depth(kl, L.depth + (size_t)f * L.frameStride, L.w, L.h, L.stride);
            good = true;
        }
    }
    if (lane == 0) {
        L.depthLine[slot] = depthLine;
        double* o = L.lines3d + 6 * slot;
        o[0] = good ? A.x : 0.0; o[1] = good ? A.y : 0.0; o[2] = good ? A.z : 0.0;
        o[3] = good ? B.x : 0.0; o[4] = good ? B.y : 0.0; o[5] = good ? B.z : 0.0;
        L.nInliers[slot] = nInliers;
        if (good) atomicAdd(L.nGood + f, 1);
    }
}

hipError_t drfe_launch_line3d(const Line3dLaunch& L, hipStream_t s)
{
    if (L.nframes <= 0) return hipSuccess;
    if (L.maxLines > 0) hipLaunchKernelGGL(k_line3d_prepare, dim3(L.maxLines, L.nframes), dim3(64), 0, s, L);
    hipLaunchKernelGGL(k_line3d_ransac, dim3(L.nframes), dim3(64), 0, s, L);
    if (L.maxLines > 0) hipLaunchKernelGGL(k_line3d_finish, dim3(L.maxLines, L.nframes), dim3(64), 0, s, L);
    return hipGetLastError();
}
