/* map_plane_kernels.hip — MapPlane::UpdateCoefficientsAndPoints (reference src/MapPlane.cc:298-371) on the resident plane maps
 * of drfe_plane_map_upload, on gfx950.  One round of updates (at most one per map plane) is three launches around the
 * unchanged pcl::VoxelGrid of voxel_kernels.hip (map_plane.cpp drives them):
 *   k_mp_gather   one workgroup row per input segment: a frame or keyframe cloud moved into world by its pose
 *                 (map_plane_core.h: the pose's 4x4 from thread 0 through LDS, then one lane per point, f64 multiply-add as
 *                 written, no FMA), or the plane's resident cloud copied as is; each job's segments lie back to back, in the
 *                 reference's concatenation order;
 *   k_voxel_grid  over the jobs (drfe_launch_voxel_grid);
 *   k_mp_commit   the centroids of every job the device finished into the plane's slot of the arena, and the slot's end.
 * k_mp_move copies every plane's cloud into a new arena when slots must grow.  -ffp-contract=off. */
#include <hip/hip_runtime.h>
#include <cstdint>
#include "plane_map_internal.h"
#include "map_plane_core.h"

#define MP_THREADS 256
#define MP_MAX_ROWS 256           /* workgroups per segment / job (grid-stride beyond) */

__global__ __launch_bounds__(MP_THREADS) void k_mp_gather(const MpSeg* __restrict__ segs, const float* __restrict__ poses,
                                                          const float* __restrict__ src, const float* __restrict__ arena,
                                                          float* __restrict__ in)
{
    __shared__ double T[16];
    const MpSeg g = segs[blockIdx.x];
    if (g.form != MP_SEG_RESIDENT && threadIdx.x == 0) {
        if (g.form == MP_SEG_FRAME) mp_pose_update(poses + 16 * (size_t)g.pose, T);
        else mp_pose_rebuild(poses + 16 * (size_t)g.pose, T);
    }
    __syncthreads();
    for (int p = blockIdx.y * MP_THREADS + threadIdx.x; p < g.n; p += gridDim.y * MP_THREADS) {
        float* o = in + 3 * ((size_t)g.dst + p);
        if (g.form == MP_SEG_RESIDENT) {
            const float* q = arena + 3 * ((size_t)g.src + p);
            o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        } else {
            const float* q = src + 3 * ((size_t)g.src + p);
            mp_transform_point(T, q[0], q[1], q[2], o);
        }
    }
}

__global__ __launch_bounds__(MP_THREADS) void k_mp_commit(const MpCommit* __restrict__ jobs, const int* __restrict__ counts,
                                                          const float* __restrict__ out, float* __restrict__ arena,
                                                          int32_t* __restrict__ cloudEnd)
{
    const MpCommit j = jobs[blockIdx.x];
    const int n = counts[blockIdx.x];
    if (n < 0 || n > j.cap) return;                   /* handed back to the host (map_plane.cpp) */
    for (int p = blockIdx.y * MP_THREADS + threadIdx.x; p < 3 * n; p += gridDim.y * MP_THREADS)
        arena[3 * (size_t)j.dstBeg + p] = out[3 * (size_t)j.inOff + p];
    if (blockIdx.y == 0 && threadIdx.x == 0) cloudEnd[j.plane] = j.dstBeg + n;
}

__global__ __launch_bounds__(MP_THREADS) void k_mp_move(const int4* __restrict__ moves, const float* __restrict__ from,
                                                        float* __restrict__ to)
{
    const int4 m = moves[blockIdx.x];                 /* old begin, new begin, points */
    for (int p = blockIdx.y * MP_THREADS + threadIdx.x; p < 3 * m.z; p += gridDim.y * MP_THREADS)
        to[3 * (size_t)m.y + p] = from[3 * (size_t)m.x + p];
}

static int mp_rows(int64_t floats) { return (int)std::max<int64_t>(1, std::min<int64_t>((floats + MP_THREADS - 1) / MP_THREADS, MP_MAX_ROWS)); }

hipError_t drfe_launch_map_plane_gather(const MpSeg* segs, int nseg, int maxN, const float* poses, const float* src,
                                        const float* arena, float* in, hipStream_t s)
{
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_mp_gather, dim3(nseg, mp_rows(maxN)), dim3(MP_THREADS), 0, s, segs, poses, src, arena, in);
    return hipGetLastError();
}

hipError_t drfe_launch_map_plane_commit(const MpCommit* jobs, int njobs, int maxN, const int* counts, const float* out, float* arena,
                                        int32_t* cloudEnd, hipStream_t s)
{
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_mp_commit, dim3(njobs, mp_rows(3 * (int64_t)maxN)), dim3(MP_THREADS), 0, s, jobs, counts, out, arena, cloudEnd);
    return hipGetLastError();
}

hipError_t drfe_launch_map_plane_move(const int4* moves, int nplanes, int maxN, const float* from, float* to, hipStream_t s)
{
    if (nplanes <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_mp_move, dim3(nplanes, mp_rows(3 * (int64_t)maxN)), dim3(MP_THREADS), 0, s, moves, from, to);
    return hipGetLastError();
}
