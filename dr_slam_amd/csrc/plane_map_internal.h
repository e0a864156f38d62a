/* plane_map_internal.h — the device-resident plane maps shared by plane association (plane_match.cpp) and map upkeep
 * (map_plane.cpp).  Map plane j of all maps owns the arena points [beg[j], beg[j] + cnt[j]) inside its slot of cap[j] points;
 * the host keeps the exact count of every plane (updates report it back), so the association batch sizes its work list from
 * it.  DESIGN.md sections 12 and 13. */
#ifndef DRFE_PLANE_MAP_INTERNAL_H
#define DRFE_PLANE_MAP_INTERNAL_H

#include "post_internal.h"
#include "stage_layout.h"

#include <algorithm>
#include <string>
#include <vector>

/* Every buffer of the maps and batches holds at least 16 bytes: grow `b` to n elements, or to 16 bytes if that is more. */
template <class T, bool Pinned>
static inline hipError_t drfe_pm_reserve(HipBuf<T, Pinned>& b, size_t n)
{
    return b.grow(std::max(n, 16 / sizeof(T)));
}

struct PmBuffers {
    /* the resident maps: per plane coefficients, bad flag and the slot of its cloud in the arena (device copies of the host
     * mirrors below; cloudEnd is also written by the update's commit kernel) */
    DevBuf<float> mapCoefs, cloud, points;          /* 4 per plane, xyz per cloud point, xyz per map point */
    DevBuf<uint8_t> mapBad;
    DevBuf<int32_t> cloudBeg, cloudEnd;
    std::vector<int32_t> planeOff, pointOff;
    std::vector<float> coefsH;
    std::vector<uint8_t> badH;
    std::vector<int32_t> begH, cntH, capH;
    std::vector<int64_t> mapChunks;   /* work items of one frame plane against all planes of map s */
    int maps = 0;
    /* one batch: the packed inputs / index outputs (io), the pair arrays, the work list, the accumulators, the flags */
    DevBuf<char> io;
    PinnedBuf<char> hio;
    DevBuf<float> angle;
    DevBuf<uint32_t> key;
    DevBuf<int4> work;
    DevBuf<int32_t> acc;                          /* counter [4], nmatches [frames], npairs [frames] */
    DevBuf<uint8_t> flags;
    hipEvent_t staged = nullptr, done = nullptr;
    int frames = 0, planes = 0, flagged = 0;
    std::vector<int32_t> frameOff, frameMap;
    size_t offMap = 0, offPar = 0, offVer = 0;   /* byte offsets of the three index outputs in io */
    /* map upkeep (map_plane.cpp): frame clouds of a call, one round's staging, gather input and voxel-grid scratch */
    DevBuf<float> upSrc, upPose, upIn, upOut;
    DevBuf<char> upRec;
    PinnedBuf<char> upHost;
    DevBuf<unsigned long long> upRecs, upTmp;
    DevBuf<uint32_t> upPosL, upPosR;
    DevBuf<int> upList, upCounts;
    DevBuf<int4> upMove;
    int64_t upStats[4] = {0, 0, 0, 0};   /* voxel jobs on the device, jobs redone on the host, rounds, arena repacks */
    /* plane culling (plane_cull.cpp): pair angles and keys (column-major triangle), the gated rows of every column */
    DevBuf<float> pcAngle;
    DevBuf<uint32_t> pcKey;
    DevBuf<int32_t> pcRowList, pcRowCount;
    int64_t cullStats[4] = {0, 0, 0, 0}; /* calls, device calls, distance launches, rebuild calls */
};

/* Map upkeep launches (map_plane_kernels.hip).  A segment is one piece of a voxel job's input: `n` points written to
 * in[dst, dst + n), read from src[src ..] and moved into world by pose `pose` (MP_SEG_FRAME: the frame form's Tcw,
 * MP_SEG_KEYFRAME: the observation form's Twc), or copied from the arena (MP_SEG_RESIDENT). */
enum { MP_SEG_FRAME = 0, MP_SEG_KEYFRAME = 1, MP_SEG_RESIDENT = 2 };
struct MpSeg { int32_t form, pose, src, n, dst, pad[3]; };
/* a round's job: voxel counts[k] centroids of in / out offset inOff go to arena[dstBeg ..] of plane `plane` (cap = its slot) */
struct MpCommit { int32_t plane, inOff, dstBeg, cap; };
hipError_t drfe_launch_map_plane_gather(const MpSeg* segs, int nseg, int maxN, const float* poses, const float* src,
                                        const float* arena, float* in, hipStream_t s);
hipError_t drfe_launch_map_plane_commit(const MpCommit* jobs, int njobs, int maxN, const int* counts, const float* out, float* arena,
                                        int32_t* cloudEnd, hipStream_t s);
/* moves[k] = (old begin, new begin, points) of plane k */
hipError_t drfe_launch_map_plane_move(const int4* moves, int nplanes, int maxN, const float* from, float* to, hipStream_t s);

/* one voxel job of an update or rebuild call: segments [seg0, seg1) of the call's list, then (resident) the plane's cloud */
struct MpJob { int plane, seg0, seg1; bool resident; };
/* the rounds of map_plane.cpp over a call's jobs (global plane indices): gather, voxel grid, commit, hand-back, repack */
int drfe_pm_run_jobs(drfe_ctx* c, PmBuffers* b, const std::vector<MpJob>& jobs, const std::vector<MpSeg>& segs, const float* poses,
                     int nposes, const float* src, size_t nsrc, hipStream_t s);
/* replaces the cloud of global plane g with n host points (a repack when the slot is too small) */
int drfe_pm_set_cloud(drfe_ctx* c, PmBuffers* b, int g, const float* xyz, int n, hipStream_t s);

/* Plane culling launches (plane_cull_kernels.hip) over the P planes of one map, global planes [pb, pb + P) */
#define PC_THREADS 256
#define PC_POINTS_PER_LANE 4
#define PC_CHUNK (PC_THREADS * PC_POINTS_PER_LANE)   /* cloud points of one work item of the distance pass */
#define PC_ROW_TILE 16                               /* gated rows one work item scans its points against */
struct PcLaunch {
    const float *mapCoefs, *cloud;
    const uint8_t* mapBad;
    const int32_t *cloudBeg, *cloudEnd;
    float* angle;
    uint32_t* key;
    int32_t *rowList, *rowCount;
    int pb, P, tile;
    double aTh;
};
/* angle, key reset and the gated rows of every column; rowCount must be zero */
hipError_t drfe_launch_plane_cull_pairs(const PcLaunch& L, hipStream_t s);
/* the distance pass over columns [col0, col0 + ncols): maxChunks / maxRows bound the chunks of a cloud and the rows of a column */
hipError_t drfe_launch_plane_cull_dist(const PcLaunch& L, int col0, int ncols, int maxChunks, int maxRows, hipStream_t s);

/* per-plane arrays and work-list sizes from the host mirrors (after an upload, an edit or an update) */
int drfe_pm_push_planes(drfe_ctx* c, PmBuffers* b);
/* the match batch's work-list sizes (mapChunks) from the host's cloud sizes */
void drfe_pm_chunks(PmBuffers* b);

#endif
