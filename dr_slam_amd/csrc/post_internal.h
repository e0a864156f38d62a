/* post_internal.h — records shared by normals_kernels.hip and planes_post.cpp (Frame::ComputePlanes post-processing) */
#ifndef DRFE_POST_INTERNAL_H
#define DRFE_POST_INTERNAL_H
#include "drfe_internal.h"

/* the 3x-subsampled organized cloud of src/Frame.cc:1027-1048: ceil(rows/3.0) x ceil(cols/3.0) */
static inline int drfe_sn_w(int w) { return (w + 2) / 3; }
static inline int drfe_sn_h(int h) { return (h + 2) / 3; }

struct SnBuffers {            /* device scratch of the surface-normal pass, [frame][...] */
    DevBuf<float> d_cloud;    /* W*H x 3 */
    DevBuf<float> d_dist;     /* W*H: depth-change seeds, then the chamfer distance */
    DevBuf<double> d_integ;   /* (W+1)*(H+1) x 6 */
    DevBuf<unsigned> d_cnt;   /* (W+1)*(H+1) x 2 */
    DevBuf<float> d_normals;  /* W*H x 3 */
    DevBuf<drfe_surface_normal> d_recs;   /* (W/2)*(H/2) */
    DevBuf<float> d_depth;    /* staging of the host-buffer entry point */
    size_t frames = 0, w = 0, h = 0;      /* capacity */
    int lastFrames = 0;       /* frames of the most recent drfe_surface_normals_batch (drfe_manhattan_track_batch reads them) */
};

hipError_t drfe_launch_surface_normals(const void* d_depth, int isU16, float factor, size_t frameStride, size_t rowStride, int w,
                                       int h, const float K4[4], float maxDist, int nframes, const SnBuffers& b, hipStream_t s);
void drfe_post_free(drfe_ctx* c);
/* Manhattan-frame tracking of nseq sequences of seq_len frames (manhattan_kernels.hip; one workgroup per sequence): records
 * of frame f at d_recs + f * nrec, lines of frame f at d_dirs[d_loff[f] .. d_loff[f + 1]).  d_cone / d_sums: per sequence
 * `scratch` bytes / 3 x `scratch` doubles, scratch >= nrec + the largest line count of a frame. */
hipError_t drfe_launch_manhattan(const drfe_surface_normal* d_recs, int nrec, const float* d_R0, int nseq, int seq_len,
                                 const double* d_dirs, const int32_t* d_loff, int n_calls, uint8_t* d_cone, double* d_sums,
                                 size_t scratch, float* d_R, drfe_manhattan_info* d_info, uint16_t* d_rbits, uint16_t* d_lbits,
                                 hipStream_t s);
void drfe_manhattan_free(drfe_ctx* c);
/* Plane association of a batch of frames against device-resident maps (plane_match_kernels.hip, driven by plane_match.cpp).
 * Frame plane q (of Q) belongs to frame qFrame[q] and map qMap[q]; its pairs with the map's planes are angle / key
 * [qPair[q], qPair[q] + planes of the map).  Map s owns planes [planeOff[s], planeOff[s + 1]) and points
 * [pointOff[s], pointOff[s + 1]).  workCap bounds the chunks of the gated clouds (the host's exact cloud sizes).  Expects key memset to 0xFF, counter / nmatches / npairs to 0 and (flagPoints) flags to 0. */
#define PM_CHUNK 2048             /* cloud points per work item of the distance pass (256 lanes x 8) */
#define PM_FLAG_POINTS 2048       /* map points per workgroup of the flag sweep */
struct PmLaunch {
    const float *Tcw, *coefs;
    const int32_t *qFrame, *qMap, *qPair, *planeOff, *pointOff;
    int32_t *mapOut, *parOut, *verOut;
    const float* mapCoefs;
    const uint8_t* mapBad;
    const int32_t *cloudBeg, *cloudEnd;     /* map plane j's cloud: cloud points [cloudBeg[j], cloudEnd[j]) */
    const float *cloud, *points;
    float* angle;
    uint32_t* key;
    int4* work;
    int workCap;
    uint32_t* counter;
    int32_t *nmatches, *npairs;
    uint8_t* flags;
    int Q, maxPts;
    drfe_plane_match_params params;
    bool flagPoints;
};
hipError_t drfe_launch_plane_match(const PmLaunch& L, hipStream_t s);
void drfe_plane_match_free(drfe_ctx* c);
#include <string>
/* pcl::VoxelGrid for njobs point clouds at once (voxel_kernels.hip): job j = points [jobs[j].x, jobs[j].x + jobs[j].y) of d_pts
 * (xyz packed); d_list: njobs + 2 ints of scratch (the job order); scratch arrays span all points; centroids of job j to d_out at the job's offset, their number to d_counts[j]
 * (-1: grid overflows int32, PCL keeps the input cloud; -2: the sort needs the heap-sort branch: run the job on the host; <= -9: a loop
 * bound of the sort).  d_recs holds job j's sorted leaf << 32 | point records at the job's offset afterwards.  Tests only:
 * depthLimit >= 0 replaces introsort's 2 lg n, workgroups > 0 caps the launch's grid below the resident count. */
hipError_t drfe_launch_voxel_grid(const float* d_pts, const int2* d_jobs, int njobs, int* d_list, unsigned long long* d_recs, unsigned long long* d_tmp,
                                  uint32_t* d_posL, uint32_t* d_posR, float* d_out, int* d_counts, float leafSize, hipStream_t s, int depthLimit = -1,
                                  int workgroups = 0);
/* Gates + Frame::MaxPointDistanceFromPlane (RANSAC + least-squares refit) of njobs planes on the centroids k_voxel_grid left
 * (refit_kernels.hip): job j = plane j % planeCap of frame j / planeCap of the extractor's frame table; d_post[j] / d_status[j]
 * (0 final, 1 not certified: refit on the host, 2 the voxel grid came back: grid + refit on the host, -1 no such plane).
 * d_mtState: std::mt19937(12345)'s 624 state words after seeding; logP = log(1 - 0.99) by the host's libm. */
struct AhcDevFrame;
hipError_t drfe_launch_plane_refit(const AhcDevFrame* d_frames, const int2* d_jobs, const int* d_vcounts, const float* d_vout, const uint32_t* d_mtState,
                                   int njobs, int planeCap, float maxPointDist, double distThreshold, double logP, drfe_plane_post* d_post, int* d_status,
                                   hipStream_t s);
/* a lane's device voxel grid (planes_post.cpp): buffers + stream; NULL = the host voxel grid */
struct VoxelDevice;
VoxelDevice* drfe_voxel_device_create(int device, std::string* err);
void drfe_voxel_device_free(VoxelDevice* v);
int drfe_ahc_post_core(std::string* err, const uint16_t* depth, int w, int h, size_t stride, const float* K4, float depth_factor,
                       const drfe_plane* planes, int n_planes, const int32_t* member_offsets, const int32_t* member_idx,
                       float max_point_dist, double dist_threshold, drfe_plane_post* post, float* voxel_xyz, int32_t* voxel_offsets,
                       int cap_voxels, int* n_accepted, int* plane_num, VoxelDevice* vox = nullptr);
int drfe_ahc_post_from_coarse(std::string* err, const drfe_plane* planes, int n_planes, const float* const* coarse_xyz, const int* coarse_n,
                              float max_point_dist, double dist_threshold, drfe_plane_post* post, float* voxel_xyz, int32_t* voxel_offsets,
                              int cap_voxels, int* n_accepted, int* plane_num);
#endif
