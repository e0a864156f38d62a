/* drfe_debug.h - test hooks of libdrfe.so: entry points that exist so that tests can hold an internal routine (the correctly
 * rounded sin / cos, the restated introsort, the device sort, the vectorised AHC trial solver) to its reference.  Not part of the
 * drop-in boundary (include/drfe.h): a DR-SLAM build never includes this file. */
#ifndef DRFE_DEBUG_H
#define DRFE_DEBUG_H
#include "drfe.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test hook of dr_slam_amd/csrc/cr_sincos.h: correctly rounded sin / cos of n doubles in [0, 64) (host build of the routine the
 * device path uses for region2rect's direction and region_grow's seed direction); ok[i] = 0 where the rounding could not be
 * certified.  Host code. */
int drfe_debug_cr_sincos(const double* x, int n, double* s, double* c, int32_t* ok);

/* Test hook of dr_slam_amd/csrc/lsd_order_kernels.hip: n LSD ordering keys (gradient bin << 22 | y << 11 | x) sorted in place on the
 * device into std::sort's order under lsd.cpp's compare_norm (larger bins first, the order of equal bins = libstdc++'s
 * introsort's, heap-sort branch included).  *status: 0, or 1 if a range above 1024 keys exhausted introsort's depth limit (one
 * lane heap-sorts shorter ones; the caller orders such a frame on the host).  _depth: depth_limit >= 0 replaces 2 lg n, so that
 * tests reach the heap-sort branch (compare with drfe_debug_order_sort, mode 3, same depth_limit). */
int drfe_debug_device_order_sort(drfe_ctx* ctx, uint32_t* keys, size_t n, int* status);
int drfe_debug_device_order_sort_depth(drfe_ctx* ctx, uint32_t* keys, size_t n, int depth_limit, int* status);

/* Test hook of the vectorised trial-merge solver of the AHC clustering (dr_slam_amd/csrc/ahc_math_simd.h): plane fits of n (nine
 * sums, N) records by the scalar routine (mode 0), its 8-lane AVX2 (1) or 8-lane AVX-512F (2) instantiation; out8 = center,
 * normal, mse, curvature per record.  DRFE_ERR_STATE if this CPU lacks the mode.  Host code. */
int drfe_debug_ahc_trials(const double* sums9, const int32_t* N, int n, int mode, double* out8);

/* Test hook of dr_slam_amd/csrc/introsort_restated.h, the two std::sort calls whose permutation of equal keys reaches the output:
 * kind 0 = LSD's pseudo-ordering (uint32 keys: gradient bin << 22 | y << 11 | x, larger bins first: lsd.cpp compare_norm), kind 1 =
 * pcl::VoxelGrid's index sort (uint64 records: leaf << 32 | point, smaller leaves first).  recs[n] sorted in place.  mode 0:
 * std::sort with the reference's comparator; 1 / 2: the product's restatement with scalar / AVX2 stopper masks; 3: the plain
 * transcription of libstdc++'s introsort.  depth_limit >= 0 replaces the 2 lg n of modes 1-3 (reaches the heap-sort branch).
 * skip_below > 0 (kind 0, modes 1 / 2): only the keys whose bin is >= skip_below are wanted - they form a prefix of the result
 * and come out in std::sort's order, the rest follows unsorted within its bins' ranges (what the product asks for: pixels
 * without a level-line angle never seed a region).  DRFE_ERR_STATE if this CPU lacks AVX2 (mode 2).  Host code. */
int drfe_debug_order_sort(void* recs, size_t n, int kind, int mode, int depth_limit, uint32_t skip_below);
/* The same records through mode 3 (the plain transcription; depth_limit as above), which also reports in *longest the longest range
 * that ran out of depth and reached std::__partial_sort, 0 if none did.  The device sorts partition identically and leave ranges
 * above 1024 records (introsort_device.h: ORD_HEAP_MAX) to the host: they hand an input back if and only if *longest > 1024.
 * Host code. */
int drfe_debug_order_sort_heap_max(void* recs, size_t n, int kind, int depth_limit, size_t* longest);

/* Test hook of voxel_kernels.hip (the uint64 / 256-thread instantiation of introsort_device.h): n_clouds hand-built clouds in CSR
 * form (cloud i = points [offsets[i], offsets[i + 1]) of xyz, n_clouds <= 256) through one device voxel-grid lane, k_voxel_jobs_order
 * + k_voxel_grid, the code path of the batch post-processing.  out_xyz (as large as xyz): cloud i's centroids from offsets[i] on;
 * out_counts[i]: the kernel's raw count - their number, or -1 (the grid exceeds int32: PCL keeps the input), -2 (a range above 1024
 * records reached the heap-sort branch: the caller's host path), <= -9 (a loop bound of the sort: never).  out_recs (optional, as
 * many as points): cloud i's sorted leaf << 32 | point records.  depth_limit >= 0 replaces introsort's 2 lg n (compare with
 * drfe_debug_order_sort, kind 1, mode 3), -1 is the natural limit.  workgroups > 0 caps the launch's grid, so that one workgroup
 * takes job after job; 0 is the product's resident count. */
int drfe_debug_device_voxel_grid(drfe_ctx* ctx, const float* xyz, const int32_t* offsets, int n_clouds, float leaf, int depth_limit, int workgroups,
                                 float* out_xyz, int32_t* out_counts, uint64_t* out_recs);

/* Test hook of the gates and the RANSAC refit behind the voxel grids (Frame::MaxPointDistanceFromPlane): n_planes hand-built
 * extractor planes, each with a hand-built voxel cloud (plane i = points [coarse_offsets[i], coarse_offsets[i + 1]) of coarse_xyz).
 * on_device = 1: refit_kernels.hip's k_plane_refit over n_planes + 1 jobs of one fabricated frame (the last job is past the
 * frame's planes); status[n_planes + 1] is the kernel's raw status: 0 post[i] is final, 1 not certified (the product refits on the
 * host), 2 the plane's voxel grid came back, -1 no such plane; post[i] is written where status is 0 or 2.  vcounts_override
 * (optional, n_planes): the voxel count the kernel is told, a negative one marks the grid as handed back.  on_device = 0:
 * planes_post.cpp's host loop on the same data, status 0 (-1 for the last).  ctx may be NULL then. */
int drfe_debug_plane_refit(drfe_ctx* ctx, int on_device, const drfe_plane* planes, int n_planes, const float* coarse_xyz, const int32_t* coarse_offsets,
                           const int32_t* vcounts_override, float max_point_dist, double dist_threshold, drfe_plane_post* post, int32_t* status);

/* Test hook of include/drfe_math.h's canonical libm of the Manhattan-frame tracker: out[i] = drfe_asin(x[i]) (which 0),
 * drfe_exp(x[i]) (which 1) or drfe_tanf((float)x[i]) widened to double (which 2).  Host code. */
int drfe_debug_manhattan_math(int which, const double* x, int n, double* out);

/* Test hook of include/drfe_math.h's canonical libm of triangulation: out[i] = drfe_atan2f(y[i], x[i]) (which 0),
 * drfe_cosf(y[i]) (which 1) or the stereo parallax drfe_cosf(2 * drfe_atan2f(y[i] / 2, x[i])) (which 2).  Host code. */
int drfe_debug_triangulate_math(int which, const float* y, const float* x, int n, float* out);
/* The same three expressions on the device, one lane per element, by a kernel of dr_slam_amd/csrc/triangulate_kernels.hip (so
 * under the flags the triangulation kernel is compiled with): same bits as the host hook. */
int drfe_debug_triangulate_math_device(drfe_ctx* ctx, int which, const float* y, const float* x, int n, float* out);

/* Test hooks of the Sim3 solver.  _atan2: out[i] = dr_slam_amd/csrc/cr_atan2.h's correctly rounded atan2(y[i], x[i]), y >= 0;
 * ok[i] = 0 where it was not certified.  _rand: the first n values of rand() after srand(seed), from
 * dr_slam_amd/csrc/glibc_rand.h.  Host code. */
int drfe_debug_sim3_atan2(const double* y, const double* x, int n, double* out, int32_t* ok);
int drfe_debug_sim3_rand(uint32_t seed, int n, int32_t* out);
/* _horn: sim3_core.h's ComputeSim3 on n samples (P1, P2: 3x3 row-major, one point per column), out = 37 floats per sample (R12 9,
 * t12 3, s12, T12 12, T21 12); libm != 0 takes atan2, sin and cos from the host's libm, the way a hypothesis that was not
 * certified is finished; ok[i] = 0 where the core refused.  Host code.
 * _hand_back: every > 0 makes drfe_sim3_ransac_batch treat every `every`-th hypothesis of a call as not certified by the device,
 * so that the host finishes it (0 = off): the table must not change. */
int drfe_debug_sim3_horn(const float* P1, const float* P2, int n, int fix_scale, int libm, float* out, int32_t* ok);
int drfe_debug_sim3_hand_back(drfe_ctx* ctx, int every);
/* Test hooks of the PnP solver (test-only, like everything in this header: no integration calls them).
 * pnp_core.h's double Jacobi SVD of a row-major m x n matrix (n <= m <= 12) on the host: w [n], the left singular vectors as
 * rows ut [n x m], the right ones as rows vt [n x n].  For tests. */
int drfe_debug_pnp_svd(const double* A, int m, int n, double* w, double* ut, double* vt);
/* pnp_core.h's CheckInliers under the pose R [9], t [3] (double) and K = fx, fy, cx, cy over n correspondences: out[i] = 1 for an
 * inlier.  Host code. */
int drfe_debug_pnp_inliers(const double* R, const double* t, const float* K, const float* p2d, const float* Xw, const float* max_err,
                           int n, uint8_t* out);
/* The same through the device's inlier sweep (pnp_kernels.hip's pnp_sweep, one wavefront; n <= DRFE_PNP_MAX_CORR): same bytes. */
int drfe_debug_pnp_inliers_device(drfe_ctx* ctx, const double* R, const double* t, const float* K, const float* p2d, const float* Xw,
                                  const float* max_err, int n, uint8_t* out);
/* Test hooks of the Initializer (dr_slam_amd/csrc/init_core.h).
 * _cos_keys: key[i] = the unsigned key the accepted cosine c[i] is ordered by (-0 as +0, a NaN 0xFFFFFFFF, above every number),
 * value[i] = the cosine that key stands for.  Host code.
 * _null_vectors: for n samples of eight normalised matches (x1 y1 x2 y2 each, 32 floats a sample), h = vt.row(8) of ComputeH21's
 * 16x9 system and fpre = vt.row(8) of ComputeF21's 8x9 system, 9 floats each, as the float Jacobi SVD leaves them.  Host code.
 * _check_rt: CheckRT of one motion hypothesis R [9], t [3] under K [9] and sigma over n <= DRFE_INIT_MAX_KEYS matches (u1 v1 u2 v2
 * each), every one an inlier, match i's reference key being i: nGood, the selected cosine, the parallax, the DRFE_INIT_MOTION_*
 * status, vbGood [n] and vP3D [3 n].  ctx == NULL: the host entry's routine; otherwise the device's CheckRT kernel.  This is how
 * tests reach a point triangulated onto the first camera's centre, whose cosine is 0 / 0. */
int drfe_debug_init_cos_keys(const float* c, int n, uint32_t* key, float* value);
int drfe_debug_init_null_vectors(const float* points, int n, float* h, float* fpre);
int drfe_debug_init_check_rt(drfe_ctx* ctx, const float* K, const float* R, const float* t, float sigma, const float* matches, int n,
                             int32_t* good, float* cos_selected, float* parallax, int32_t* status, uint8_t* vbGood, float* vP3D);
/* Test hooks of PoseOptimization (dr_slam_amd/csrc/pose_opt_core.h, cr_cube.h).  Host code.
 * _cr_cube: out[i] = the correctly rounded x[i]^3 and ok[i] = 1, or ok[i] = 0 where cr_cube.h cannot certify the rounding.
 * _pose_opt_ldlt: pose_opt_core.h's Eigen::LDLT of the symmetric 6x6 A (row-major, the lower triangle is read) and its solve of
 * A x = b: returns isPositive() in *positive; x is written only then.
 * _plane_error: computeError of one plane edge (kind 3 EdgePlaneOnlyPose, 4 EdgeParallelPlaneOnlyPose, 5 EdgeVerticalPlaneOnlyPose)
 * with the measured and the world plane as float[4] coefficients under the pose Tcw: e[3] (e[2] = 0 for kinds 4 and 5).
 * _hand_back: every > 0 makes drfe_pose_opt_batch treat every `every`-th frame of a call as not certified by the device, so that
 * the host core runs it again; 0 turns it off. */
int drfe_debug_cr_cube(const double* x, int n, double* out, uint8_t* ok);
int drfe_debug_pose_opt_ldlt(const double* A, const double* b, double* x, int32_t* positive);
int drfe_debug_pose_opt_plane_error(int kind, const float* meas, const float* world, const float* Tcw, double* e);
int drfe_debug_pose_opt_hand_back(drfe_ctx* ctx, int every);
/* Test hooks of TranslationOptimization (dr_slam_amd/csrc/trans_opt_core.h).  Host code.
 * _plane_error: computeError of one translation-only plane edge (kind 3 EdgePlaneOnlyTranslation, 4
 * EdgeParallelPlaneOnlyTranslation, 5 EdgeVerticalPlaneOnlyTranslation): the world plane's normal rotated by the float R_cw of
 * Tcw, localPlane = w2n + Xc under Tcw's translation, then ominus / ominus_par / ominus_ver: e[3] (e[2] = 0 for kinds 4 and 5).
 * _hand_back: every > 0 makes drfe_trans_opt_batch treat every `every`-th frame of a call as handed back by the device, so that
 * the host core runs it again; 0 turns it off. */
int drfe_debug_trans_opt_plane_error(int kind, const float* meas, const float* world, const float* Tcw, double* e);
int drfe_debug_trans_opt_hand_back(drfe_ctx* ctx, int every);
/* Test hooks of OptimizeSim3 (dr_slam_amd/csrc/sim3_opt_core.h).  Host code.
 * _sim3_opt_ldlt: the 7x7 form of lm_core.h's Eigen::LDLT (A row-major, the lower triangle is read) and its solve of A x = b;
 *   *positive = isPositive(), x is written only then.
 * _sim3_opt_step: the core's update (so_lm_update: VertexSim3Expmap::oplusImpl of xbl[0..6] on S12, eight doubles) into S12_out, and
 *   the core's computeScale (lm_scale, what lm_judge divides by) over x = xbl[0..6], b = xbl[7..13], lambda = xbl[14], read
 *   after the update as lm_step / lm_judge and g2o do, or with read_before before oplusImpl wrote x[6] = 0 for a fixed scale.
 * _hand_back: every > 0 makes drfe_sim3_opt_batch treat every `every`-th problem of a call as not certified by the device, so that
 *   the host core finishes it; 0 switches the hook off. */
int drfe_debug_sim3_opt_ldlt(const double* A, const double* b, double* x, int32_t* positive);
int drfe_debug_sim3_opt_step(const double* S12, const double* xbl, int fix_scale, int read_before, double* S12_out, double* scale);
int drfe_debug_sim3_opt_hand_back(drfe_ctx* ctx, int every);

#ifdef __cplusplus
}
#endif
#endif /* DRFE_DEBUG_H */
