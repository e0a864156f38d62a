/* drfe.h — C-ABI of the MI355X-native DR-SLAM feature front-end (libdrfe.so).
 *
 * The reference (WangWen-Believer/DR-SLAM) has no FFI: its per-frame feature path is reached through
 * C++ classes.  Each entry point below names the reference interface it replaces; INTEGRATION.md
 * shows the adaptor a maintainer would drop into DR-SLAM (`ORBextractor::operator()` etc. calling
 * these functions).  Plain C: opaque context, caller-owned buffers with capacities, int status
 * (0 = ok, <0 = drfe_status), no exceptions and no OpenCV/torch types cross this boundary.
 *
 * Threading: a drfe_ctx is bound to one HIP device and is NOT re-entrant (like the reference's
 * ORBextractor instance, include/ORBextractor.h:85 public pyramid member); use one context per calling
 * thread (Tracking / LocalMapping / LoopClosing).
 *
 * Pointers named d_* are device (HBM) pointers; all others are host pointers.
 */
#ifndef DRFE_H
#define DRFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum drfe_status {
    DRFE_OK = 0,
    DRFE_ERR_INVALID = -1,    /* bad argument (null pointer, size mismatch, unsupported geometry) */
    DRFE_ERR_HIP = -2,        /* HIP runtime failure; see drfe_last_error */
    DRFE_ERR_CAPACITY = -3,   /* caller buffer or internal pool too small; nothing partial is returned */
    DRFE_ERR_STATE = -4       /* call order violated (e.g. match before extract) */
} drfe_status;

/* cv::KeyPoint binary layout (7 x 4 bytes) so an adaptor can memcpy into std::vector<cv::KeyPoint>. */
typedef struct drfe_keypoint {
    float x, y;       /* pt, level-0 pixel units (already multiplied by the level scale) */
    float size;       /* 31 * scale[octave] truncated to int, src/ORBextractor.cc:837,846 */
    float angle;      /* degrees [0,360), IC_Angle */
    float response;   /* FAST score */
    int32_t octave;
    int32_t class_id; /* -1 */
} drfe_keypoint;

/* ORBextractor constructor arguments (include/ORBextractor.h:56-57; yaml keys ORBextractor.*,
 * src/Tracking.cc:120-126) plus the capacities the device buffers are sized for. */
typedef struct drfe_config {
    int32_t device;        /* HIP device ordinal */
    int32_t max_width;     /* largest frame the context will see (e.g. 640) */
    int32_t max_height;    /* (e.g. 480) */
    int32_t max_batch;     /* frames processed per batched call (>=1) */
    int32_t nfeatures;     /* 1000 */
    float scale_factor;    /* 1.2f */
    int32_t nlevels;       /* 8 */
    int32_t ini_th_fast;   /* 20 */
    int32_t min_th_fast;   /* 7 */
} drfe_config;

typedef struct drfe_ctx drfe_ctx;

/* Camera / Frame constants the glue and matchers read (Frame::Frame, src/Frame.cc:104-196). */
typedef struct drfe_camera {
    float fx, fy, cx, cy;
    float bf;            /* Camera.bf */
    float depth_factor;  /* 1/DepthMapFactor: metres per raw depth unit (src/Tracking.cc:144-148) */
    float min_x, max_x, min_y, max_y; /* mnMinX.. (image bounds when k1 == 0, src/Frame.cc:884-889) */
} drfe_camera;

/* ------------------------------------------------------------------------------------------------ */
/* lifetime                                                                                          */
int drfe_create(const drfe_config* cfg, drfe_ctx** out);
void drfe_destroy(drfe_ctx* ctx);
const char* drfe_last_error(const drfe_ctx* ctx); /* ctx may be NULL: last create() failure */
const char* drfe_version(void);

/* ------------------------------------------------------------------------------------------------ */
/* ORBextractor (replaces src/ORBextractor.cc)                                                       */

/* Getters of include/ORBextractor.h:63-83: arrays of nlevels floats. */
int drfe_orb_scale_tables(const drfe_ctx* ctx, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2);
/* Capacity a caller needs for keypoint/descriptor buffers of one frame (>= any N the path can emit). */
int drfe_orb_max_keypoints(const drfe_ctx* ctx);

/* ORBextractor::operator()(image, mask, keypoints, descriptors), src/ORBextractor.cc:1043-1105.
 * gray: CV_8UC1 host image with row stride `stride` bytes.  Writes N keypoints and N x 32 descriptor
 * bytes (level-major order exactly as the reference concatenates them).  Empty image (w==0||h==0 or
 * gray NULL) -> *n_out = 0, DRFE_OK (reference returns silently, :1046-1047). */
int drfe_orb_extract(drfe_ctx* ctx, const uint8_t* gray, int w, int h, size_t stride, drfe_keypoint* kps,
                     uint8_t* desc, int cap, int* n_out);

/* Batched, device-resident form: nframes (<= max_batch) CV_8UC1 frames already in HBM, frame f at
 * d_gray + f*frame_stride, rows `row_stride` bytes apart.  Asynchronous on `stream` (a hipStream_t;
 * NULL = the context's own stream).  Results stay in the context's frame slots 0..nframes-1.
 * Several contexts working at once (batches in flight): pass NULL - the stream every drfe_create makes sits on its own
 * hardware queue, so the contexts' kernels really overlap (+10 % device rate at three batches in flight); streams from a
 * framework's pool may share a queue, and the batches then run one behind the other.
 * The frames are read until the call's last extraction kernel (orientation + descriptors) has finished, not only at its start:
 * where d_gray, frame_stride and row_stride are multiples of 16 and the frame size allows it (w a multiple of 16; 640x480 and
 * 1280x960 do), pyramid level 0 is not copied into the context but read from the frames in place.  Do not overwrite or free them
 * before the stream has passed the call. */
int drfe_orb_extract_batch(drfe_ctx* ctx, const uint8_t* d_gray, size_t frame_stride, size_t row_stride, int w,
                           int h, int nframes, void* stream);
/* 0: drfe_orb_extract_batch always copies level 0 into the context (the frames are then read at the start of the call only);
 * 1 (default): it reads level 0 in place where it can.  Results are identical.  DRFE_LEVEL0_COPY=1 in the environment sets 0 at
 * drfe_create. */
int drfe_orb_configure_level0(drfe_ctx* ctx, int in_place);
/* 1 if the most recent drfe_orb_extract_batch on ctx read level 0 in place, 0 if it copied it. */
int drfe_orb_level0_in_place(const drfe_ctx* ctx);
/* How drfe_orb_extract_batch runs DistributeOctTree for frames of width x height in a batch of nframes: per level the
 * workgroup size, the candidate keys a thread keeps in registers, the node-list capacity, the level's node capacity
 * (quota + 4) and the index of its launch, as out[nlevels][5].  A pure function of its arguments: needs no device, reads only
 * cfg's nfeatures, scale_factor and nlevels.  force: NULL, or the text DRFE_QT_FORCE would hold in the environment at
 * drfe_create ("<threads>,<kpt>" for every level it is legal for, or one pair per level separated by ';').  Returns the number
 * of launches, or a DRFE_ERR_* code. */
int drfe_orb_quadtree_plan(const drfe_config* cfg, int width, int height, int nframes, const char* force, int32_t* out);
/* Copy slot results to host (synchronises the batch stream). */
int drfe_orb_download(drfe_ctx* ctx, int slot, drfe_keypoint* kps, uint8_t* desc, int cap, int* n_out);
/* The whole batch to host memory in five copies, asynchronous on `stream` (hipStream_t; NULL = the context stream): for a
 * pipeline that overlaps the results of batch i with the kernels of batch i+1 (pinned host buffers).  kps
 * [nframes][max_keypoints], desc [nframes][max_keypoints][32], kp_counts [nframes]; matches [nframes][max_keypoints] and
 * match_counts [nframes] (both may be NULL) as drfe_match_download returns them.  Rows past a frame's count are
 * unspecified.  The caller synchronises the stream before reading. */
int drfe_batch_download_async(drfe_ctx* ctx, int nframes, drfe_keypoint* kps, uint8_t* desc, int32_t* kp_counts,
                              int32_t* matches, int32_t* match_counts, void* stream);
/* The device status words of the batch most recently extracted / matched on ctx, copied asynchronously on `stream` (NULL: the
 * context's): status[0] = extraction (bit 0: FAST candidate arena overflow, bit 1: quadtree node pool overflow), status[1] =
 * drfe_match_consecutive_batch (bit 2: more than 256 keypoints in one search window).  Non-zero = keypoints / matches of that
 * batch are truncated.  The batch matcher's word is its own: no other search clears it. */
int drfe_batch_status_async(drfe_ctx* ctx, int32_t* status, void* stream);
/* The same check, blocking (waits for the context's stream): DRFE_ERR_CAPACITY with the reason in drfe_last_error if an arena
 * overflowed.  drfe_pipeline_sync calls it for every context it waits for. */
int drfe_batch_check(drfe_ctx* ctx);
/* Per-slot keypoint counts (host array of nframes ints; synchronises). */
int drfe_orb_counts(drfe_ctx* ctx, int nframes, int* counts);

/* mvImagePyramid parity (public member, include/ORBextractor.h:85): copy the bordered level
 * ((w_l+38) x (h_l+38), tightly packed) of a slot to host.  out may be NULL to query sizes.
 * Level 0 of a slot whose batch read it in place (drfe_orb_level0_in_place) is bordered by this call, from the frame that was
 * passed to drfe_orb_extract_batch: that frame must still be alive and unchanged. */
int drfe_orb_pyramid_level(drfe_ctx* ctx, int slot, int level, uint8_t* out, int* bordered_w, int* bordered_h);
/* Debug/parity taps (tests): blurred interior level, FAST candidates (x,y,response relative to the
 * 16-px detection border, unordered). */
int drfe_orb_blurred_level(drfe_ctx* ctx, int slot, int level, uint8_t* out, int* w, int* h);
int drfe_orb_candidates(drfe_ctx* ctx, int slot, int level, int32_t* xyr, int cap, int* n_out);

/* ------------------------------------------------------------------------------------------------ */
/* Frame glue (replaces Frame::ComputeStereoFromRGBD + AssignFeaturesToGrid, src/Frame.cc:224-237,
 * 893-911; no-distortion path of UndistortKeyPoints :836-838).                                      */

/* d_depth: raw CV_16U depth frames in HBM (same indexing as d_gray).  For every slot computes
 * mvDepth/mvuRight and the 64x48 feature grid, all kept on device for the matchers. */
int drfe_frame_stereo_grid_batch(drfe_ctx* ctx, const uint16_t* d_depth, size_t frame_stride_elems,
                                 size_t row_stride_elems, const drfe_camera* cam, int nframes, void* stream);
/* Sparse-depth form of the glue for a pipeline fed from HOST memory: ComputeStereoFromRGBD reads the depth image at <= max_keypoints
 * pixels per frame, so a host that keeps its depth images can ship one raw value per keypoint (2 KB per frame) instead of the
 * frame (614 KB).  Three steps after drfe_orb_extract_batch:
 *   drfe_orb_keypoint_pixels_async   the pixel of every keypoint (u | v << 16, truncated as the reference truncates kp.pt;
 *                                    0xFFFFFFFF = outside the image) and the per-frame counts, D2H on `stream`
 *   drfe_gather_keypoint_depth       HOST code: out[f][i] = depth_f(v, u) on n_threads threads (<= 0: the CPUs this process may use)
 *   drfe_frame_stereo_grid_batch_kpdepth   the glue from those values ([nframes][max_keypoints], host or device memory)
 * Results are identical to drfe_frame_stereo_grid_batch on the same depth images (tests/test_gpu_match.py). */
int drfe_orb_keypoint_pixels_async(drfe_ctx* ctx, int nframes, uint32_t* uv, int32_t* counts, void* stream);
int drfe_gather_keypoint_depth(const uint16_t* depth, size_t frame_stride_elems, size_t row_stride_elems, int nframes,
                               const uint32_t* uv, const int32_t* counts, int max_keypoints, uint16_t* out, int n_threads);
int drfe_frame_stereo_grid_batch_kpdepth(drfe_ctx* ctx, const uint16_t* kp_depth, int kp_depth_on_host, const drfe_camera* cam,
                                         int nframes, void* stream);
/* Frame::UndistortKeyPoints / ComputeImageBounds (src/Frame.cc:835-891) for cameras with k1 != 0 (TUM1/TUM2
 * settings): dist = (k1, k2, p1, p2[, k3]) as Tracking reads Camera.k1.. into mDistCoef, cam supplies mK.  With a
 * model set, drfe_frame_stereo_grid_batch first builds mvKeysUn on the device (cv::undistortPoints(pts, K, dist,
 * Mat(), K): five fixed-point iterations in double) and the depth association, the grid and every matcher read
 * mvKeysUn, exactly as the reference does; n = 0 or k1 == 0 restores mvKeysUn = mvKeys.  The image bounds
 * (min_x, max_x, min_y, max_y of drfe_camera) come from drfe_frame_image_bounds. */
int drfe_frame_set_distortion(drfe_ctx* ctx, const drfe_camera* cam, const float* dist, int n);
int drfe_frame_image_bounds(const drfe_camera* cam, const float* dist, int n, int cols, int rows,
                            float* bounds /* min_x, max_x, min_y, max_y */);
int drfe_frame_download_keys_un(drfe_ctx* ctx, int slot, drfe_keypoint* kps, int cap);
int drfe_frame_download_stereo(drfe_ctx* ctx, int slot, float* u_right, float* depth, int cap);
/* grid as CSR in the reference's iteration order (cell = ix*48 + iy): offsets[64*48+1], indices[N] */
int drfe_frame_download_grid(drfe_ctx* ctx, int slot, int32_t* offsets, int32_t* indices, int cap);

/* ------------------------------------------------------------------------------------------------ */
/* Batches in flight: `depth` contexts used round robin, each on the stream it owns (its own hardware queue), so that the
 * latency-bound kernels of one batch (quadtree, claim resolution, glue) run beside the VALU-bound ones of the others:
 * +10-13 % device rate at depth 3, the measured optimum (bench.py uses this object).
 *   drfe_pipeline_submit   one batch through drfe_orb_extract_batch -> [d_depth != NULL: drfe_frame_stereo_grid_batch ->
 *                          Tcw && Twc: drfe_match_consecutive_batch] on the next context; asynchronous; returns the index k
 *                          (>= 0) of the context that holds the batch's results, or a negative DRFE_ERR_* code.  The caller
 *                          must have consumed the previous results of that context (depth submissions earlier).
 *                          frame_stride / row_stride count ELEMENTS of each image (bytes of d_gray, 16-bit words of d_depth).
 *   drfe_pipeline_context  context k: result access (drfe_orb_download, drfe_match_download, drfe_batch_download_async, ...)
 *                          and per-context setup (drfe_frame_set_distortion, drfe_voc_upload - once per context)
 *   drfe_pipeline_sync     waits for context k's stream (k < 0: all of them) */
typedef struct drfe_pipeline drfe_pipeline;
int drfe_pipeline_create(const drfe_config* cfg, int depth, drfe_pipeline** out);
void drfe_pipeline_destroy(drfe_pipeline* pipe);
int drfe_pipeline_depth(const drfe_pipeline* pipe);
drfe_ctx* drfe_pipeline_context(drfe_pipeline* pipe, int k);
const char* drfe_pipeline_last_error(const drfe_pipeline* pipe);
int drfe_pipeline_submit(drfe_pipeline* pipe, const uint8_t* d_gray, const uint16_t* d_depth, size_t frame_stride, size_t row_stride,
                         int w, int h, const float* Tcw, const float* Twc, const drfe_camera* cam, float th, int mono, int check_ori,
                         int nframes);
int drfe_pipeline_sync(drfe_pipeline* pipe, int k);

/* ------------------------------------------------------------------------------------------------ */
/* Per-frame pipelined flow: what Frame::Frame (src/Frame.cc:74-160) does for ONE frame, without waiting for it.
 * Tracking::GrabImageRGBD (src/Tracking.cc:191) builds one Frame at a time and matches it against the previous one:
 * frame k goes to slot k % max_batch, the slot of frame k-1 keeps LastFrame's keypoints, descriptors and grid on the
 * device for the slot-pair matchers (drfe_search_by_projection_last(cur_slot, last_slot, ...), drfe_match_orb_points,
 * drfe_search_by_bow, ...).  Other slots are not touched.
 *   drfe_frame_submit   copies the frame into pinned staging and enqueues, as one captured hipGraph per slot: H2D ->
 *                       ORBextractor::operator() -> [depth != NULL: UndistortKeyPoints / ComputeStereoFromRGBD /
 *                       AssignFeaturesToGrid with `cam` and the model of drfe_frame_set_distortion] -> D2H of mvKeys,
 *                       mDescriptors, mvuRight, mvDepth.  Returns without waiting: the calling thread is free for the host
 *                       halves of the line / plane extractors (the reference starts threads for ExtractORB / ExtractLSD /
 *                       ComputePlanes, src/Frame.cc:124-134).  depth: raw CV_16U image, rows depth_stride_elems apart,
 *                       or NULL (ORB only).  One submission per slot may be outstanding (DRFE_ERR_STATE otherwise).
 *   drfe_frame_collect  waits for that slot's submission and copies its results out (u_right / depth_m may be NULL; they
 *                       need a submission with a depth image).  Results are identical to drfe_orb_extract +
 *                       drfe_frame_stereo_grid_batch on the same frame (tests/test_gpu_match.py).
 * The batch entry points renumber the slots (a batch fills 0..nframes-1): use one context per flow. */
int drfe_frame_submit(drfe_ctx* ctx, int slot, const uint8_t* gray, int w, int h, size_t stride, const uint16_t* depth,
                      size_t depth_stride_elems, const drfe_camera* cam);
int drfe_frame_collect(drfe_ctx* ctx, int slot, drfe_keypoint* kps, uint8_t* desc, float* u_right, float* depth_m, int cap,
                       int* n_out);

/* A frame that lives on the HOST into a slot: the KeyFrame* / Frame& arguments of ORBmatcher's methods (include/ORBmatcher.h:41-84)
 * are objects of the map whose keypoints were extracted long ago (KeyFrame copies mvKeys, mvKeysUn, mDescriptors, mvuRight, mvDepth
 * from its Frame, src/KeyFrame.cc:36-66).  kps = mvKeys, kps_un = mvKeysUn (NULL: the same array), desc = mDescriptors (n x 32),
 * u_right = mvuRight, depth_m = mvDepth (either may be NULL: monocular, all -1), cam = intrinsics + the image bounds
 * mnMinX .. mnMaxY.  The arrays are uploaded as they are and Frame::AssignFeaturesToGrid (src/Frame.cc:224-237) runs on the
 * device, so the slot is indistinguishable from one the frame was extracted in; every slot-based matcher below then takes it.
 * n <= drfe_orb_max_keypoints(ctx).  Without a distortion model the context keeps one keypoint array (mvKeysUn == mvKeys) and
 * stores kps_un.  Synchronous; the slot must have no drfe_frame_submit outstanding.  The slot's BoW transform, if any, is
 * forgotten (drfe_bow_transform_slot). */
int drfe_frame_load(drfe_ctx* ctx, int slot, const drfe_keypoint* kps, const drfe_keypoint* kps_un, const uint8_t* desc,
                    const float* u_right, const float* depth_m, int n, const drfe_camera* cam);

/* ------------------------------------------------------------------------------------------------ */
/* ORBmatcher (replaces src/ORBmatcher.cc hot paths)                                                 */

/* What the matcher reads through LastFrame.mvpMapPoints[i] (MapPoint::GetWorldPos/GetDescriptor/
 * Observations, src/ORBmatcher.cc:1419-1423,1468-1470). */
typedef struct drfe_map_point {
    uint8_t valid;        /* pMP != NULL && !mvbOutlier[i] */
    uint8_t obs_positive; /* Observations() > 0 */
    uint8_t pad[2];
    float world[3];
    uint8_t desc[32];
} drfe_map_point;

/* ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1396-1535,
 * for every consecutive slot pair of a batch: cur = slot s, last = slot s-1 (s = 1..nframes-1).
 * Map points of `last` are its own keypoints with valid depth, unprojected with Twc[last]
 * (Frame::UnprojectStereo, src/Frame.cc:913-923) — the state Tracking::UpdateLastFrame leaves for an
 * RGB-D stream.  Tcw/Twc: nframes row-major 4x4 float matrices (host).  d_matches (device, may be
 * NULL) / results kept in ctx: per slot s, int32[max_keypoints]: index of the last-frame keypoint
 * matched to current keypoint i, or -1.  nnratio unused by this overload (no ratio test in the
 * reference); check_ori = mbCheckOrientation. */
/* DRFE_ERR_CAPACITY when a slot can hold more than 4096 keypoints (nfeatures > 4064 at 8 levels): one pair's map points
 * must fit the claim resolution.  drfe_search_by_projection_last has the same limit on n_last. */
int drfe_match_consecutive_batch(drfe_ctx* ctx, const float* Tcw, const float* Twc, const drfe_camera* cam,
                                 float th, int mono, int check_ori, int nframes, void* stream);
int drfe_match_download(drfe_ctx* ctx, int slot, int32_t* cur_to_last, int cap, int* nmatches);

/* General form of the same overload with caller-supplied map points for `last` slot and initial
 * CurrentFrame.mvpMapPoints claims (cur_mp in/out: -1 = NULL; cur_obs: Observations()>0 of the
 * initial claims, may be NULL = all 1). Synchronous. */
int drfe_search_by_projection_last(drfe_ctx* ctx, int cur_slot, int last_slot, const float* Tcw_cur,
                                   const float* Tcw_last, const drfe_camera* cam, const drfe_map_point* last_mp,
                                   int n_last, float th, int mono, int check_ori, const uint8_t* cur_obs,
                                   int32_t* cur_mp, int n_cur, int* nmatches);

/* ONE submission per tracked frame: drfe_frame_submit (above) followed, inside the same captured graph, by
 * ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, mono) as Tracking::TrackWithMotionModel calls it
 * (src/Tracking.cc:2181-2202; src/ORBmatcher.cc:1396-1535) - H2D -> ORB -> glue -> map points -> window search + claim
 * resolution + rotation histogram -> D2H of keypoints, descriptors, mvuRight / mvDepth AND the match array.  CurrentFrame goes
 * to `slot`, LastFrame is the frame an earlier submission left in `last_slot` (with its grid: submitted with a depth image).
 * Tcw_cur = the pose the search projects with (mVelocity * LastFrame.mTcw), Tcw_last = LastFrame.mTcw (forward / backward
 * test).  last_mp != NULL: LastFrame.mvpMapPoints as the caller's map holds them, n_last = LastFrame's keypoint count;
 * last_mp == NULL: every keypoint of LastFrame with depth, unprojected with Twc_last (Frame::UnprojectStereo) - the
 * temporal points Tracking::UpdateLastFrame creates on an RGB-D stream - built on the device, so a frame can be submitted
 * before the previous one has been collected.  CurrentFrame's claims start empty, as TrackWithMotionModel's do.  Needs a depth
 * image.  drfe_frame_collect_tracked returns what drfe_frame_collect does plus cur_to_last[n] (index of the matched
 * LastFrame keypoint per current keypoint, -1 = none) and the number of matches; results are identical to
 * drfe_frame_submit + drfe_frame_collect + drfe_search_by_projection_last (tests/test_gpu_match.py). */
int drfe_frame_submit_tracked(drfe_ctx* ctx, int slot, const uint8_t* gray, int w, int h, size_t stride, const uint16_t* depth,
                              size_t depth_stride_elems, const drfe_camera* cam, int last_slot, const float* Tcw_cur,
                              const float* Tcw_last, const float* Twc_last, const drfe_map_point* last_mp, int n_last, float th,
                              int mono, int check_ori);
int drfe_frame_collect_tracked(drfe_ctx* ctx, int slot, drfe_keypoint* kps, uint8_t* desc, float* u_right, float* depth_m, int cap,
                               int* n_out, int32_t* cur_to_last, int* n_matches);

/* What SearchByProjection(Frame&, vector<MapPoint*>&, th) reads (fields written by
 * Frame::isInFrustum, src/Frame.cc:602-657). */
typedef struct drfe_tracked_point {
    uint8_t track_in_view, bad, obs_positive, pad;
    int32_t level;   /* mnTrackScaleLevel */
    float proj_x, proj_y, proj_xr, view_cos;
    uint8_t desc[32];
} drfe_tracked_point;

/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th), src/ORBmatcher.cc:46-130.
 * frame_mp in/out: per frame keypoint the index into mps or -1. Synchronous. */
int drfe_search_by_projection_map(drfe_ctx* ctx, int slot, const drfe_tracked_point* mps, int m, float th,
                                  float nnratio, const uint8_t* claim_obs, int32_t* frame_mp, int n,
                                  int* nmatches);

/* ORBmatcher::MatchORBPoints(CurrentFrame, LastFrame), src/ORBmatcher.cc:1332-1394 — the fallback
 * Tracking uses when SearchByProjection finds < 40 matches (src/Tracking.cc:2195-2200): brute-force
 * 1-NN of the current slot's descriptors against the last slot's (both device-resident), keep
 * dist < max(2*min_dist, 15), copy map points with the reference's mvbOutlier[match counter] quirk.
 * last_mp: per last-frame keypoint the map point id or -1; cur_mp (in/out): ids written for matched
 * current keypoints; *n_pairs = the function's return value (NPair). */
int drfe_match_orb_points(drfe_ctx* ctx, int cur_slot, int last_slot, const int32_t* last_mp,
                          const uint8_t* last_outlier, int n_last, int32_t* cur_mp, int n_cur, int* n_pairs);

/* LSDmatcher descriptor matching (src/LSDmatcher.cpp): BFMatcher::knnMatch(k=2) of LBD descriptors on the
 * device + Frame::lineDescriptorMAD (src/Frame.cc:560-584) + the accept rule.
 *   mode 0  SearchByDescriptor(KeyFrame*, Frame&, ...), :242-279: query = keyframe lines, train = frame
 *           lines, accept d0/d1 < 1/1.5 when the keyframe line has a MapLine (has_line[q]);
 *           out[train idx] = query idx (later queries overwrite earlier ones), out has n_t entries.
 *   mode 1  SearchByDescriptor(KeyFrame*, KeyFrame*, ...), :281-314 and SerachForInitialize, :213-240:
 *           accept when d1 - d0 > 0.5 * MAD of that gap and has_line[train idx] (NULL = all);
 *           out[query idx] = train idx, out has n_q entries. */
int drfe_lsd_search_by_descriptor(drfe_ctx* ctx, const uint8_t* desc_q, int n_q, const uint8_t* desc_t, int n_t,
                                  const uint8_t* has_line, int mode, int32_t* out, int* nmatches);
/* LSDmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs), src/LSDmatcher.cpp:334-367 (LocalMapping::
 * CreateNewMapLines): knnMatch(k = 2) on the device, accept the nearest neighbour when the NN2-NN1 gap exceeds a tenth
 * of its MAD and neither line has a MapLine (has1 / has2).  out12[line of KF1] = line of KF2 or -1. */
int drfe_lsd_search_for_triangulation(drfe_ctx* ctx, const uint8_t* desc1, int n1, const uint8_t* desc2, int n2,
                                      const uint8_t* has1, const uint8_t* has2, int32_t* out12, int* nmatches);

/* cv::BFMatcher(NORM_HAMMING).match / knnMatch(k<=2) on 256-bit descriptors (src/ORBmatcher.cc:1346,
 * src/LSDmatcher.cpp:222,254): ascending distance, ties -> lower train index. idx/dist: nq x k. */
int drfe_match_bf_knn(drfe_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int k, int32_t* idx,
                      int32_t* dist);

/* ------------------------------------------------------------------------------------------------ */
/* LineSegment (replaces src/LSDextractor.cpp: LSDDetector::detect + BinaryDescriptor::compute)      */

/* cv::line_descriptor::KeyLine fields (angle, class_id, octave, pt, response, size, start/end point,
 * start/end point in octave, lineLength, numOfPixels). */
typedef struct drfe_keyline {
    float angle;
    int32_t class_id, octave;
    float pt_x, pt_y, response, size;
    float start_point_x, start_point_y, end_point_x, end_point_y;
    float s_point_in_octave_x, s_point_in_octave_y, e_point_in_octave_x, e_point_in_octave_y;
    float line_length;
    int32_t num_of_pixels;
} drfe_keyline;

/* LineSegment::ExtractLineSegment(img, keylines, ldesc, keylineFunctions, scale = 1.2f, numOctaves = 1),
 * src/LSDextractor.cpp:12-43.  gray: host CV_8UC1.  max_lines = lsdNFeatures (40).  Outputs: up to
 * max_lines key lines (the highest-response ones, class_id renumbered, :23-28), ldesc = NL x 32 LBD
 * bytes, line_f = NL x 3 normalised line equations; *n_detected = lines found before the cut. */
int drfe_lsd_extract(drfe_ctx* ctx, const uint8_t* gray, int w, int h, size_t stride, int max_lines,
                     drfe_keyline* lines, uint8_t* ldesc, double* line_f, int cap, int* n_lines, int* n_detected);
/* The sequential half of cv::LineSegmentDetector (pixel ordering, region growing, rectangle fit + refinement, NFA validation)
 * on caller-supplied level-line fields, without a device: what drfe_lsd_extract runs on the host between its device passes,
 * with the rectangle pixel counts taken on the host too.  modgrad / angles: W x H doubles of the 0.8-scaled image (angle
 * -1024 = undefined); cs: W x H x 2 floats, (cos, sin) of float(angle); max_grad: the largest modgrad.  segs: up to cap x 4
 * floats (x1, y1, x2, y2 in input-image coordinates).  Host code: CPU tests and profiling. */
int drfe_lsd_segments_host(const double* modgrad, const double* angles, const float* cs, int W, int H, double max_grad, float* segs,
                           int cap, int* n_segs);
/* The same for nframes host images (gray + f * frame_stride).  Default: the whole extractor runs on the DEVICE, frames side by
 * side - the image passes, std::sort's permutation of the pixel ordering (k_lsd_order), the seed loop with region_grow /
 * region2rect / refine (k_lsd_grow: one wavefront per frame executing the reference's order of operations), rect_improve with
 * its NFA decisions certified against the host libm's values (k_rect_improve, drfe_lsd_configure_nfa), the key lines, the
 * response cut's std::sort, the line equations (k_lsd_keylines) and the LBD descriptors (k_lbd); n_threads host threads upload,
 * launch and copy the results out (two are plenty), and finish on the host the rare frame a device stage hands back (an
 * uncertified rounding or comparison, a capacity: drfe_lsd_stats counts them).
 * drfe_lsd_configure(ctx, 0): every frame through drfe_lsd_extract's host path on the pool, one device lane per thread
 * (frames instead of the reference's four extractors across threads, src/Frame.cc:116-126).  Outputs per frame f at
 * lines[f * cap], ldesc[f * cap * 32], line_f[f * cap * 3], n_lines[f], n_detected[f]; results are identical to nframes
 * calls of drfe_lsd_extract either way.  n_threads <= 0: 1.25 x the CPUs this process may use (affinity mask clipped by the
 * cgroup quota). */
int drfe_lsd_extract_batch(drfe_ctx* ctx, const uint8_t* gray, size_t frame_stride, int w, int h, size_t stride, int nframes,
                           int max_lines, drfe_keyline* lines, uint8_t* ldesc, double* line_f, int cap, int* n_lines,
                           int* n_detected, int n_threads);
/* Where drfe_lsd_extract_batch grows regions: 0 on the host threads; on the device 1 (default) with the kernel chosen by the size of
 * the call, 2 with one wavefront per frame (the least device time per frame: what counts when calls of hundreds of frames run side by
 * side), 3 with four wavefronts per frame (seeds speculated against a commit-only `used` map and committed in seed order: 1.6x
 * shorter per frame, what counts when the call cannot fill the device; the default up to 256 frames per call).  Frames whose
 * 0.8-scaled size exceeds the device path's LDS bitmap (about 1.2 M pixels) take the host path regardless.  Results are identical. */
int drfe_lsd_configure(drfe_ctx* ctx, int device_grow);
/* Which reading of cv::LineSegmentDetectorImpl::rect_nfa / nfa (OpenCV 3.4 imgproc/src/lsd.cpp, the detector behind reference
 * src/LSDextractor.cpp:14-17) validates the rectangles of this context's line entries.
 * 0 (default) - the source text.  rect_nfa: `struct edge { cv::Point p; bool taken; }` has integer corners, so the four edge steps
 *   are INTEGER quotients, and the second steps use (y - tailp->p.x) in their guards and in their denominators (the scan lines of
 *   an oblique rectangle are then not the rectangle's own).  nfa: `log1term = (double(n) + 1) - log_gamma(double(k) + 1) -
 *   log_gamma(double(n-k) + 1) + ...` - the first log_gamma of the LSD paper is missing, the binomial tail all but vanishes and
 *   nearly every rectangle with k > n p passes at rect_improve's first test.  Library behaviour, preserved.
 * 1 - the LSD paper's reading of both, as rounds 2-3 shipped (double quotients, (y - tailp->p.y) denominators, a step that would
 *   divide by zero taken as 0; log_gamma(n + 1)).
 * 2 - integer corners with log_gamma(n + 1): round 4's default.
 * 1 and 2 stay until a pin against a real OpenCV 3.4.4 build decides (tools/dump_opencv_reference.py dumps the per-rectangle
 * counts and NFA values such a pin compares). */
int drfe_lsd_configure_rect(drfe_ctx* ctx, int rect_mode);
/* Where drfe_lsd_extract_batch takes the decisions of cv::LineSegmentDetectorImpl::rect_improve (OpenCV 3.4 lsd.cpp: which
 * refinement candidate replaces a rectangle, whether its NFA passes): 1 (default) on the device behind the region growing
 * (k_rect_improve: the host libm's log-gamma / log tables, its own exp / log10 / pow, every comparison certified against a
 * bound on the difference to the host's value - a frame with a comparison too close to call is validated on the host), 0 on
 * the pool threads with the caller's libm (rounds 2-3).  Results are identical. */
int drfe_lsd_configure_nfa(drfe_ctx* ctx, int device_nfa);
/* counters since drfe_create: out4[0] frames through drfe_lsd_extract_batch's device path, [1] frames whose region growing
 * returned to the host, [2] frames whose NFA decisions returned to the host, [3] frames whose key-line stage (KeyLine fields,
 * the response cut's std::sort, LBD direction: k_lsd_keylines) returned to the host */
int drfe_lsd_stats(drfe_ctx* ctx, long long* out4);
/* Kernel durations of the two long batch entries, measured live: with the clock on, drfe_lsd_extract_batch and
 * drfe_planes_ahc_post_batch bracket every kernel of their first chunk with HIP events on the stream it is launched on.
 * drfe_long_kernel_ms: the last clocked call's intervals in ms - lines [0..6]: upload, image passes, k_lsd_keys, k_lsd_order,
 * k_lsd_grow(_mw), k_rect_improve, k_lsd_keylines + k_lbd; planes [8..14]: upload, k_ahc_blocks, k_ahc_cluster, k_ahc_refine,
 * k_ahc_labels_*, k_voxel_grid, k_plane_refit ([7], [15] unused).  An interval contains whatever its kernel waited for: it is the
 * kernel's duration when the call runs alone on the device (bench.py full_frontend's solo steps). */
int drfe_long_kernel_clock(drfe_ctx* ctx, int on);
int drfe_long_kernel_ms(drfe_ctx* ctx, float* out16);
/* drfe_lsd_segments_host with rect_nfa's reading chosen by the caller (drfe_lsd_segments_host: 0). */
int drfe_lsd_segments_host_mode(const double* modgrad, const double* angles, const float* cs, int W, int H, double max_grad,
                                int rect_mode, float* segs, int cap, int* n_segs);
/* Parity taps of the device image passes of the last drfe_lsd_extract call (any pointer may be NULL):
 * 0.8-scaled image, gradient magnitude and level-line angle (sw x sh), Sobel dx/dy of the LBD image. */
int drfe_lsd_stages(drfe_ctx* ctx, uint8_t* scaled, double* modgrad, double* angles, int16_t* gx, int16_t* gy,
                    int* sw, int* sh);

/* Frame::isLineGood, src/Frame.cc:481-558, with the 3-D line lifting of src/LineExtractor.cpp:1157-1470: up to 51
 * nearest-pixel depth samples per key line, per-sample covariance, Mahalanobis RANSAC driven by rand(), refit,
 * accept if inliers / length > 0.4 and |A - B| > 0.02.  Host code (40 lines x 51 samples of double arithmetic), no
 * context needed.  depth: the CV_32F depth image in metres; K: the nine floats of mK exactly as the reference passes
 * them.  k_as_f64 = 0 reproduces the shipped behaviour — compPt3dCov reads that CV_32F matrix with at<double>, the
 * focal length becomes a subnormal, every covariance is NaN and NO line is accepted (depth_line = -1, lines3d = 0
 * for all) — by doing the same arithmetic on the same bytes; k_as_f64 = 1 runs the algorithm with f = fx as it was
 * meant (agrees with an OpenCV build to rounding, endpoint order not pinned; see lines_3d.cpp).  seed: srand() state
 * (1 = a fresh process).  Outputs per line: mvDepthLine, mvLines3D (A xyz, B xyz), optional inlier counts. */
int drfe_lines_is_good(const drfe_keyline* lines, int n, const float* depth, int w, int h, size_t stride,
                       const float* K, int k_as_f64, float cx, float cy, float invfx, float invfy, uint32_t seed,
                       float* depth_line, double* lines3d, int32_t* n_inliers, int* n_good);

/* The same for the key lines of nframes frames in one device call: frame f's key lines at lines[f * cap],
 * n_lines[f] <= cap of them - the layout drfe_lsd_extract_batch writes - and its CV_32F depth image at depth + f * frame_stride
 * (strides in floats).  depth_on_device: depth is a device pointer and nothing of it is uploaded.  One camera per call.
 * seeds[f] is frame f's srand() state; seeds == NULL: 1 for every frame.  cap <= DRFE_LINE3D_MAX_CAP. */
enum { DRFE_LINE3D_MAX_CAP = 4096 };
/* frames in a call from which drfe::Line3DBatch uses the device entry.  The crossover has not been measured (DESIGN.md section
 * 18), so by default it stays on the host entry */
enum { DRFE_LINE3D_DEVICE_FROM = 2147483647 };
typedef struct drfe_line3d_frames {
    int32_t nframes, cap;
    const drfe_keyline* lines;   /* nframes x cap */
    const int32_t* n_lines;      /* nframes */
    const float* depth;
    size_t frame_stride, stride; /* floats between two frames, between two rows (>= w) */
    int32_t w, h;
    int32_t depth_on_device, k_as_f64;
    float K[9];                  /* mK as the reference passes it */
    float cx, cy, invfx, invfy;
    const uint32_t* seeds;       /* nframes, or NULL */
} drfe_line3d_frames;
/* Frame f's results at f * cap, its first n_lines[f] entries written; n_inliers may be NULL. */
typedef struct drfe_line3d_out {
    float* depth_line;           /* nframes x cap: mvDepthLine */
    double* lines3d;             /* nframes x cap x 6: mvLines3D */
    int32_t* n_inliers;          /* nframes x cap */
    int32_t* n_good;             /* nframes */
} drfe_line3d_out;
/* Frame f's outputs are byte for byte what drfe_lines_is_good writes for it with seeds[f], in both k_as_f64 modes.  The key
 * lines and a rand() table staged with one copy (a host depth image goes up as it lies), three launches, the results back with
 * one copy; returns with the outputs written (`stream` NULL = the context's).  A call of more frames than
 * drfe_line3d_chunk_frames(cap) runs in chunks of that many. */
int drfe_lines_is_good_batch(drfe_ctx* ctx, const drfe_line3d_frames* in, drfe_line3d_out* out, void* stream);
int drfe_line3d_chunk_frames(int cap);
/* Counters since the context was created: stats[0] batch calls, [1] frames, [2] key lines, [3] key lines that ran the RANSAC
 * (at least 10 lifted samples), [4] RANSAC iterations run, [5] of those with a coincident pair, [6] candidate sets verify3dLine
 * rejected, [7] accepted lines. */
int drfe_line3d_stats(drfe_ctx* ctx, int64_t* stats /* 8 */);

/* LSDmatcher::SearchByProjection, src/LSDmatcher.cpp:20-139 (Frame, Frame) and :141-211 (Frame,
 * vector<MapLine*>), with Frame::GetLinesInArea (src/Frame.cc:781-813): project the 3-D end points with
 * Tcw (float cv::Mat path), collect the current key lines whose midpoint lies within the radius and
 * whose slope difference passes, best / second-best LBD Hamming distance in index order, TH_HIGH = 100
 * and the same-octave ratio test, sequential claims (a line already holding a MapLine with
 * Observations() > 0 is skipped).  One wavefront replays the loop on the device. */
typedef struct drfe_map_line {      /* read through LastFrame.mvpMapLines[i] / mvKeylinesUn[i] */
    int32_t valid;                  /* pML && !pML->isBad() && !mvbLineOutlier[i] */
    int32_t octave;                 /* LastFrame.mvKeylinesUn[i].octave */
    int32_t obs_positive;           /* pML->Observations() > 0 */
    int32_t pad;
    double world[6];                /* MapLine::GetWorldPos(): start xyz, end xyz */
    uint8_t desc[32];
} drfe_map_line;
typedef struct drfe_tracked_line {  /* fields Frame::isInFrustum(MapLine*) leaves on the map line */
    int32_t in_view;                /* pML && !isBad() && mbTrackInView */
    int32_t level;                  /* mnTrackScaleLevel */
    int32_t obs_positive;
    float x1, y1, x2, y2;           /* mTrackProjX1 / Y1 / X2 / Y2 */
    float view_cos;
    uint8_t desc[32];
} drfe_tracked_line;
/* cur_lines / cur_desc: the current frame's key lines (pt, angle, octave are read) and LBD rows.
 * cur_ml in/out, n_cur entries: -1 = no MapLine, >= 0 = holds one (cur_obs[i] = its Observations() > 0,
 * NULL = all); a new match writes the index of the matched last/tracked record.  Synchronous. */
int drfe_lsd_search_by_projection_last(drfe_ctx* ctx, const float* Tcw_cur, const float* Tcw_last,
                                       const drfe_camera* cam, const drfe_map_line* last_lines, int n_last,
                                       const drfe_keyline* cur_lines, const uint8_t* cur_desc, int n_cur, float th,
                                       int mono, float nnratio, const uint8_t* cur_obs, int32_t* cur_ml, int* nmatches);
int drfe_lsd_search_by_projection_map(drfe_ctx* ctx, const drfe_tracked_line* lines, int n,
                                      const drfe_keyline* cur_lines, const uint8_t* cur_desc, int n_cur, float th,
                                      float nnratio, const uint8_t* cur_obs, int32_t* cur_ml, int* nmatches);

/* Frame::isInFrustum, src/Frame.cc:602-657 (MapPoint*) and :659-727 (MapLine*), the step Tracking::SearchLocalPoints
 * runs over the local map before SearchByProjection(F, MapPoints): project with Tcw, image bounds, scale-invariance
 * distance band (0.8 * min, 1.2 * max), viewing-angle cosine against the mean normal, MapPoint::PredictScale
 * (ceil(log(max / dist) / log scaleFactor), clamped to the pyramid; MapLine::PredictScale does not clamp).  One thread
 * per map point.  log() is the shared routine drfe_logf (include/drfe_math.h) because glibc's logf is not pinned.
 * out: only the tracking fields are written (track_in_view / in_view, level, projections, view_cos): fill bad /
 * obs_positive / desc yourself and hand the array to drfe_search_by_projection_map / drfe_lsd_search_by_projection_map. */
typedef struct drfe_frustum_point { float world[3], normal[3], min_distance, max_distance; } drfe_frustum_point;
typedef struct drfe_frustum_line { double world[6], normal[3]; float min_distance, max_distance; } drfe_frustum_line;
int drfe_frame_is_in_frustum(drfe_ctx* ctx, const float* Tcw, const drfe_camera* cam, const drfe_frustum_point* pts, int n,
                             float viewing_cos_limit, drfe_tracked_point* out);
int drfe_frame_is_in_frustum_lines(drfe_ctx* ctx, const float* Tcw, const drfe_camera* cam, const drfe_frustum_line* lines,
                                   int n, float viewing_cos_limit, drfe_tracked_line* out);

/* ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>, th), src/ORBmatcher.cc:829-985 (LocalMapping::SearchInNeighbors): the
 * search.  The keyframe is a slot with extract + glue done; per map point (skip[i] = !pMP || isBad() ||
 * IsInKeyFrame(pKF), may be NULL): projection with Tcw, KeyFrame::IsInImage, distance band, 60-degree viewing cone,
 * PredictScale, KeyFrame::GetFeaturesInArea(u, v, th * scale[level]), octave in [level-1, level], chi-square
 * reprojection gate (7.8 with a right coordinate, 5.99 without), first minimum of the Hamming distance.
 * best_idx[i] = keyframe keypoint or -1, best_dist[i] = its distance (256 if none).  Applying the result
 * (bestDist <= TH_LOW: Replace / AddObservation / AddMapPoint) mutates the map graph and is the caller's loop. */
int drfe_fuse_search(drfe_ctx* ctx, int slot, const float* Tcw, const drfe_frustum_point* pts, const uint8_t* descs,
                     const uint8_t* skip, int n, float th, int32_t* best_idx, int32_t* best_dist);
/* ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, points, th, vpReplacePoint), src/ORBmatcher.cc:981-1107 (LoopClosing::
 * SearchAndFuse): the same search under a similarity pose — Scw is decomposed as the reference does (:989-993), invz is
 * 1.0 / z evaluated in double, and there is no chi-square gate. */
int drfe_fuse_search_sim3(drfe_ctx* ctx, int slot, const float* Scw, const drfe_frustum_point* pts, const uint8_t* descs,
                          const uint8_t* skip, int n, float th, int32_t* best_idx, int32_t* best_dist);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th), src/ORBmatcher.cc:1106-1330 (LoopClosing::ComputeSim3):
 * both keyframes are slots with extract + glue done; pts / descs / skip are per KEYPOINT of the keyframe (skip[i] = no good
 * map point there or already matched, :1131-1142).  Every remaining map point of KF1 is carried into KF2 by
 * (sR21, t21) — and those of KF2 into KF1 by (sR12, t12) — and searched in a th * scale[level] window (octave
 * level-1..level, distance <= TH_HIGH, first minimum) on the device; a pair is kept when both directions agree.
 * matches12[i1] = keypoint of KF2 or -1 (vpMatches12[i1] = vpMapPoints2[matches12[i1]]); *n_found = the return value. */
int drfe_search_by_sim3(drfe_ctx* ctx, int slot1, int slot2, const float* T1w, const float* T2w, float s12, const float* R12,
                        const float* t12, const drfe_frustum_point* pts1, const uint8_t* descs1, const uint8_t* skip1, int n1,
                        const drfe_frustum_point* pts2, const uint8_t* descs2, const uint8_t* skip2, int n2, float th,
                        int32_t* matches12, int* n_found);

/* ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched,
 * int th), src/ORBmatcher.cc:294-407 (LoopClosing::ComputeSim3, th = 10): the n candidate map points are projected with
 * the similarity and matched, IN ORDER, to the slot's keypoints that have no match yet: matched[k] != 0 means
 * vpMatched[k] != NULL on entry (n_kp = the slot's keypoint count), skip[i] != 0 means the point is bad or already in
 * vpMatched (:321).  new_match[k] = the point this call assigned to keypoint k (vpMatched[k] = vpPoints[new_match[k]]) or
 * -1; *n_matches = the return value.  Windows, octave gate and Hamming distances run on the device, the first-come
 * claim order is replayed on the host from the device's per-point candidate lists. */
int drfe_search_by_projection_kf(drfe_ctx* ctx, int slot, const float* Scw, const drfe_frustum_point* pts, const uint8_t* descs,
                                 const uint8_t* skip, int n, const uint8_t* matched, int n_kp, float th, int32_t* new_match,
                                 int* n_matches);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, const float th,
 * const int ORBdist), src/ORBmatcher.cc:1537-1664 (Tracking::Relocalization, src/Tracking.cc:3638 / :3651): the keyframe's
 * map points (pts / descs per entry of pKF->GetMapPointMatches(), skip[i] = !pMP || isBad() || sAlreadyFound.count(pMP),
 * kf_angles[i] = pKF->mvKeysUn[i].angle) are projected into the current frame (slot) with Tcw = CurrentFrame.mTcw — no
 * depth test, double 1/z, inclusive image bounds, 0.8 / 1.2 distance band, MapPoint::PredictScale — and matched IN ORDER
 * to the frame's keypoints without a map point (matched[k] = CurrentFrame.mvpMapPoints[k] != NULL), octaves
 * level-1..level+1, first minimum, accepted when <= orb_dist; then the rotation-histogram filter when check_orientation.
 * new_match[k] = index i of the point assigned to keypoint k (CurrentFrame.mvpMapPoints[k] = vpMPs[i]) or -1;
 * *n_matches = the return value.  A point with camera-space z == 0 is skipped (the reference projects it to infinity). */
int drfe_search_by_projection_reloc(drfe_ctx* ctx, int slot, const float* Tcw, const drfe_frustum_point* pts, const uint8_t* descs,
                                    const float* kf_angles, const uint8_t* skip, int n, const uint8_t* matched, int n_kp, float th,
                                    int orb_dist, int check_orientation, int32_t* new_match, int* n_matches);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:409-524; monocular
 * initialisation).  F1 / F2 = slots of the last extracted batch (frame glue done).  prev_matched[n1 * 2] = vbPrevMatched (x, y per
 * F1 keypoint), updated in place as the reference does; matches12[n1] = index into F2's keypoints or -1; *n_matches = the return
 * value.  nnratio / check_orientation = the ORBmatcher constructor's arguments.  A window holding more than 256 level-0
 * keypoints fails with DRFE_ERR_CAPACITY. */
int drfe_search_for_initialization(drfe_ctx* ctx, int slot1, int slot2, float* prev_matched, int n1, int window_size, float nnratio,
                                   int check_orientation, int32_t* matches12, int* n_matches);

/* LSDmatcher::Fuse(KeyFrame* pKF, const vector<MapLine*>& vpMapLines, const float th = 3.0), src/LSDmatcher.cpp:884-1010
 * (LocalMapping::SearchInNeighbors, src/LocalMapping.cc:1103 / :1124): the search per map line — both end points projected
 * with the keyframe pose (camera centre as KeyFrame::SetPose builds it), image bounds, distance band, 60-degree cone,
 * MapLine::PredictScale, KeyFrame::GetLinesInArea (src/KeyFrame.cc:749-781) over the keyframe's key lines, octave window
 * level-1..level, first minimum of the LBD Hamming distance.  skip[i] = !pML || pML->isBad().  best_idx[i] = key line
 * or -1; -2 when the predicted level is outside the pyramid (MapLine::PredictScale does not clamp and the reference then
 * reads mvScaleFactors out of bounds: undefined there, reported here).  best_dist[i] = the distance (INT_MAX when none);
 * the caller applies `<= TH_LOW` (50) and the Replace / AddObservation / AddMapLine surgery (:993-1008). */
int drfe_lsd_fuse_search(drfe_ctx* ctx, const float* Tcw, const drfe_camera* cam, const drfe_frustum_line* lines, const uint8_t* descs,
                         const uint8_t* skip, int n, const drfe_keyline* kf_lines, const uint8_t* kf_desc, int n_kf, float th,
                         int32_t* best_idx, int32_t* best_dist);
/* The search of LSDmatcher::Fuse(pKF, Scw, vpLines, th, vpReplaceLine) (src/LSDmatcher.cpp:750-882; public API without a caller in
 * the reference): as drfe_lsd_fuse_search with the pose taken from the similarity Scw (4x4 row-major, decomposed as :759-763).
 * skip[i] = !pML || isBad() || spAlreadyFound.count(pML).  The caller applies TH_LOW and the Replace / AddObservation surgery. */
int drfe_lsd_fuse_search_sim3(drfe_ctx* ctx, const float* Scw, const drfe_camera* cam, const drfe_frustum_line* lines, const uint8_t* descs,
                              const uint8_t* skip, int n, const drfe_keyline* kf_lines, const uint8_t* kf_desc, int n_kf, float th,
                              int32_t* best_idx, int32_t* best_dist);
/* LSDmatcher::SearchByProjection(pKF, Scw, vpLines, vpMatched, th) (src/LSDmatcher.cpp:377-502).  matched[n_kf] = vpMatched[idx] !=
 * NULL on entry; new_match[n_kf] = the map line that claimed key line idx in this call or -1 (the caller sets vpMatched[idx] =
 * vpLines[new_match[idx]]); *n_matches = the return value.  First come, first served over the map lines, as the reference. */
int drfe_lsd_search_by_projection_kf(drfe_ctx* ctx, const float* Scw, const drfe_camera* cam, const drfe_frustum_line* lines,
                                     const uint8_t* descs, const uint8_t* skip, int n, const drfe_keyline* kf_lines, const uint8_t* kf_desc,
                                     int n_kf, const uint8_t* matched, int th, int32_t* new_match, int* n_matches);
/* LSDmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/LSDmatcher.cpp:504-748).  lines / descs / skip: one
 * entry per key line of the keyframe (its map line; skip = none, bad, or already matched: :534-555), kf*_lines / kf*_desc the key
 * lines themselves; T1w / T2w = the keyframe poses (4x4 row-major), R12 3x3 row-major.  matches12[n1] = key line of KF2 or -1
 * (the caller stores vpMapLines2[matches12[i1]]); *n_found = the return value. */
int drfe_lsd_search_by_sim3(drfe_ctx* ctx, const drfe_camera* cam, const float* T1w, const float* T2w, float s12, const float* R12,
                            const float* t12, const drfe_frustum_line* lines1, const uint8_t* descs1, const uint8_t* skip1,
                            const drfe_keyline* kf1_lines, const uint8_t* kf1_desc, int n1, const drfe_frustum_line* lines2,
                            const uint8_t* descs2, const uint8_t* skip2, const drfe_keyline* kf2_lines, const uint8_t* kf2_desc, int n2,
                            float th, int32_t* matches12, int* n_found);

/* ------------------------------------------------------------------------------------------------ */
/* Multi-GPU, batched-sequence mode (no counterpart in the reference, whose only parallelism is the three
 * extractor threads of src/Frame.cc:124-134).  One process (or thread) per GPU, each with its own drfe_ctx / drfe_pipeline;
 * whole sequences are dealt to the ranks and NO collective runs on the data path.  The one exchange is the ORB vocabulary at
 * start-up: rank 0 loads it and broadcasts the node table over RCCL (xGMI inside a node); every rank then calls
 * drfe_voc_upload on its own context.  RCCL is loaded at run time (librccl.so.1): a single-GPU host never needs it.
 *   rank 0:     drfe_shard_unique_id(id)  -> hand the 128 bytes to the other ranks (file, pipe, MPI, environment ...)
 *   every rank: drfe_shard_create(id, nranks, rank, device, &sh)
 *               drfe_shard_broadcast(sh, &header, sizeof header, 0); drfe_shard_broadcast(sh, parent, 4 * n_nodes, 0); ... desc, weight, is_leaf
 *               drfe_voc_upload(ctx, k, L, scoring, weighting, n_nodes, parent, desc, weight, is_leaf)
 *               ... its sequences (drfe_shard_sequences_of_rank) through drfe_pipeline_submit ...
 *               drfe_shard_reduce_report(sh, &seconds, 1, &frames, 1)      MAX of the times, SUM of the frames: whole-job frames/s
 *               drfe_shard_destroy(sh) */
typedef struct drfe_shard drfe_shard;
#define DRFE_SHARD_ID_BYTES 128
int drfe_shard_unique_id(uint8_t* id /* DRFE_SHARD_ID_BYTES */);
int drfe_shard_create(const uint8_t* id, int nranks, int rank, int device, drfe_shard** out);
void drfe_shard_destroy(drfe_shard* shard);
/* a HOST buffer from rank `root` to every rank (staged through device memory, one ncclBroadcast); collective: every rank calls it */
int drfe_shard_broadcast(drfe_shard* shard, void* buf, size_t bytes, int root);
/* in place on every rank: element-wise MAX over the ranks of n_max doubles, SUM of n_sum 64-bit counters; collective */
int drfe_shard_reduce_report(drfe_shard* shard, double* max_inout, int n_max, long long* sum_inout, int n_sum);
/* sequences dealt round robin (sequence i -> rank i % nranks): writes up to cap indices of rank's share, returns their number */
int drfe_shard_sequences_of_rank(int n_sequences, int nranks, int rank, int* out, int cap);
const char* drfe_shard_last_error(const drfe_shard* shard /* NULL: the calling thread's last creation error */);

/* ------------------------------------------------------------------------------------------------ */
/* Bag of words (replaces the DBoW2 tree descent of Frame::ComputeBoW, src/Frame.cc:828-833, and
 * ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...), src/ORBmatcher.cc:160-292)                        */

/* Upload a vocabulary in the node format of TemplatedVocabulary::loadFromTextFile
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424): node 0 is the root; for node i >= 1
 * parent[i], is_leaf[i], 32 descriptor bytes, weight.  Children of a node are ordered by node id and
 * word ids are assigned to leaves in node order, exactly as the loader does.  k <= 20, L <= 10, at most 32
 * children per node.  DRFE_ERR_INVALID when is_leaf[i] disagrees with whether node i has children (a file
 * DBoW2 never writes); a rejected table leaves the previous vocabulary in place. */
int drfe_voc_upload(drfe_ctx* ctx, int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                    const uint8_t* desc, const double* weight, const uint8_t* is_leaf);
/* Device part of TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup) for the
 * descriptors of slots 0..nframes-1: per feature the word id, the word weight and the node id at level
 * L-levelsup.  Asynchronous on `stream`. */
int drfe_bow_transform_batch(drfe_ctx* ctx, int levelsup, int nframes, void* stream);
/* The same for the frame in ONE slot (drfe_frame_submit / drfe_frame_load): Frame::ComputeBoW / KeyFrame::ComputeBoW.  The transform
 * is a pure function of descriptors and vocabulary: a keyframe loaded from the host gets the mFeatVec it stored at creation.
 * Every call that writes a slot's descriptors (drfe_orb_extract, drfe_orb_extract_batch, drfe_frame_submit(_tracked),
 * drfe_frame_load, drfe_pipeline_submit) drops the slot's transform: the BoW calls then return DRFE_ERR_STATE for that
 * slot until it is transformed again. */
int drfe_bow_transform_slot(drfe_ctx* ctx, int levelsup, int slot, void* stream);
/* Per-feature results of a slot.  The caller folds them into BowVector / FeatureVector (std::map) in
 * feature order — addWeight's float64 sums depend on that order (BowVector.cpp). */
int drfe_bow_download(drfe_ctx* ctx, int slot, int32_t* word, double* weight, int32_t* nid, int cap);
/* ORBmatcher(nnratio, checkOri).SearchByBoW(pKF = kf_slot, F = f_slot, vpMapPointMatches).
 * kf_mp[i] >= 0 iff keyframe keypoint i holds a non-bad MapPoint.  f_match[j] = keyframe keypoint index
 * matched to frame keypoint j, or -1; *nmatches = return value. */
int drfe_search_by_bow(drfe_ctx* ctx, int kf_slot, int f_slot, const int32_t* kf_mp, int n_kf, float nnratio,
                       int check_ori, int32_t* f_match, int n_f, int* nmatches);
/* ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12), src/ORBmatcher.cc:526-660 (LoopClosing::ComputeSim3): the keyframe-
 * keyframe overload — keypoints of BOTH keyframes need a good map point (mp >= 0) and the test is bestDist1 < TH_LOW.
 * match2[keypoint of KF2] = keypoint of KF1 or -1, i.e. vpMatches12[match2[i2]] = vpMapPoints2[i2]. */
int drfe_search_by_bow_kf(drfe_ctx* ctx, int slot1, int slot2, const int32_t* mp1, int n1, const int32_t* mp2, int n2,
                          float nnratio, int check_ori, int32_t* match2, int* nmatches);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo), src/ORBmatcher.cc:661-827 (LocalMapping::
 * CreateNewMapPoints): for every vocabulary node common to both keyframes, match the keypoints of KF1 without a map
 * point against those of KF2 (distance <= TH_LOW, epipole exclusion, CheckDistEpipolarLine against F12, rotation
 * histogram).  Both slots need the glue (mvKeysUn, mvuRight) and drfe_bow_transform_batch.  mp1 / mp2: >= 0 where the
 * keyframe keypoint already has a map point.  F12: 3x3 row-major; Cw1: KF1 camera centre (GetCameraCenter); T2w: KF2
 * pose (4x4 row-major); cam2: KF2 intrinsics.  matches12[i1] = keypoint of KF2 or -1 (vMatchedPairs = the pairs with
 * a match, ascending i1). */
int drfe_search_for_triangulation(drfe_ctx* ctx, int slot1, int slot2, const int32_t* mp1, int n1, const int32_t* mp2, int n2,
                                  const float* F12, const float* Cw1, const float* T2w, const drfe_camera* cam2,
                                  int only_stereo, int check_ori, int32_t* matches12, int* nmatches);

/* ------------------------------------------------------------------------------------------------ */
/* PlaneDetection (replaces src/PlaneExtractor.cpp:7-63 + include/peac/ : the live AHC extractor)   */

/* One extracted plane: ahc::PlaneSeg fields Frame::ComputePlanes reads (src/Frame.cc:952-979:
 * plane_filter.extractedPlanes[i]->normal / center), plus mse, curvature, N, rid. */
typedef struct drfe_plane {
    double normal[3];   /* unit normal pointing towards the camera (dot(normal, center) <= 0) */
    double center[3];   /* centre of mass, metres */
    double mse, curvature;
    int32_t n_points;   /* PlaneSeg::N (points of the merged init blocks) */
    int32_t rid;        /* root block id */
} drfe_plane;

/* PlaneDetection::readDepthImage(depth16, K, depthfactor) + runPlaneDetection().
 * depth: host CV_16U image, `stride` elements per row; K4 = {fx, fy, cx, cy} (the float K entries the
 * reference promotes to double); depth_factor = the float passed as `depthfactor` (1/DepthMapFactor).
 * Outputs: planes[0..n) sorted by N descending (extractedPlanes); seg (w*h, may be NULL) = seg_output
 * (plane index + 1, 0 = none); member_offsets[n+1] / member_idx (may be NULL) = plane_vertices_ as CSR,
 * pixel indices ascending. */
int drfe_planes_ahc(drfe_ctx* ctx, const uint16_t* depth, int w, int h, size_t stride, const float* K4,
                    float depth_factor, drfe_plane* planes, int cap, int* n_planes, uint8_t* seg,
                    int32_t* member_offsets, int32_t* member_idx);
/* drfe_planes_ahc for nframes host depth images (depth + f * frame_stride elements).  Default (drfe_planes_configure_extractor
 * (ctx, 1), frames up to 640 x 480 class, nframes > 1): clustering / flood fill / re-merge run on the device, one wavefront per
 * frame (ahc_frame_kernels.hip), the n_threads host threads only fetch results; otherwise the per-frame sequential host code
 * (~3.5 ms) runs on n_threads host threads, one device lane each.  Outputs per frame f at
 * planes[f * cap], n_planes[f], seg + f * w * h, member_offsets[f * (cap + 1)], member_idx + f * w * h (the last three
 * may be NULL); identical to nframes single calls.  n_threads <= 0: 1.25 x the CPUs this process may use (affinity mask clipped by
 * the cgroup quota). */
int drfe_planes_ahc_batch(drfe_ctx* ctx, const uint16_t* depth, size_t frame_stride, int w, int h, size_t stride, int nframes,
                          const float* K4, float depth_factor, drfe_plane* planes, int cap, int* n_planes, uint8_t* seg,
                          int32_t* member_offsets, int32_t* member_idx, int n_threads);
/* Parity tap of the device stage: per 10x10 init block 17 doubles (9 sums, center, normal, mse,
 * curvature) and (enters-graph flag, N). cap = number of blocks the buffers hold. */
int drfe_planes_ahc_blocks(drfe_ctx* ctx, const uint16_t* depth, int w, int h, size_t stride, const float* K4,
                           float depth_factor, double* blocks17, int32_t* valid_n, int cap);

/* The host half of drfe_planes_ahc on caller-supplied block fits (the records drfe_planes_ahc_blocks returns), without a device:
 * graph, agglomerative clustering, block membership, flood fill, re-merge and labels.  Host code: CPU tests and profiling. */
int drfe_planes_ahc_from_blocks(const double* blocks17, const int32_t* valid_n, const uint16_t* depth, int w, int h, size_t stride,
                                const float* K4, float depth_factor, drfe_plane* planes, int cap, int* n_planes, uint8_t* seg,
                                int32_t* member_offsets, int32_t* member_idx);

/* PlaneDetection_CAPE (replaces src/PlaneExtractor.cpp:65-191 + src/CAPE/{CAPE,PlaneSeg,Histogram}.cpp;
 * its thread launch is commented out in the reference, src/Frame.cc:129, but the class is public API).
 * One entry of plane_params (CAPE PlaneSeg: normal, d, mean, MSE, score, nr_pts). */
typedef struct drfe_cape_plane {
    double normal[3];
    double mean[3];
    double d;           /* plane equation normal . p + d = 0, d > 0 */
    float mse, score;
    int32_t n_points;
    int32_t pad;
} drfe_cape_plane;

/* PlaneDetection_CAPE::readDepthImage(depth32f, K) + runPlaneDetection().  depth_m: host CV_32F depth in
 * metres (`stride` elements per row); patch = PATCH_SIZE (Plane.PATCH_SIZE: 20 or 10); cos_angle_max =
 * COS_ANGLE_MAX (cos(pi/12)); max_merge_dist = MAX_MERGE_DIST (Plane.MAX_MERGE_DIST: 50).  w and h must
 * be multiples of patch.  Outputs: planes[0..n), seg (w*h) = seg_output (plane number, 0 = none).
 * Parity taps (may be NULL): per cell 16 doubles (9 sums, mean, normal, d), 3 floats (MSE, score,
 * merge tolerance), 2 ints (planar, nr_pts). */
int drfe_planes_cape(drfe_ctx* ctx, const float* depth_m, int w, int h, size_t stride, const float* K4, int patch,
                     float cos_angle_max, float max_merge_dist, drfe_cape_plane* planes, int cap, int* n_planes,
                     uint8_t* seg, double* cells16, float* cells_mst, int32_t* cells_pn);
/* The same for nframes depth images (metres; frame f at depth_m + f * frame_stride floats): planes[f * cap ..], n_planes[f],
 * seg[f * w * h ..] (seg may be NULL).  Default (drfe_planes_configure_cape(ctx, 1), nframes > 1): end to end on the device -
 * cell fits, CAPE::process (one wavefront per frame), per-pixel refinement - from the calling thread, which uploads the frames
 * through two pinned staging buffers and copies the results out; n_threads host threads (one device lane each) only for frames
 * the device hands back and in the host mode.  Identical to nframes calls of drfe_planes_cape.  n_threads <= 0: up to 4. */
int drfe_planes_cape_batch(drfe_ctx* ctx, const float* depth_m, size_t frame_stride, int w, int h, size_t stride, int nframes,
                           const float* K4, int patch, float cos_angle_max, float max_merge_dist, drfe_cape_plane* planes, int cap,
                           int* n_planes, uint8_t* seg, int n_threads);

/* ------------------------------------------------------------------------------------------------ */
/* Plane post-processing and surface normals (replaces the PCL part of Frame::ComputePlanes / ComputePlanes_CAPE,  */
/* src/Frame.cc:949-1094, 1096-1213, and Frame::MaxPointDistanceFromPlane, src/Frame.cc:1222-1307)                 */

/* One plane after the per-plane loop of Frame::ComputePlanes (:952-1011): coef = the 4x1 float Mat pushed into
 * mvPlaneCoefficients when accepted (normal, d AFTER the RANSAC + least-squares refit of MaxPointDistanceFromPlane, sign
 * kept on the side of the extractor's d), else the extractor's (normal, d); n_voxels = coarseCloud->size(). */
typedef struct drfe_plane_post {
    float coef[4];
    int32_t accepted;   /* 1: coefficients + voxel cloud pushed (mvPlaneCoefficients / mvPlanePoints) */
    int32_t n_voxels;
} drfe_plane_post;

/* pcl::VoxelGrid (leaf x leaf x leaf) of a point list in inputCloud order: centroids ordered by leaf index.  Host code. */
int drfe_plane_voxel_grid(const float* xyz, int n, float leaf, float* out_xyz, int cap, int* n_out);
/* Frame::MaxPointDistanceFromPlane(plane, cloud) with Plane.DistanceThreshold = dist_threshold: *valid = its return value;
 * coef4 is overwritten by the refit when valid.  Host code. */
int drfe_plane_refit(float* coef4, const float* xyz, int n, double dist_threshold, int* valid);

/* The per-plane loop of Frame::ComputePlanes for the planes drfe_planes_ahc returned (same depth image, K4, depth_factor;
 * planes / member_offsets / member_idx as that call filled them).  max_point_dist = Point.MaxDistance, dist_threshold =
 * Plane.DistanceThreshold.  Outputs: post[n_planes]; voxel_offsets[n_planes + 1] + voxel_xyz (may be NULL) = mvPlanePoints
 * of the accepted planes as CSR; *n_accepted = mvPlaneCoefficients.size(); *plane_num (may be NULL) = planeDetector.plane_num_
 * after `-= fail_planes`.  Host code: ctx may be NULL (no error text then). */
int drfe_planes_ahc_postprocess(drfe_ctx* ctx, const uint16_t* depth, int w, int h, size_t stride, const float* K4, float depth_factor,
                                const drfe_plane* planes, int n_planes, const int32_t* member_offsets, const int32_t* member_idx,
                                float max_point_dist, double dist_threshold, drfe_plane_post* post, float* voxel_xyz,
                                int32_t* voxel_offsets, int cap_voxels, int* n_accepted, int* plane_num);
/* drfe_planes_ahc_batch and, on the same worker thread, drfe_planes_ahc_postprocess of every frame: the plane path of nframes host
 * depth images end to end.  planes / post: [nframes][cap]; n_planes / n_accepted / plane_num (may be NULL): [nframes]; seg (may be
 * NULL): [nframes][w*h].  The voxel clouds are not returned here.  n_threads <= 0: the CPUs this process may use. */
int drfe_planes_ahc_post_batch(drfe_ctx* ctx, const uint16_t* depth, size_t frame_stride, int w, int h, size_t stride, int nframes,
                               const float* K4, float depth_factor, float max_point_dist, double dist_threshold, drfe_plane* planes,
                               int cap, int* n_planes, uint8_t* seg, drfe_plane_post* post, int* n_accepted, int* plane_num, int n_threads);
/* Where drfe_planes_ahc_post_batch runs pcl::VoxelGrid (leaf 0.05) of a frame's planes (voxel_kernels.hip: leaf indices,
 * std::sort's permutation by the device introsort, centroid sums in that order - one workgroup per plane).  1 (default): on the
 * device behind the device extractor, which also gathers each plane's cloud (one launch for all planes of the batch; the pool's
 * threads fetch centroids and run gates + refit); the host-extractor mode keeps the host grid.  2: on the device in the
 * host-extractor mode too (one launch per frame from each pool thread).  0: always on the pool's host threads.  Results are
 * identical (tests/test_gpu_post.py). */
int drfe_planes_configure(drfe_ctx* ctx, int device_voxel_grid);
/* Where drfe_planes_ahc_post_batch runs the gates and Frame::MaxPointDistanceFromPlane (src/Frame.cc:1003-1011, 1222-1307: RANSAC with
 * pcl's mt19937 sample sequence, adaptive iteration bound, least-squares refit, sign) of every plane: 1 (default) on the device behind
 * the device voxel grids, one wavefront per plane (refit_kernels.hip) - the pool's threads then receive 24-byte post records instead of
 * voxel clouds; 0 on the pool's host threads.  A plane whose libm-dependent roundings the device cannot certify sends its frame to the
 * host's refit (drfe_planes_refit_stats counts them).  Results are identical (tests/test_gpu_post.py). */
int drfe_planes_configure_refit(drfe_ctx* ctx, int on_device);
/* out2[0] = frames whose gates + refit ran on the device since drfe_create, out2[1] = of those, sent to the host's refit */
int drfe_planes_refit_stats(drfe_ctx* ctx, long long* out2);
/* Where drfe_planes_ahc_post_batch runs PEAC's extractor after the init-block fits (graph, agglomerative clustering, block
 * membership, flood fill, re-merge, labels and member lists): 1 (default) on the device, one wavefront per frame executing the
 * reference's sequence (ahc_frame_kernels.hip), the batch's frames side by side; 0 on the pool's host threads (the path of
 * drfe_planes_ahc).  Results are identical (tests/test_gpu_post.py, tests/test_gpu_planes.py). */
int drfe_planes_configure_extractor(drfe_ctx* ctx, int on_device);
/* out4[0] = frames through the device extractor (drfe_planes_ahc_batch / drfe_planes_ahc_post_batch) since drfe_create, out4[1] = of
 * those, redone on the host (a capacity of the device path ran out, a cosine could not be certified), out4[2] = plane voxel grids
 * run on the device, out4[3] = of those, redone on the host.  The device extractor takes frames of up to 12 800 init blocks and
 * 2^21 pixels (1280 x 960, BASELINE config 5, included); larger frames run on the pool's host threads and are not counted. */
int drfe_planes_ahc_stats(drfe_ctx* ctx, long long* out4);
/* Where drfe_planes_cape_batch runs CAPE::process between the cell fits and the per-pixel refinement (src/CAPE/CAPE.cpp:81-293:
 * normal histogram + seeding, cell growing, segment fits, merging, erode / dilate masks): 1 (default) on the device, one wavefront
 * per frame (cape_frame_kernels.hip; a frame whose histogram bins the device cannot certify - acos / atan2 are the host libm's in
 * the reference - is finished by the host), 0 on the pool's host threads.  Results are identical. */
int drfe_planes_configure_cape(drfe_ctx* ctx, int on_device);
/* out2[0] = frames through drfe_planes_cape_batch's device path since drfe_create, out2[1] = of those, finished by the host */
int drfe_planes_cape_stats(drfe_ctx* ctx, long long* out2);
/* The same loop of Frame::ComputePlanes_CAPE (:1111-1141) for the planes / seg image drfe_planes_cape returned: plane_cloud[i]
 * = the points of the pixels labelled i + 1 in raster order (src/PlaneExtractor.cpp:171-188). */
int drfe_planes_cape_postprocess(drfe_ctx* ctx, const float* depth_m, int w, int h, size_t stride, const float* K4, const uint8_t* seg,
                                 const drfe_cape_plane* planes, int n_planes, float max_point_dist, double dist_threshold,
                                 drfe_plane_post* post, float* voxel_xyz, int32_t* voxel_offsets, int cap_voxels, int* n_accepted,
                                 int* plane_num);

/* SurfaceNormal (include/LSDextractor.h:34-41): cv::Point3f normal, cv::Point3f cameraPosition, cv::Point2i FramePosition */
typedef struct drfe_surface_normal {
    float normal[3];            /* NaN where PCL leaves the normal undefined (border, depth discontinuity) */
    float camera_position[3];
    int32_t frame_x, frame_y;
} drfe_surface_normal;

/* vSurfaceNormal of Frame::ComputePlanes (:1025-1090): depth_m = the CV_32F depth in metres (`stride` elements per row),
 * K4 = {fx, fy, cx, cy} (Frame's static floats).  out[(h3/2) * (w3/2)] with w3 = ceil(w/3), h3 = ceil(h/3), rows of odd m,
 * inside a row odd n, as the reference pushes them.  Parity taps (may be NULL): the organized cloud (w3*h3*3), every normal
 * (w3*h3*3), the distance map (w3*h3). */
int drfe_surface_normals(drfe_ctx* ctx, const float* depth_m, int w, int h, size_t stride, const float* K4, float max_point_dist,
                         drfe_surface_normal* out, int cap, int* n_out, float* cloud_tap, float* normals_tap, float* dist_tap);
/* The same for nframes device-resident raw depth images (CV_16U; depth = raw * depth_factor in float32, as
 * imDepth.convertTo does): asynchronous on `stream` (hipStream_t; NULL = the context stream), results stay on the device. */
int drfe_surface_normals_batch(drfe_ctx* ctx, const uint16_t* d_depth, size_t frame_stride, size_t row_stride, int w, int h,
                               const float* K4, float depth_factor, float max_point_dist, int nframes, void* stream);
/* Records of frame `slot` of the most recent drfe_surface_normals_batch (synchronises). */
int drfe_surface_normals_download(drfe_ctx* ctx, int slot, drfe_surface_normal* out, int cap, int* n_out);

/* Manhattan-frame tracking (Tracking::TrackManhattanFrame, src/Tracking.cc:1336-1527, with ProjectSN2Conic :1198-1266,
 * ProjectSN2MF :1055-1196 and MeanShift :1529-1546).  One call refines R_cm (Manhattan frame -> camera, row-major 3x3 float)
 * from a frame's SurfaceNormal records and optional line directions (FrameLine::direction, 3 doubles each); Tracking::Track
 * chains three calls per frame (:328-332), each starting from the previous call's output.  Bit-exact with the reference's
 * arithmetic (asin / exp / tanf canonicalised in drfe_math.h; the OpenCV pieces unpinned: DESIGN.md section 11).
 *
 * Side outputs rebuild what the reference leaves on the frame: rec_bits[i] (one per record) and line_bits[l] (one per line)
 * have bit 3 * call + axis (axis 0..2 = x, y, z) set when ProjectSN2MF pushed the record / line to that axis's list
 * (Frame::vSurfaceNormalx/y/z and vSurfacePointx/y/z; vVanishingLinex/y/z) in that call, NaN m_j included, and bit 15
 * when it was inside a cone of the conic pass in any call (bsurfacenormal_inline).  The lists are call-major, then record
 * order. */
#define DRFE_MANHATTAN_MAX_CALLS 5
#define DRFE_MANHATTAN_INLINE_BIT 0x8000
typedef struct drfe_manhattan_call {
    int32_t in_cone[3];     /* normals inside each axis's cone (conic pass, numInCone) */
    int32_t n_selected[3];  /* m_j_selected.size() per axis (non-NaN m_j of normals and lines in the mean-shift cone) */
    int32_t threshold;      /* minNumOfSN used: records / 20 (NaN records counted), or (smallest + middle) / 2 */
    int32_t deficient;      /* 1 when the "normal vector deficiency" rule replaced the threshold */
    int32_t found;          /* bit a: axis a's column was replaced (sum of the new column != 0) */
    int32_t svd;            /* 1 when 2 or 3 axes were found and R = U * VT ran */
    float density[3];       /* MeanShift density of each axis taken (n_selected > threshold), else 0 */
    int32_t pad;
} drfe_manhattan_call;      /* 56 B */
typedef struct drfe_manhattan_info {
    int32_t n_calls, pad;
    drfe_manhattan_call call[DRFE_MANHATTAN_MAX_CALLS];
} drfe_manhattan_info;      /* 288 B */

/* Single frame on the host, no context: n_calls (1..DRFE_MANHATTAN_MAX_CALLS, the reference uses 3) chained calls from
 * R_in to R_out.  line_dirs may be NULL when n_lines == 0; info, rec_bits (n) and line_bits (n_lines) may be NULL. */
int drfe_manhattan_track_host(const float* R_in, const drfe_surface_normal* recs, int n, const double* line_dirs, int n_lines,
                              int n_calls, float* R_out, drfe_manhattan_info* info, uint16_t* rec_bits, uint16_t* line_bits);
/* The same for nseq * seq_len frames of the context's most recent drfe_surface_normals_batch, read in place on the device:
 * frame s * seq_len + t is frame t of sequence s; frame 0 of sequence s starts from R0 + 9 * s (host), frame t > 0 from
 * frame t - 1's result (mLastRcm).  line_dirs (host, 3 doubles per line) / line_offsets (host, nseq * seq_len + 1 entries)
 * give each frame's lines, both NULL for none.  Asynchronous on `stream` (hipStream_t; NULL = the context stream). */
int drfe_manhattan_track_batch(drfe_ctx* ctx, const float* R0, int nseq, int seq_len, const double* line_dirs,
                               const int32_t* line_offsets, int n_calls, void* stream);
/* Results of frame `frame` of the most recent drfe_manhattan_track_batch (synchronises): R (9 floats), info, rec_bits (the
 * frame's record count) and line_bits (the frame's line count); any may be NULL. */
int drfe_manhattan_download(drfe_ctx* ctx, int frame, float* R, drfe_manhattan_info* info, uint16_t* rec_bits,
                            uint16_t* line_bits);

/* Plane association (PlaneMatcher::SearchMapByCoefficients, src/PlaneMatcher.cpp:11-91 with PointDistanceFromPlane :206-226;
 * Map::FlagMatchedPlanePoints, src/Map.cc:406-431; PlaneMatcher::bMatchStatus, src/PlaneMatcher.cpp:94-201).  Tracking calls
 * SearchMapByCoefficients up to twice per frame (src/Tracking.cc:2202, 2332, 2451, 2584, 2807) and FlagMatchedPlanePoints once
 * (:532).  Frame planes are camera-frame coefficients (Frame::mvPlaneCoefficients, 4 floats); world coefficients are
 * transpose(Tcw) * coef (Frame::ComputePlaneWorldCoeff, src/Frame.cc:1311-1317).  A map plane is its world coefficients
 * (MapPlane::GetWorldPos), its isBad() and its merged cloud (mvPlanePoints, xyz floats) in CSR form: plane j owns points
 * [cloud_offsets[j], cloud_offsets[j + 1]) of cloud_xyz.  Map planes are indexed in vpMapPlanes order; -1 is a null pointer.
 * Bit-exact with the reference's float arithmetic; DESIGN.md section 12. */
typedef struct drfe_plane_match_params {
    float dTh, aTh, verTh, parTh;   /* PlaneMatcher's constructor arguments; the reference's defaults 0.1, 0.86, 0.08716, 0.9962 */
} drfe_plane_match_params;

/* SearchMapByCoefficients on one frame, on the host, no context.  map_idx / par_idx / ver_idx (n_planes each:
 * mvpMapPlanes / mvpParallelPlanes / mvpVerticalPlanes) are in / out: the reference does not reset them, so an entry the
 * call does not assign keeps what it held.  *nmatches = the return value (frame planes that found a map plane). */
int drfe_plane_match_host(const drfe_plane_match_params* params, const float* Tcw, const float* coefs, int n_planes,
                          const float* map_coefs, const uint8_t* map_bad, const int32_t* cloud_offsets, const float* cloud_xyz,
                          int n_map, int32_t* map_idx, int32_t* par_idx, int32_t* ver_idx, int* nmatches);
/* FlagMatchedPlanePoints on one frame, on the host: every frame plane with map_idx[i] >= 0 (its map plane's isBad() is not
 * read) sets flags[p] = 1 for the map points p (xyz floats, MapPoint::GetWorldPos) with |world coef . (x, y, z, 1)| < 0.5;
 * flags are only ever set (SetAssociatedWithPlaneFlag(true)), never cleared.  The reference's dTh argument is unused there and
 * has no counterpart.  *n_pairs (may be NULL) = the reference's nMatches, the number of (plane, point) pairs that passed. */
int drfe_plane_flag_points_host(const float* Tcw, const float* coefs, int n_planes, const int32_t* map_idx, const float* points_xyz,
                                int n_points, uint8_t* flags, int* n_pairs);
/* bMatchStatus on one frame, on the host: matched_coefs[i] (4 floats) and matched[i] describe mvpMapPlanes[i] (matched 0: null
 * or isBad(), skipped).  Rwc_MF (row-major 3x3) is read only when MF_contrast != 0; with MF_contrast == 0 the reference reads an
 * uninitialised angle_MF, canonicalised to 0 here (the test then never fails).  *status = the return value (1 = true). */
int drfe_plane_match_status_host(const drfe_plane_match_params* params, const float* Tcw, const float* coefs, int n_planes,
                                 const float* matched_coefs, const uint8_t* matched, int MF_contrast, const float* Rwc_MF,
                                 int* status);

/* Device-resident maps of drfe_plane_match_batch: n_maps maps, map s owning map planes [plane_offsets[s], plane_offsets[s + 1])
 * of map_coefs / map_bad / cloud_offsets (plane-local order = vpMapPlanes order; cloud_offsets has one entry per plane plus
 * one, global into cloud_xyz) and map points [point_offsets[s], point_offsets[s + 1]) of points_xyz (mspMapPoints, any order).
 * Replaces the previous upload (synchronises). */
int drfe_plane_map_upload(drfe_ctx* ctx, int n_maps, const int32_t* plane_offsets, const float* map_coefs, const uint8_t* map_bad,
                          const int32_t* cloud_offsets, const float* cloud_xyz, const int32_t* point_offsets,
                          const float* points_xyz);
/* SearchMapByCoefficients (then, with flag_points, FlagMatchedPlanePoints) of nframes frames on the device, each against map
 * frame_map[f] as uploaded: frame f has planes [plane_offsets[f], plane_offsets[f + 1]) of coefs (4 floats each) and pose
 * Tcw + 16 f.  map_idx / par_idx / ver_idx: the prior contents of the three pointer vectors, plane-local map indices, one per
 * frame plane (NULL = all null).  Host inputs; asynchronous on `stream` (hipStream_t; NULL = the context stream). */
int drfe_plane_match_batch(drfe_ctx* ctx, const drfe_plane_match_params* params, int nframes, const int32_t* frame_map,
                           const float* Tcw, const int32_t* plane_offsets, const float* coefs, const int32_t* map_idx,
                           const int32_t* par_idx, const int32_t* ver_idx, int flag_points, void* stream);
/* Results of frame `frame` of the most recent drfe_plane_match_batch (synchronises): the three index arrays (the frame's plane
 * count each), *nmatches and *n_pairs (0 without flag_points); any may be NULL. */
int drfe_plane_match_download(drfe_ctx* ctx, int frame, int32_t* map_idx, int32_t* par_idx, int32_t* ver_idx, int* nmatches,
                              int* n_pairs);
/* The map-point flags of map `map` after the most recent drfe_plane_match_batch with flag_points: the OR over every frame of
 * that map in the call (0 everywhere for a map no frame used); one byte per map point (synchronises). */
int drfe_plane_flags_download(drfe_ctx* ctx, int map, uint8_t* flags);

/* MapPlane::UpdateCoefficientsAndPoints (src/MapPlane.cc:298-371): a map plane's cloud (mvPlanePoints, xyz floats) becomes
 * pcl::VoxelGrid(0.05) of new points followed by its current cloud, or of its keyframe observations alone.  The SAC
 * segmentation the reference runs afterwards writes only locals and has no counterpart.  DESIGN.md section 13.
 *
 * Per-frame form (pMP->UpdateCoefficientsAndPoints(F, i)), on the host: frame_xyz (n_frame points, F.mvPlanePoints[i]) moved
 * into world by Isometry3d(Converter::toSE3Quat(Tcw)).inverse() - the rotation's quaternion round trip, not the plain
 * transpose - then map_xyz (n_map points, the plane's cloud) after them, then the voxel grid.  *n_out = the output's points;
 * DRFE_ERR_CAPACITY when that exceeds cap (n_frame + n_map always suffices). */
int drfe_map_plane_update_host(const float* Tcw, const float* frame_xyz, int n_frame, const float* map_xyz, int n_map, float* out_xyz,
                               int cap, int* n_out);
/* Observation form (pMP->UpdateCoefficientsAndPoints()), on the host: for each of n_obs observations (KF, idx) in the order
 * given (the reference iterates GetObservations(), a std::map keyed by KeyFrame*), the cloud KF->mvPlanePoints[idx] = points
 * [obs_cloud_offsets[o], obs_cloud_offsets[o + 1]) of obs_xyz moved by Twc + 16 o (KF->GetPoseInverse(), widened element by
 * element), concatenated, then the voxel grid. */
int drfe_map_plane_rebuild_host(int n_obs, const float* Twc, const int32_t* obs_cloud_offsets, const float* obs_xyz, float* out_xyz,
                                int cap, int* n_out);
/* The per-frame form on the resident maps of drfe_plane_map_upload: frame f (pose Tcw + 16 f, planes [plane_offsets[f],
 * plane_offsets[f + 1]), frame plane q's cloud = points [cloud_offsets[q], cloud_offsets[q + 1]) of cloud_xyz) updates the
 * planes of map frame_map[f] that map_idx[q] names (plane-local, -1 = none; the reference's test is mvpMapPlanes[i] != NULL,
 * priors included, isBad() not read).  map_idx NULL = the decisions of the most recent drfe_plane_match_batch, which must have
 * had the same frame_map and plane_offsets (DRFE_ERR_STATE otherwise).  Updates of one map plane apply in call order (frame,
 * then frame plane); clouds grow without bound on the device.  Host inputs, `stream` as drfe_plane_match_batch; the call
 * returns once the clouds are updated (it reads each round's voxel counts back, 4 bytes per update). */
int drfe_plane_map_update_batch(drfe_ctx* ctx, int nframes, const int32_t* frame_map, const float* Tcw, const int32_t* plane_offsets,
                                const int32_t* cloud_offsets, const float* cloud_xyz, const int32_t* map_idx, void* stream);
/* The observation form on the resident maps: job k replaces the cloud of plane job_plane[k] of map job_map[k] with the voxel
 * grid of its observations [obs_offsets[k], obs_offsets[k + 1]) (pose Twc + 16 o, cloud [cloud_offsets[o], cloud_offsets[o + 1])
 * of cloud_xyz), in the order given.  Same stream and return rules as drfe_plane_map_update_batch. */
int drfe_plane_map_rebuild_batch(drfe_ctx* ctx, int njobs, const int32_t* job_map, const int32_t* job_plane, const int32_t* obs_offsets,
                                 const float* Twc, const int32_t* cloud_offsets, const float* cloud_xyz, void* stream);
/* Edits n planes of resident map `map`: plane_index[k] < the map's plane count sets that plane's coefficients (coefs + 4 k,
 * MapPlane::SetWorldPos; coefs may be NULL) and bad flag (bad[k], SetBadFlag; bad may be NULL); plane_index[k] == the count
 * appends a plane (coefs required, bad NULL = 0) with an empty cloud, for drfe_plane_map_rebuild_batch to fill.  All-or-nothing
 * validation; synchronises. */
int drfe_plane_map_edit(drfe_ctx* ctx, int map, int n, const int32_t* plane_index, const float* coefs, const uint8_t* bad);
/* The current cloud of plane `plane` of map `map` (synchronises): *n = its points; xyz NULL asks for the size only;
 * DRFE_ERR_CAPACITY when *n > cap. */
int drfe_plane_map_cloud_download(drfe_ctx* ctx, int map, int plane, float* xyz, int cap, int* n);
/* Counters since drfe_plane_map_upload: stats[0] voxel jobs the device finished, [1] jobs redone on the host (grid overflow or
 * the sort's heap-sort branch), [2] rounds, [3] arena repacks (clouds that outgrew their slots). */
int drfe_plane_map_update_stats(drfe_ctx* ctx, int64_t* stats /* 4 */);

/* LocalMapping::MapPlaneCulling (src/LocalMapping.cc:233-307) with Map::PointDistanceFromPlane (src/Map.cc:433-448) and
 * MapPlane::Replace (src/MapPlane.cc:197-271) over all planes of one map in vpMapPlanes order (GetAllMapPlanes(); null entries
 * are not supported).  Row i scans the merged cloud of every later plane j that passes the angle gate against plane i's
 * coefficients; the nearest below dTh is merged with i (the one with fewer observations is replaced, plane i on a tie), and the
 * survivor's cloud becomes the voxel grid of its merged observations (the observation form above).  Then the recent-plane
 * list is walked.  DESIGN.md section 30.
 *
 * Per plane: found / visible (mnFound, mnVisible), n_obs (nObs), first_kf_id ((int)mnFirstKFid) and mObservations in CSR form in
 * std::map<KeyFrame*> order: observation o of plane p, o in [obs_offsets[p], obs_offsets[p + 1]), is plane obs_idx[o] of key
 * frame obs_kf[o].  obs_kf indexes the call's key-frame table, which is in pointer order too, so inside one plane obs_kf
 * increases strictly.  Twc + 16 k is key frame k's GetPoseInverse().  The cloud of observation o (KF->mvPlanePoints[idx]) is
 * obs_cloud_n[o] points, point q's x y z being the three floats at (const char*)obs_cloud[o] + q * obs_cloud_stride; it is
 * read only when a survivor that holds the observation is rebuilt.
 * recent: mlpRecentAddedMapPlanes as plane indices, -1 for a plane that has left the map (bad by construction, erased). */
enum { DRFE_PLANE_CULL_KEPT = 0, DRFE_PLANE_CULL_ERASED_BAD = 1, DRFE_PLANE_CULL_BAD_BY_RATIO = 2,
       DRFE_PLANE_CULL_BAD_BY_OBSERVATIONS = 3, DRFE_PLANE_CULL_ERASED_BY_AGE = 4 };
typedef struct drfe_plane_cull_in {
    int32_t n_planes, n_kfs, n_recent, current_kf_id;    /* current_kf_id: (int)mpCurrentKeyFrame->mnId */
    double dTh, aTh;                                     /* Plane.AssociationDisRef / AngRef, doubles in the reference */
    const int32_t *found, *visible, *n_obs, *first_kf_id;            /* n_planes each */
    const int32_t *obs_offsets, *obs_kf, *obs_idx;       /* n_planes + 1; one per observation */
    const float* const* obs_cloud;                       /* one per observation; may be NULL where obs_cloud_n is 0 */
    const int32_t* obs_cloud_n;
    int32_t obs_cloud_stride;                            /* bytes between points, >= 12 (sizeof(PointT) for a PCL cloud) */
    const float* Twc;                                    /* n_kfs x 16 */
    const int32_t* recent;                               /* n_recent */
} drfe_plane_cull_in;
typedef struct drfe_plane_cull_out {
    int32_t n_events, n_rebuilt;
    int32_t* events;            /* n_planes x 2: (replaced, survivor) in the order they happen, at most one per row */
    uint8_t* bad;               /* n_planes each: isBad(), nObs, mnFound, mnVisible after the call */
    int32_t *n_obs, *found, *visible;
    int32_t* rebuilt;           /* n_planes: the planes whose cloud was rebuilt, ascending, each once */
    int32_t* rebuilt_offsets;   /* n_planes + 1: plane rebuilt[k]'s cloud = points [rebuilt_offsets[k], rebuilt_offsets[k + 1]) */
    float* rebuilt_xyz;
    int32_t rebuilt_capacity;   /* points; DRFE_ERR_CAPACITY when too small (the sum of obs_cloud_n always suffices) */
    uint8_t* verdicts;          /* n_recent: DRFE_PLANE_CULL_*; every verdict but KEPT erases the list entry, BAD_BY_* after SetBadFlag */
    int64_t counters[4];        /* pairs scanned, cloud points scanned, clouds rebuilt, rebuilt clouds read again as a column */
} drfe_plane_cull_out;
/* On the host, no context: map_coefs (4 per plane, GetWorldPos), map_bad and the clouds in CSR form as drfe_plane_match_host
 * takes them.  DRFE_ERR_INVALID on an argument out of range (offsets, key-frame or recent indices, observation order, stride);
 * nothing is written then. */
int drfe_plane_map_cull_host(const drfe_plane_cull_in* in, const float* map_coefs, const uint8_t* map_bad,
                             const int32_t* cloud_offsets, const float* cloud_xyz, drfe_plane_cull_out* out);
/* The same on resident map `map` of drfe_plane_map_upload, whose coefficients, bad flags and clouds are read in place:
 * DRFE_ERR_STATE when in->n_planes is not the map's plane count.  Same outputs, byte for byte.  On success the call commits into
 * the resident map with nothing re-uploaded: the bad flags, and the rebuilt clouds through the rounds of
 * drfe_plane_map_rebuild_batch (drfe_plane_map_update_stats counts them); with DRFE_ERR_CAPACITY for rebuilt_capacity the map is
 * committed all the same and drfe_plane_map_cloud_download still returns the clouds.  mode 0 runs on the device from
 * DRFE_PLANE_CULL_DEVICE_FROM planes and below it runs the host walk on the downloaded clouds; 1 forces the device, 2 the host
 * walk, 3 the device with one row per tile (a per-pair work list, kept for measurement).  More than
 * DRFE_PLANE_CULL_MAX_PLANES planes always take the host walk.  Synchronises. */
enum { DRFE_PLANE_CULL_MAX_PLANES = 16384, DRFE_PLANE_CULL_DEVICE_FROM = 16385 };
int drfe_plane_map_cull_batch(drfe_ctx* ctx, int map, const drfe_plane_cull_in* in, int mode, drfe_plane_cull_out* out, void* stream);
/* out[0] cloud points of one chunk of the distance pass, [1] gated rows of one tile, [2] DRFE_PLANE_CULL_DEVICE_FROM,
 * [3] DRFE_PLANE_CULL_MAX_PLANES */
int drfe_plane_map_cull_limits(int32_t* out4);
/* Counters since drfe_plane_map_upload: stats[0] calls, [1] calls that took the device pass, [2] distance launches (the first
 * pass and one per recomputed column), [3] rebuild calls into the rounds (one per stale column or replaced survivor, one for
 * the end-of-call batch). */
int drfe_plane_map_cull_stats(drfe_ctx* ctx, int64_t* stats /* 4 */);

/* Map-point and map-line upkeep: MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (src/MapPoint.cc:288-350,
 * 376-411) and MapLine::ComputeDistinctiveDescriptors + UpdateAverageDir (src/MapLine.cpp:241-318, 320-362) for n independent
 * items.  Each item lists its observations in the caller's order (the reference iterates a std::map<KeyFrame*, size_t>, so
 * pointer order; the adaptor passes GetObservations()'s order): the order decides the tie-break and the float sums.
 * DESIGN.md section 14.
 *
 * `what`: DRFE_UPKEEP_DESCRIPTOR, DRFE_UPKEEP_NORMAL or both (the two halves are independent).
 * Descriptor: a bad item, one without observations, or one whose observations all name bad keyframes is unchanged; otherwise
 *   the rows of the observations of non-bad keyframes, in order, and the first row with the strictly least median Hamming
 *   distance to the rows (its own 0 included; median = element (N - 1) / 2 of the sorted row).  best_obs = that row's index in
 *   the item's observation list (bad-keyframe observations counted), desc = its 32 bytes.
 * Normal (every observation counts, bad keyframes too): points sum (X - Ow) / |X - Ow| in float as OpenCV evaluates it, lines
 *   the endpoints' middle minus Ow normalised in double; divided by the observation count; max = |P - Ow_ref| * scale[ref_level],
 *   min = max / scale[n_levels - 1] (P = X, or the float middle of a line).  A bad item or one without observations is unchanged.
 * Every output slot is written: an unchanged half leaves best_obs = -1 and zero bytes / normal / distances; status[i] holds the
 * DRFE_UPKEEP_* bits of the halves computed.  frustum (optional) gets drfe_frustum_point / drfe_frustum_line records as
 * Frame::isInFrustum reads them (world, normal, 0.8f * min, 1.2f * max) for items whose normal was computed, zero records
 * otherwise; with desc they feed drfe_frame_is_in_frustum, drfe_search_by_projection_map and drfe_fuse_search as they stand. */
enum { DRFE_UPKEEP_DESCRIPTOR = 1, DRFE_UPKEEP_NORMAL = 2 };
typedef struct drfe_upkeep_keyframes {
    int32_t n;                   /* keyframes the observations and ref_kf index */
    int32_t n_levels;            /* mnScaleLevels */
    const float* center;         /* 3 per keyframe: GetCameraCenter() */
    const uint8_t* bad;          /* 1 per keyframe: isBad(); NULL = none bad */
    const float* scale_factors;  /* mvScaleFactors, n_levels entries */
} drfe_upkeep_keyframes;
typedef struct drfe_upkeep_items {
    int32_t n;                   /* items */
    int32_t pad;
    const uint8_t* bad;          /* 1 per item: isBad(); NULL = none bad */
    const int32_t* obs_offsets;  /* n + 1: item i observes [obs_offsets[i], obs_offsets[i + 1]); obs_offsets[0] == 0 */
    const int32_t* obs_kf;       /* keyframe of each observation */
    const uint8_t* obs_desc;     /* 32 bytes per observation: pKF->mDescriptors.row(idx) / mLineDescriptors.row(idx) */
    const void* world;           /* per item: float[3] GetWorldPos() of a point, double[6] (head, tail) of a line */
    const int32_t* ref_kf;       /* per item: GetReferenceKeyFrame() as a keyframe index */
    const int32_t* ref_level;    /* per item: the octave of pRefKF->mvKeysUn / mvKeyLines[observations[pRefKF]] (index 0 when
                                  * the ref keyframe is not among the observations: operator[] on the copy inserts 0) */
} drfe_upkeep_items;
typedef struct drfe_upkeep_out {
    int32_t* best_obs;           /* per item; NULL = not wanted (as every output but status) */
    uint8_t* desc;               /* 32 per item */
    void* normal;                /* per item: float[3] (points) or double[3] (lines) */
    float* max_distance;
    float* min_distance;
    uint8_t* status;             /* per item, required */
    void* frustum;               /* per item: drfe_frustum_point (points) or drfe_frustum_line (lines) */
} drfe_upkeep_out;
/* On the host, no context.  DRFE_ERR_INVALID on an argument out of range (offsets, keyframe indices, ref_level of an item
 * whose normal is computed). */
int drfe_map_point_upkeep_host(int what, const drfe_upkeep_keyframes* kfs, const drfe_upkeep_items* items, drfe_upkeep_out* out);
int drfe_map_line_upkeep_host(int what, const drfe_upkeep_keyframes* kfs, const drfe_upkeep_items* items, drfe_upkeep_out* out);
/* The same on the device: host inputs staged with one copy, the kernels, the results back with one copy; returns with the
 * outputs written (`stream` NULL = the context's).  Same bits as the host entries.  An item with more than
 * DRFE_UPKEEP_DEVICE_ROWS descriptor rows has its descriptor computed by the host entry's code during the call (counted). */
#define DRFE_UPKEEP_DEVICE_ROWS 2048
int drfe_map_point_upkeep_batch(drfe_ctx* ctx, int what, const drfe_upkeep_keyframes* kfs, const drfe_upkeep_items* items,
                                drfe_upkeep_out* out, void* stream);
int drfe_map_line_upkeep_batch(drfe_ctx* ctx, int what, const drfe_upkeep_keyframes* kfs, const drfe_upkeep_items* items,
                               drfe_upkeep_out* out, void* stream);
/* Counters since the context was created: stats[0] batch calls, [1] items, [2..5] descriptors computed on the device by
 * bucket (rows <= 4: four lanes per item, <= 16: sixteen lanes, <= 64: one wavefront, <= DRFE_UPKEEP_DEVICE_ROWS: one
 * workgroup), [6] descriptors handed back to the host, [7] normals computed on the device. */
int drfe_map_upkeep_stats(drfe_ctx* ctx, int64_t* stats /* 8 */);

/* Map-point and map-line triangulation: the per-match body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:383-538)
 * and CreateNewMapLines2 (:875-1026), RGB-D / stereo branch (mbMonocular == false; `monocular` != 0 is rejected), with
 * KeyFrame::UnprojectStereo and obtain3DLine (src/KeyFrame.cc:788-815).  DESIGN.md section 15.
 *
 * A pair is (KF1 = the current keyframe, KF2 = a neighbour) with its matches (idx1, idx2) in vMatchedIndices order; the matching
 * (SearchForTriangulation), object creation and AddObservation stay with the caller.  A pair is skipped when
 * (float)cv::norm(Ow2 - Ow1) < KF2's mb.  Per match: the status (DRFE_TRI_ACCEPTED or the code of the `continue` that fired,
 * one per site, in the reference's order), the branch taken, and the point (x3d[3]) or the line's endpoints (sp, ep: x3d[6],
 * the floats that the reference's Vector6d widens) of an accepted match, zeros otherwise.
 * Points: stereo = mvuRight >= 0; a stereo keypoint must have mvDepth > 0 (UnprojectStereo's empty Mat would throw in the
 *   reference), else DRFE_ERR_INVALID.
 * Lines: only the stereo branches create a line; bStereo2 reads KF1's mvDepthLine[idx2], as the reference.  When idx2 is past
 *   KF1's key lines the reference reads out of bounds: the entries take bStereo2 = false and set DRFE_TRI_IDX2_PAST_KF1 in the
 *   status (the one deliberate deviation). */
enum {
    DRFE_TRI_ACCEPTED = 0,
    DRFE_TRI_BASELINE = 1,        /* the pair was skipped: baseline < pKF2->mb */
    DRFE_TRI_NO_PARALLAX = 2,     /* points: no stereo and too little parallax; lines: neither end stereo */
    /* points */
    DRFE_TRI_W_ZERO = 3,          /* x3D(3) == 0 */
    DRFE_TRI_Z1 = 4, DRFE_TRI_Z2 = 5, DRFE_TRI_REPROJ1 = 6, DRFE_TRI_REPROJ2 = 7,
    DRFE_TRI_DIST = 8,            /* dist1 == 0 || dist2 == 0 */
    DRFE_TRI_SCALE = 9,           /* scale consistency */
    /* lines */
    DRFE_TRI_L_Z_SP1 = 3, DRFE_TRI_L_Z_EP1 = 4, DRFE_TRI_L_Z_SP2 = 5, DRFE_TRI_L_Z_EP2 = 6,
    DRFE_TRI_L_REPROJ_SP1 = 7, DRFE_TRI_L_REPROJ_EP1 = 8, DRFE_TRI_L_REPROJ_SP2 = 9, DRFE_TRI_L_REPROJ_EP2 = 10,
    DRFE_TRI_L_DIST = 11, DRFE_TRI_L_SCALE = 12,
    DRFE_TRI_IDX2_PAST_KF1 = 0x80 /* flag (lines): idx2 >= KF1's key-line count, bStereo2 taken as false */
};
enum { DRFE_TRI_BRANCH_NONE = 0, DRFE_TRI_BRANCH_SVD = 1, DRFE_TRI_BRANCH_STEREO1 = 2, DRFE_TRI_BRANCH_STEREO2 = 3 };
typedef struct drfe_tri_keyframe {
    float Tcw[12];               /* [Rcw | tcw], 3x4 row-major: GetRotation(), GetTranslation() */
    float Twc[12];               /* the stored Twc's top three rows (UnprojectStereo and obtain3DLine read it) */
    float Ow[3];                 /* GetCameraCenter() */
    float fx, fy, cx, cy, invfx, invfy;
    float mb, mbf;
    float scale_factor;          /* mfScaleFactor */
} drfe_tri_keyframe;
typedef struct drfe_tri_keyframes {
    int32_t n;                   /* keyframes the pairs index */
    int32_t n_levels;            /* mnScaleLevels */
    const drfe_tri_keyframe* kf;
    const float* scale_factors;  /* n x n_levels: mvScaleFactors */
    const float* level_sigma2;   /* n x n_levels: mvLevelSigma2 */
} drfe_tri_keyframes;
typedef struct drfe_tri_keypoints {
    const int32_t* offsets;      /* n + 1: keyframe k's keypoints are [offsets[k], offsets[k + 1]) of the arrays below */
    const float* un;             /* 2 per keypoint: mvKeysUn[i].pt */
    const float* raw;            /* 2 per keypoint: mvKeys[i].pt (UnprojectStereo reads the distorted keys) */
    const int32_t* octave;       /* mvKeysUn[i].octave */
    const float* u_right;        /* mvuRight */
    const float* depth;          /* mvDepth */
} drfe_tri_keypoints;
typedef struct drfe_tri_keylines {
    const int32_t* offsets;      /* n + 1, as for keypoints */
    const float* ends;           /* 4 per line: startPointX, startPointY, endPointX, endPointY of mvKeyLines[i] */
    const int32_t* octave;       /* mvKeyLines[i].octave */
    const float* depth;          /* mvDepthLine */
    const double* lines3d;       /* 6 per line: mvLines3D[i] (camera frame) */
} drfe_tri_keylines;
typedef struct drfe_tri_pairs {
    int32_t n;                   /* pairs */
    int32_t pad;
    const int32_t* kf1;          /* per pair: the current keyframe */
    const int32_t* kf2;          /* per pair: the neighbour */
    const int32_t* match_offsets;/* n + 1: pair p's matches are [match_offsets[p], match_offsets[p + 1]); [0] == 0 */
    const int32_t* matches;      /* 2 per match: idx1 (KF1), idx2 (KF2) */
} drfe_tri_pairs;
typedef struct drfe_tri_out {
    uint8_t* status;             /* per match, required */
    uint8_t* branch;             /* per match: DRFE_TRI_BRANCH_*; NULL = not wanted (as every output but status) */
    float* x3d;                  /* per match: 3 floats (points) or 6 (lines: sp, ep) */
    uint8_t* pair_skipped;       /* per pair */
    int32_t* accepted;           /* per pair: matches accepted */
} drfe_tri_out;
/* On the host, no context.  DRFE_ERR_INVALID on an argument out of range (keyframe, feature or octave indices, offsets). */
int drfe_triangulate_points_host(int monocular, const drfe_tri_keyframes* kfs, const drfe_tri_keypoints* kps,
                                 const drfe_tri_pairs* pairs, drfe_tri_out* out);
int drfe_triangulate_lines_host(int monocular, const drfe_tri_keyframes* kfs, const drfe_tri_keylines* kls,
                                const drfe_tri_pairs* pairs, drfe_tri_out* out);
/* The same on the device, one lane per match: the inputs staged with one copy, the results back with one copy; returns with the
 * outputs written (`stream` NULL = the context's).  Same bits as the host entries.  The pairs of one call must not depend on
 * each other's results (the caller keeps CreateNewMap*'s loop over the neighbours of one keyframe: points made for neighbour i
 * change which keypoints SearchForTriangulation may use for neighbour i + 1). */
int drfe_triangulate_points_batch(drfe_ctx* ctx, int monocular, const drfe_tri_keyframes* kfs, const drfe_tri_keypoints* kps,
                                  const drfe_tri_pairs* pairs, drfe_tri_out* out, void* stream);
int drfe_triangulate_lines_batch(drfe_ctx* ctx, int monocular, const drfe_tri_keyframes* kfs, const drfe_tri_keylines* kls,
                                 const drfe_tri_pairs* pairs, drfe_tri_out* out, void* stream);
/* Counters since the context was created, points and lines together: stats[0] batch calls, [1] pairs, [2] pairs skipped,
 * [3] matches, [4] SVD branch, [5] stereo branch of KF1, [6] of KF2, [7] accepted. */
int drfe_triangulate_stats(drfe_ctx* ctx, int64_t* stats /* 8 */);

/* Sim3Solver (src/Sim3Solver.cc), the RANSAC between SearchByBoW(KF, KF) and SearchBySim3 in LoopClosing::ComputeSim3
 * (src/LoopClosing.cc:277-446): every hypothesis of every solver of a call at once.  DESIGN.md section 16.
 *
 * A solver is two keyframes and its compacted correspondences (those the constructor keeps, in i1 order; isBad,
 * GetIndexInKeyFrame and mvnIndices1 stay with the caller).  The inlier count of a hypothesis does not depend on an earlier one,
 * so the entries fill the whole table: row h of a solver is what iteration h of iterate() computes, `best` and `returns` what its
 * bookkeeping makes of the counts of rows 0 .. h, and the reference's iterate(nIterations, ..) is a walk over the table.
 * The one deviation: rand() is process-wide and unseeded in the reference; here each solver draws from a glibc rand() stream of
 * its own, srand(seed), and iteration h uses draws 3h .. 3h + 2.
 * Caps: DRFE_SIM3_MAX_CORR correspondences per solver, DRFE_SIM3_MAX_ITERATIONS for max_iterations; above them the call is
 * refused (DRFE_ERR_INVALID), as are decreasing offsets, min_inliers < 0 and a sigma2 with 9.210 * sigma2 outside [0, 2^63). */
enum { DRFE_SIM3_MAX_CORR = 4096, DRFE_SIM3_MAX_ITERATIONS = 300 };
typedef struct drfe_sim3_problems {
    int32_t n;                   /* solvers */
    int32_t pad;
    const float* Tcw1;           /* n x 12: [Rcw | tcw] of pKF1, 3x4 row-major */
    const float* Tcw2;           /* n x 12: of pKF2 */
    const float* K1;             /* n x 4: fx, fy, cx, cy of pKF1->mK */
    const float* K2;             /* n x 4 */
    const uint8_t* fix_scale;    /* n: mbFixScale */
    const double* probability;   /* n: SetRansacParameters' arguments */
    const int32_t* min_inliers;  /* n */
    const int32_t* max_iterations; /* n: <= DRFE_SIM3_MAX_ITERATIONS; below 1 counts as 1, as the reference clamps */
    const uint32_t* seed;        /* n */
    const int32_t* offsets;      /* n + 1: solver s's correspondences are [offsets[s], offsets[s + 1]); [0] == 0 */
    const float* Xw1;            /* 3 per correspondence: pMP1->GetWorldPos() */
    const float* Xw2;            /* 3 per correspondence: pMP2->GetWorldPos() */
    const float* sigma2_1;       /* per correspondence: pKF1->mvLevelSigma2[kp1.octave] */
    const float* sigma2_2;
} drfe_sim3_problems;
/* Every pointer is required.  Solver s owns the rows [row0(s), row0(s) + cap(s)), cap(s) = max(1, max_iterations[s]), row0 the
 * prefix sum of cap; its masks start at word mask0(s), the prefix sum of cap(s) * words(s), words(s) = ceil(N(s) / 64), row h at
 * mask0(s) + h * words(s), correspondence i in bit i % 64 of word i / 64.  Rows from hypotheses[s] on are zero. */
typedef struct drfe_sim3_out {
    int32_t* iterations;         /* n: mRansacMaxIts after SetRansacParameters' clamp */
    int32_t* hypotheses;         /* n: rows filled: iterations[s], or 0 when N < min_inliers (iterate returns at once with
                                    bNoMore) or N < 3 (the reference would index an empty vector) */
    int32_t* sample;             /* rows x 3: the sampled correspondences in draw order */
    float* R12;                  /* rows x 9: mR12i */
    float* t12;                  /* rows x 3: mt12i */
    float* s12;                  /* rows: ms12i */
    float* T12;                  /* rows x 12: the upper 3x4 of mT12i */
    int32_t* inliers;            /* rows: mnInliersi */
    uint8_t* returns;            /* rows: 1 = iterate hands the transform back at this iteration */
    int32_t* best;               /* rows: the iteration that holds mBest* after this one */
    uint64_t* mask;              /* mvbInliersi */
} drfe_sim3_out;
/* On the host, no context. */
int drfe_sim3_ransac_host(const drfe_sim3_problems* problems, drfe_sim3_out* out);
/* The same on the device: the inputs staged with one copy, four launches, the table back with one copy; returns with the outputs
 * written (`stream` NULL = the context's).  Same bits as the host entry. */
int drfe_sim3_ransac_batch(drfe_ctx* ctx, const drfe_sim3_problems* problems, drfe_sim3_out* out, void* stream);
/* Counters since the context was created: stats[0] batch calls, [1] solvers, [2] hypotheses, [3] correspondences, [4] solvers
 * whose correspondences the counting kernel kept in LDS, [5] solvers it read from global memory, [6] hypotheses the device
 * could not certify (atan2, sin / cos) and the host finished, [7] solvers without a hypothesis. */
int drfe_sim3_stats(drfe_ctx* ctx, int64_t* stats /* 8 */);

/* PnPsolver (src/PnPsolver.cc), the RANSAC between SearchByBoW(KF, F) and the relocalisation SearchByProjection in
 * Tracking::Relocalization (src/Tracking.cc:3540-3700): every row of every solver of a call at once.  DESIGN.md section 17.
 *
 * A solver is a frame's intrinsics and its compacted correspondences (those the constructor keeps, in match order; isBad and
 * mvKeyPointIndices stay with the caller).  Row h of a solver is what iteration h of iterate() computes from draws 4h .. 4h + 3 of
 * the solver's own glibc rand() stream, srand(seed) (the deviation of section 16: the reference's stream is process-wide).
 * iterate's loop is `while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)`, so a call that starts at or above
 * mRansacMaxIts still runs nIterations rows: a solver's table has iterations + tail rows, tail the caller's.  best[h] is the row
 * that holds mBest* after row h (-1: none), Refine() runs over the inliers of every distinct best row and its result is stored
 * at that row; returns[h] says iterate hands the refined pose of best[h] back at row h.  minSet is 4.
 * Caps: DRFE_PNP_MAX_CORR correspondences per solver, DRFE_PNP_MAX_ITERATIONS for max_iterations, DRFE_PNP_MAX_TAIL for tail,
 * 65 535 solvers, DRFE_PNP_MAX_ROWS rows and DRFE_PNP_MAX_MASK_WORDS mask words per call; above them the call is refused
 * (DRFE_ERR_INVALID), as are decreasing offsets, min_inliers < 0, tail < 0
 * and a sigma2 * th2 that is not finite. */
enum { DRFE_PNP_MAX_CORR = 4096, DRFE_PNP_MAX_ITERATIONS = 300, DRFE_PNP_MAX_TAIL = 300 };
/* per call, over all its solvers: rows of the caller's table (the sum of cap(s)) and words of one of its two masks (128 MiB) */
enum { DRFE_PNP_MAX_ROWS = 1048576, DRFE_PNP_MAX_MASK_WORDS = 16777216 };
/* solvers in a call from which drfe::PnPBatch uses the device entry (the measured crossover) */
enum { DRFE_PNP_DEVICE_FROM = 4 };
typedef struct drfe_pnp_problems {
    int32_t n;                   /* solvers */
    int32_t pad;
    const float* K;              /* n x 4: fx, fy, cx, cy of the frame (widened to the double fu, fv, uc, vc) */
    const double* probability;   /* n: SetRansacParameters' arguments */
    const int32_t* min_inliers;  /* n */
    const int32_t* max_iterations; /* n: <= DRFE_PNP_MAX_ITERATIONS; below 1 counts as 1, as the reference clamps */
    const float* epsilon;        /* n */
    const float* th2;            /* n */
    const int32_t* tail;         /* n: rows past mRansacMaxIts, 0 .. DRFE_PNP_MAX_TAIL */
    const uint32_t* seed;        /* n */
    const int32_t* offsets;      /* n + 1: solver s's correspondences are [offsets[s], offsets[s + 1]); [0] == 0 */
    const float* p2d;            /* 2 per correspondence: F.mvKeysUn[i].pt */
    const float* Xw;             /* 3 per correspondence: pMP->GetWorldPos() */
    const float* sigma2;         /* per correspondence: F.mvLevelSigma2[kp.octave] */
} drfe_pnp_problems;
/* Every pointer is required.  Solver s owns the rows [row0(s), row0(s) + cap(s)), cap(s) = max(1, max_iterations[s]) + tail[s],
 * row0 the prefix sum of cap; its masks (and refined masks) start at word mask0(s), the prefix sum of cap(s) * words(s),
 * words(s) = ceil(N(s) / 64), row h at mask0(s) + h * words(s), correspondence i in bit i % 64 of word i / 64.  Rows from
 * hypotheses[s] on are zero, as are the refined_* fields of a row that is no row's best.  Every NaN of R, t, refined_R and
 * refined_t is the quiet NaN 0x7FF8000000000000. */
typedef struct drfe_pnp_out {
    int32_t* iterations;         /* n: mRansacMaxIts after SetRansacParameters' clamp */
    int32_t* min_inliers;        /* n: mRansacMinInliers after SetRansacParameters' adjustment */
    int32_t* hypotheses;         /* n: rows filled: iterations[s] + tail[s], or 0 when N < min_inliers (iterate returns at once
                                    with bNoMore) */
    int32_t* refines;            /* n: rows Refine ran over */
    int32_t* sample;             /* rows x 4: the sampled correspondences in draw order */
    double* R;                   /* rows x 9: mRi */
    double* t;                   /* rows x 3: mti */
    int32_t* inliers;            /* rows: mnInliersi */
    uint64_t* mask;              /* mvbInliersi */
    int32_t* best;               /* rows: the row that holds mBest* after this one, -1 before the first */
    uint8_t* returns;            /* rows: 1 = iterate hands the refined pose of best back at this row */
    double* refined_R;           /* rows x 9: mRi after Refine over the inliers of this row */
    double* refined_t;           /* rows x 3 */
    int32_t* refined_inliers;    /* rows: mnRefinedInliers */
    uint64_t* refined_mask;      /* mvbRefinedInliers, laid out as mask */
} drfe_pnp_out;
/* On the host, no context. */
int drfe_pnp_ransac_host(const drfe_pnp_problems* problems, drfe_pnp_out* out);
/* The same on the device: the inputs staged with one copy, six launches, the table back with one copy; returns with the outputs
 * written (`stream` NULL = the context's).  Same bits as the host entry. */
int drfe_pnp_ransac_batch(drfe_ctx* ctx, const drfe_pnp_problems* problems, drfe_pnp_out* out, void* stream);
/* Counters since the context was created: stats[0] batch calls, [1] solvers, [2] rows, [3] correspondences, [4] refine jobs,
 * [5] correspondences the refine jobs ran over, [6] solvers whose correspondences the counting kernel read from global memory
 * (the others with rows were kept in LDS), [7] solvers without a row. */
int drfe_pnp_stats(drfe_ctx* ctx, int64_t* stats /* 8 */);

/* Initializer (src/Initializer.cc), the RANSAC behind ORBmatcher::SearchForInitialization in Tracking::MonocularInitialization
 * (src/Tracking.cc:1657-1760): the point-only Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated) of every solver
 * of a call at once.  DESIGN.md section 19.
 *
 * A solver is one Initializer object plus one Initialize call: mK, sigma, the iteration count, every undistorted key of the
 * reference and of the current frame (Normalize sums over all of them) and vMatches12, one int32 per reference key.  Its matches
 * are the reference keys with vMatches12 >= 0 in index order, N of them.  Row h of a solver is iteration h of FindHomography and
 * of FindFundamental on the same eight matches, draws 8h .. 8h + 7 of the solver's own glibc rand() stream, srand(seed) (the
 * deviation of section 16: the reference calls srand(0) once per process, so seed 0 reproduces a process's first Initialize).
 * best_h[h] / best_f[h] is the row that holds the model after row h (strict `>`, -1: none).  Then RH, the branch, the 8 (H) or
 * 4 (F) motion hypotheses with what CheckRT makes of each, and the reference's choice among them.
 * What the reference leaves undefined is refused or flagged: N < 8 (RandomInt(0, -1)) gives no rows and ok = 0; SH + SF == 0
 * (RH is NaN and ReconstructF would multiply an empty F21) gives ok = 0 and DRFE_INIT_NO_MODEL; a CheckRT whose accepted cosines
 * hold a NaN (std::sort on NaN) sets DRFE_INIT_MOTION_NAN_COS on the hypothesis, which orders a NaN above every number.
 * Caps: DRFE_INIT_MAX_KEYS keys per frame, DRFE_INIT_MAX_ITERATIONS, 65 535 solvers, DRFE_INIT_MAX_ROWS rows and
 * DRFE_INIT_MAX_MASK_WORDS words of one mask per call; above them the call is refused (DRFE_ERR_INVALID), as are decreasing
 * offsets, a negative max_iterations and a match that is not -1 or an index into the current frame's keys. */
enum { DRFE_INIT_MAX_KEYS = 4096, DRFE_INIT_MAX_ITERATIONS = 300, DRFE_INIT_MAX_SOLVERS = 65535 };
enum { DRFE_INIT_MAX_ROWS = 1048576, DRFE_INIT_MAX_MASK_WORDS = 16777216 };
/* branch[s] */
enum { DRFE_INIT_BRANCH_NONE = 0, DRFE_INIT_BRANCH_H = 1, DRFE_INIT_BRANCH_F = 2 };
/* flags[s] */
enum { DRFE_INIT_TOO_FEW = 1, DRFE_INIT_NO_MODEL = 2, DRFE_INIT_H_DEGENERATE = 4 /* ReconstructH left at d1/d2, d2/d3 */ };
/* motion_status[s][m] */
enum { DRFE_INIT_MOTION_NAN_COS = 1 };
/* solvers in a call from which Planar_SLAM::Initializer uses the device entry.  The crossover has not been measured on an MI355X
 * yet, so it is INT32_MAX: the adaptor stays on the host entry unless its caller says UseDevice(true). */
enum { DRFE_INIT_DEVICE_FROM = 2147483647 };
typedef struct drfe_init_problems {
    int32_t n;                   /* solvers */
    int32_t pad;
    const float* K;              /* n x 9: mK, row-major CV_32F */
    const float* sigma;          /* n: the constructor's sigma (the reference passes 1.0) */
    const int32_t* max_iterations; /* n: 0 .. DRFE_INIT_MAX_ITERATIONS (the reference passes 200) */
    const uint32_t* seed;        /* n */
    const int32_t* key1_offsets; /* n + 1: solver s's reference keys are [key1_offsets[s], key1_offsets[s + 1]); [0] == 0 */
    const int32_t* key2_offsets; /* n + 1: its current frame's keys */
    const float* keys1;          /* 2 per reference key: mvKeysUn[i].pt */
    const float* keys2;          /* 2 per current key */
    const int32_t* matches12;    /* per reference key: -1 or an index into the solver's current keys */
} drfe_init_problems;
/* Every pointer is required.  Solver s owns the rows [row0(s), row0(s) + max_iterations[s]), row0 the prefix sum; its masks
 * start at word mask0(s), the prefix sum of max_iterations[s] * words(s), words(s) = ceil(N(s) / 64), row h at mask0(s) + h *
 * words(s), match i in bit i % 64 of word i / 64 (the layout of drfe_sim3_out.mask).  Rows from hypotheses[s] on are zero.
 * Motion hypothesis m of solver s is entry 8 s + m; its per-key arrays start at 8 * key1_offsets[s] + m * nKeys1(s).
 * Every NaN stored is the quiet NaN 0x7FC00000. */
typedef struct drfe_init_out {
    int32_t* N;                  /* n: matches */
    int32_t* iterations;         /* n: mMaxIterations */
    int32_t* hypotheses;         /* n: rows filled: iterations[s], or 0 when N < 8 */
    float* SH;                   /* n */
    float* SF;                   /* n */
    float* RH;                   /* n: SH / (SH + SF) */
    int32_t* branch;             /* n: DRFE_INIT_BRANCH_* */
    int32_t* motions;            /* n: 8, 4, or 0 */
    int32_t* ok;                 /* n: Initialize's return value */
    int32_t* flags;              /* n: DRFE_INIT_TOO_FEW | .. */
    float* R21;                  /* n x 9; zero unless ok */
    float* t21;                  /* n x 3 */
    float* vP3D;                 /* 3 per reference key, at key1_offsets; zero unless ok */
    uint8_t* vbTriangulated;     /* per reference key */
    int32_t* sample;             /* rows x 8: the sampled matches in draw order */
    float* H21;                  /* rows x 9: H21i */
    float* F21;                  /* rows x 9: F21i */
    float* score_h;              /* rows: currentScore of CheckHomography */
    float* score_f;              /* rows: of CheckFundamental */
    int32_t* best_h;             /* rows */
    int32_t* best_f;             /* rows */
    uint64_t* mask_h;            /* vbCurrentInliers of CheckHomography */
    uint64_t* mask_f;            /* of CheckFundamental */
    float* motion_R;             /* n x 8 x 9 */
    float* motion_t;             /* n x 8 x 3 */
    int32_t* motion_good;        /* n x 8: nGood */
    float* motion_cos;           /* n x 8: vCosParallax[min(50, size - 1)] after the sort, -0 as +0; 0 when nGood == 0 */
    float* motion_parallax;      /* n x 8 */
    int32_t* motion_status;      /* n x 8: DRFE_INIT_MOTION_* */
    uint8_t* motion_vbGood;      /* 8 per reference key: vbGood as CheckRT leaves it */
    float* motion_vP3D;          /* 8 x 3 per reference key: vP3D as CheckRT leaves it (written for a point CheckRT counts, also one
                                    with cosParallax >= 0.99998 whose vbGood stays false) */
} drfe_init_out;
/* On the host, no context. */
int drfe_init_ransac_host(const drfe_init_problems* problems, drfe_init_out* out);
/* The same on the device: the inputs staged with one copy, five launches, the results back with one copy; returns with the
 * outputs written (`stream` NULL = the context's).  Same bits as the host entry. */
int drfe_init_ransac_batch(drfe_ctx* ctx, const drfe_init_problems* problems, drfe_init_out* out, void* stream);
/* Counters since the context was created: stats[0] batch calls, [1] solvers, [2] rows, [3] matches, [4] solvers that took the
 * homography branch, [5] the fundamental branch, [6] solvers with ok, [7] solvers without a row. */
int drfe_init_stats(drfe_ctx* ctx, int64_t* stats /* 8 */);

/* Optimizer::PoseOptimization(Frame*, bool bStruct) (src/Optimizer.cc:601-1338), the motion-only optimisation between two
 * matchers of every Track* function and after PnP in Relocalization: every frame of a call at once.  DESIGN.md section 20.
 *
 * A frame is its pose mTcw, its intrinsics, mbf, and its matched features compacted in index order: the key points with a map
 * point (uRight < 0: monocular edge, else stereo), the key lines with a map line (two edges, start then end), the plane slots.
 * The four rounds of Levenberg-Marquardt, the classification after each, and what g2o and Eigen run under them are restated;
 * parity with a g2o / Eigen 3.3.7 build is not pinned yet.
 * A plane slot is a detected plane of the frame with up to three map planes: the matched one (EdgePlaneOnlyPose) and, read only
 * with bStruct, a parallel and a vertical one (EdgeParallelPlaneOnlyPose, EdgeVerticalPlaneOnlyPose).
 * Caps: DRFE_POSE_OPT_MAX_FRAMES frames per call, DRFE_POSE_OPT_MAX_POINTS points, DRFE_POSE_OPT_MAX_LINES lines and
 * DRFE_POSE_OPT_MAX_PLANES plane slots per frame; above them the call is refused (DRFE_ERR_INVALID), as are decreasing offsets. */
enum { DRFE_POSE_OPT_MAX_FRAMES = 4096, DRFE_POSE_OPT_MAX_POINTS = 8192, DRFE_POSE_OPT_MAX_LINES = 1024,
       DRFE_POSE_OPT_MAX_PLANES = 64 };
/* frames in a call from which drfe::PoseOptBatch uses the device entry (the measured crossover) */
enum { DRFE_POSEOPT_DEVICE_FROM = 64 };
/* plane_mask[slot] */
enum { DRFE_POSE_OPT_PLANE_MATCHED = 1, DRFE_POSE_OPT_PLANE_PARALLEL = 2, DRFE_POSE_OPT_PLANE_VERTICAL = 4 };
typedef struct drfe_pose_opt_problems {
    int32_t n;                   /* frames */
    int32_t pad;
    const float* Tcw;            /* n x 16: pFrame->mTcw, row-major */
    const float* K;              /* n x 4: fx, fy, cx, cy */
    const float* bf;             /* n: mbf */
    const uint8_t* b_struct;     /* n: bStruct */
    const int32_t* point_offsets; /* n + 1: frame f's points are [point_offsets[f], point_offsets[f + 1]); [0] == 0 */
    const float* obs;            /* 2 per point: mvKeysUn[i].pt */
    const float* u_right;        /* per point: mvuRight[i]; below 0 the point is monocular */
    const float* inv_sigma2;     /* per point: mvInvLevelSigma2[kpUn.octave] */
    const float* Xw;             /* 3 per point: pMP->GetWorldPos() */
    const int32_t* line_offsets; /* n + 1 */
    const double* line_fn;       /* 3 per line: mvKeyLineFunctions[i] */
    const double* line_ends;     /* 6 per line: pML->mWorldPos, start then end */
    const int32_t* plane_offsets; /* n + 1 */
    const float* plane_meas;     /* 4 per slot: mvPlaneCoefficients[i] */
    const float* plane_world;    /* 12 per slot: GetWorldPos() of the matched, the parallel and the vertical map plane */
    const uint8_t* plane_mask;   /* per slot: DRFE_POSE_OPT_PLANE_* of the map planes present */
    double plane_settings[7];    /* Plane.AngleInfo, DistanceInfo, ParallelInfo, VerticalInfo, Chi, VPChi, reserved (0) */
} drfe_pose_opt_problems;
/* The three offset tables are required; an array may be NULL when no frame has an element of it.  diag may be NULL. */
typedef struct drfe_pose_opt_out {
    float* Tcw;                  /* n x 16: the pose SetPose receives; the input pose when the call returns 0 before the loop */
    int32_t* returns;            /* n: nInitialCorrespondences - nBad, or 0 with fewer than 3 correspondences */
    int32_t* rounds;             /* n: rounds of the outer loop run (0 .. 4) */
    int32_t* iterations;         /* n: Levenberg iterations over all rounds */
    int32_t* trials;             /* n: trial steps (linear solves) over all rounds */
    int32_t* diag;               /* n x 8: [0] rejected trials, [1] rounds whose last trial was rejected, [2] rounds stopped by
                                    _nBad >= 3, [3] updates with theta < 1e-5, [4] with theta >= 1e-5, [5] rounds without an
                                    active edge, [6] [7] 0 */
    uint8_t* point_outlier;      /* per point: mvbOutlier */
    uint8_t* line_outlier;       /* per line: mvbLineOutlier */
    uint8_t* plane_outlier;      /* per slot: mvbPlaneOutlier */
    uint8_t* par_plane_outlier;  /* per slot: mvbParPlaneOutlier */
    uint8_t* ver_plane_outlier;  /* per slot: mvbVerPlaneOutlier */
} drfe_pose_opt_out;
/* On the host, no context. */
int drfe_pose_opt_host(const drfe_pose_opt_problems* problems, drfe_pose_opt_out* out);
/* The same on the device: the inputs staged with one copy, one launch (a workgroup per frame runs its four rounds), the results
 * back with one copy; returns with the outputs written (`stream` NULL = the context's).  Same bits as the host entry. */
int drfe_pose_opt_batch(drfe_ctx* ctx, const drfe_pose_opt_problems* problems, drfe_pose_opt_out* out, void* stream);
/* Counters since the context was created: stats[0] batch calls, [1] frames, [2] point edges, [3] line and plane edges, [4] Levenberg
 * iterations, [5] trial steps, [6] frames the device could not certify (sin / cos, atan2, x^3) and the host finished, [7] frames that
 * returned before the loop (fewer than 3 correspondences). */
int drfe_pose_opt_stats(drfe_ctx* ctx, int64_t* stats /* 8 */);

/* Optimizer::TranslationOptimization(Frame*, bool bStruct) (src/Optimizer.cc:3211-3980), the step of the decoupled mode after the
 * Manhattan rotation is written into mTcw (TranslationWithMotionModel, TranslationEstimation): only the translation is optimised.
 * Every frame of a call at once.  DESIGN.md section 21.
 *
 * The records, the caps and the diagnostics are drfe_pose_opt's.  Xw, line_ends and plane_world stay in world coordinates: the
 * entry rotates them once by the float R_cw of the input Tcw, as the reference does.  What differs from PoseOptimization: the
 * edges read only the estimate's translation; `returns` is the number of points less the point and plane outliers of the last
 * round (lines and planes do not add to it, line outliers do not take from it, so it can be negative); a frame with fewer than
 * three points returns 0 with its input pose after zero rounds, whatever its lines and planes.  Parity with a g2o / Eigen 3.3.7
 * build is not pinned yet. */
/* frames in a call from which drfe::TransOptBatch uses the device entry (the measured crossover) */
enum { DRFE_TRANSOPT_DEVICE_FROM = 64 };
/* On the host, no context. */
int drfe_trans_opt_host(const drfe_pose_opt_problems* problems, drfe_pose_opt_out* out);
/* The same on the device: the caller's arrays staged as they are with one copy, one launch (a workgroup per frame forms its
 * edges and runs its four rounds), the results back with one copy; returns with the outputs written (`stream` NULL = the
 * context's).  Same bits as the host entry. */
int drfe_trans_opt_batch(drfe_ctx* ctx, const drfe_pose_opt_problems* problems, drfe_pose_opt_out* out, void* stream);
/* Counters since the context was created: stats[0] batch calls, [1] frames, [2] point edges, [3] line and plane edges (no plane
 * edge exists in a frame that returns before the loop), [4] Levenberg iterations, [5] trial steps, [6] frames the device handed
 * back to the host (a sin / cos, atan2 or x^3 it could not certify, or a term of H or b that is not finite), [7] frames that
 * returned before the loop (fewer than 3 points). */
int drfe_trans_opt_stats(drfe_ctx* ctx, int64_t* stats /* 8 */);

/* Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:3982-4177), the fourth of the five
 * steps LoopClosing::ComputeSim3 runs per loop candidate, between SearchBySim3 and SearchByProjection(KF, Scw): every problem of a
 * call at once.  DESIGN.md section 22.
 *
 * A problem is the Sim3 estimate, the two key frames' intrinsics and poses, th2, bFixScale and its kept matches in index order:
 * the caller leaves out a match whose vpMatches1[i] is NULL, whose map point of either side is NULL or bad, or whose i2 is below 0,
 * as the reference's `continue`s do.  The two optimize() calls, the two classifications, the numeric Jacobians and what g2o and
 * Eigen run under them are restated; parity with a g2o / Eigen 3.3.7 build is not pinned yet.
 * Caps: DRFE_SIM3_OPT_MAX_PROBLEMS problems per call, DRFE_SIM3_OPT_MAX_MATCHES kept matches per problem; above them the call is
 * refused (DRFE_ERR_INVALID), as are decreasing offsets. */
enum { DRFE_SIM3_OPT_MAX_PROBLEMS = 1024, DRFE_SIM3_OPT_MAX_MATCHES = 8192 };
/* problems in a call from which drfe::Sim3OptBatch uses the device entry (the measured crossover) */
enum { DRFE_SIM3OPT_DEVICE_FROM = 8 };
typedef struct drfe_sim3_opt_problems {
    int32_t n;                   /* problems */
    int32_t pad;
    const double* S12;           /* n x 8: g2oS12 as rotation().coeffs() (x y z w), translation(), scale() */
    const float* K1;             /* n x 4: fx, fy, cx, cy of pKF1->mK */
    const float* K2;             /* n x 4: of pKF2->mK */
    const float* R1w;            /* n x 9: pKF1->GetRotation(), row-major */
    const float* t1w;            /* n x 3: pKF1->GetTranslation() */
    const float* R2w;            /* n x 9 */
    const float* t2w;            /* n x 3 */
    const float* th2;            /* n */
    const uint8_t* fix_scale;    /* n: bFixScale */
    const int32_t* match_offsets; /* n + 1: problem p's matches are [match_offsets[p], match_offsets[p + 1]); [0] == 0 */
    const int32_t* index;        /* per match: i, increasing within a problem; the entry only checks it.  May be NULL */
    const float* P3D1w;          /* 3 per match: vpMapPoints1[i]->GetWorldPos() */
    const float* P3D2w;          /* 3 per match: vpMatches1[i]->GetWorldPos() */
    const float* obs1;           /* 2 per match: pKF1->mvKeysUn[i].pt */
    const float* obs2;           /* 2 per match: pKF2->mvKeysUn[i2].pt */
    const float* inv_sigma2_1;   /* per match: pKF1->mvInvLevelSigma2[kpUn1.octave] */
    const float* inv_sigma2_2;   /* per match: pKF2->mvInvLevelSigma2[kpUn2.octave] */
} drfe_sim3_opt_problems;
/* The per-match arrays may be NULL when no problem has a match.  diag may be NULL. */
typedef struct drfe_sim3_opt_out {
    double* S12;                 /* n x 8: g2oS12 after the call; the input's bits when the call returns before the second optimize() */
    float* T12;                  /* n x 16: Converter::toCvMat(g2oS12) of that estimate */
    float* Scw;                  /* n x 16: Converter::toCvMat(g2oS12 * g2o::Sim3(toMatrix3d(R2w), toVector3d(t2w), 1.0)), mScw of
                                    src/LoopClosing.cc:379-381 */
    int32_t* returns;            /* n: nIn, or 0 when fewer than 10 matches are left after the first classification */
    int32_t* n_bad;              /* n: nBad of the first classification */
    int32_t* iterations;         /* n x 2: Levenberg iterations of the first and the second optimize() */
    int32_t* trials;             /* n x 2: trial steps (linear solves) of each */
    int32_t* diag;               /* n x 8: [0] rejected trials, [1] optimize() calls whose last trial was rejected (the classification
                                    after them reads the errors at the rejected estimate), [2] calls stopped by _nBad >= 3, [3] updates
                                    with theta < 1e-5, [4] with theta >= 1e-5, [5] 1 for the return before the second optimize(),
                                    [6] matches that the errors at the rejected estimate classified differently from the errors at the
                                    kept one, [7] 0 */
    uint8_t* outlier;            /* per match: vpMatches1[i] was set to NULL by either classification */
} drfe_sim3_opt_out;
/* On the host, no context. */
int drfe_sim3_opt_host(const drfe_sim3_opt_problems* problems, drfe_sim3_opt_out* out);
/* The same on the device: the inputs staged with one copy, one launch (a workgroup per problem runs both optimize() calls and both
 * classifications), the results back with one copy; returns with the outputs written (`stream` NULL = the context's).  A problem
 * with a free scale needs exp, which has no certified form on the device: the host core runs it inside the same call while the
 * launch is in flight.  Same bits as the host entry.  For a free scale both entries use the host libm's exp: their bits agree with
 * each other, and depend on that libm in the last place where its exp is not the correctly rounded one. */
int drfe_sim3_opt_batch(drfe_ctx* ctx, const drfe_sim3_opt_problems* problems, drfe_sim3_opt_out* out, void* stream);
/* Counters since the context was created: stats[0] batch calls, [1] problems, [2] kept matches, [3] problems with a free scale, run
 * by the host core, [4] Levenberg iterations, [5] trial steps, [6] fixed-scale problems the device could not certify (sin / cos,
 * x^3) and the host finished, [7] problems that returned before the second optimize(). */
int drfe_sim3_opt_stats(drfe_ctx* ctx, int64_t* stats /* 8 */);

/* KeyFrameDatabase (src/KeyFrameDatabase.cc:40-309) with DBoW2's L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68)
 * and the minScore loop of LoopClosing::DetectLoop (src/LoopClosing.cc:137-151): the candidate lists that ComputeSim3 and
 * Relocalization start from, every query of a call at once.  DESIGN.md section 23.
 *
 * A drfe_kfdb is an object of its own.  Created with a context it runs calls of DRFE_KFDB_DEVICE_FROM queries or more on that
 * context's device (the context must outlive it); created with NULL it is host-only.  It owns a mutex that every entry takes, as
 * the reference's mMutex: Tracking and LoopClosing may both call in.  A key frame is known by the caller's handle (>= 0; the
 * adaptor uses mnId).  Its life: put (the BowVector is stored; queries do not see it yet, but a loop query can name it as the
 * query, as connected or as covisible) -> add (in the inverted file, visible) -> erase (stored, not visible) -> remove (forgotten;
 * implies erase).  put of a stored handle, add of a visible one, erase of one that is not visible and any unknown handle are
 * refused (DRFE_ERR_INVALID), and the refused call changes nothing.
 *
 * Kept from the reference: the order of the listed key frames (ascending word of the query, each word's list in order of the
 * latest add); a connected key frame is never listed and never counts as a neighbour; minCommonWords = (int)(maxCommonWords * 0.8f);
 * mLoopScore is stored below minScore too; the float accumulation over GetBestCovisibilityKeyFrames(10) in neighbour order; strict
 * > for the best key frame, for bestAccScore and for the retain threshold; duplicates dropped at their first occurrence; the
 * relocalisation query's neighbour test (shares a word) and with it its state: a neighbour that was not scored by this query adds
 * the mRelocScore an earlier query left in it.  The reference never initialises that member: here a never-written one reads as
 * 0.0f and the read is counted (uninit_reads).  Only L1 scoring exists; another scoring type is refused (DRFE_ERR_INVALID).
 * Query ids: per kind (loop, relocalisation) nonzero and strictly greater than the last id used on this database, else
 * DRFE_ERR_INVALID.  Parity with a DBoW2 build is not pinned. */
typedef struct drfe_kfdb drfe_kfdb;
/* DBoW2::ScoringType, in its order */
enum { DRFE_KFDB_L1_NORM = 0, DRFE_KFDB_L2_NORM, DRFE_KFDB_CHI_SQUARE, DRFE_KFDB_KL, DRFE_KFDB_BHATTACHARYYA, DRFE_KFDB_DOT_PRODUCT };
/* Caps: DRFE_KFDB_MAX_QUERIES queries per call (DRFE_ERR_INVALID above); a device call of more than 2^26 (query, stored key frame)
 * pairs is refused with DRFE_ERR_CAPACITY by the _device forms and run on the host by the _batch forms. */
enum { DRFE_KFDB_NEIGHBOURS = 10, DRFE_KFDB_MAX_QUERIES = 4096 };
/* queries in a call from which the _batch entries of a database with a context use the device (the measured crossover, DESIGN.md
 * section 23, profiles/kfdb_timing.jsonl) */
enum { DRFE_KFDB_DEVICE_FROM = 16 };
int drfe_kfdb_create(drfe_ctx* ctx /* or NULL */, int scoring, drfe_kfdb** out);
void drfe_kfdb_destroy(drfe_kfdb* db);
/* the reason of the last failed call on this database (valid until its next call) */
const char* drfe_kfdb_last_error(const drfe_kfdb* db);
/* mBowVec of a key frame: n ascending word ids and their values, as drfe_bow_download and the host fold leave them */
int drfe_kfdb_put(drfe_kfdb* db, int32_t handle, int32_t n, const int32_t* word_ids, const double* values);
/* KeyFrameDatabase::add / erase / clear (clear empties the inverted file: every key frame stays stored, none is visible) */
int drfe_kfdb_add(drfe_kfdb* db, int32_t handle);
int drfe_kfdb_erase(drfe_kfdb* db, int32_t handle);
int drfe_kfdb_clear(drfe_kfdb* db);
/* a culled key frame: its vector, neighbours and mRelocScore are dropped, the handle is free again */
int drfe_kfdb_remove(drfe_kfdb* db, int32_t handle);
/* GetBestCovisibilityKeyFrames(10) of `count` key frames: nbr is count x 10 handles in the reference's order, padded with -1.  A row
 * replaces that key frame's earlier one.  A handle that has been removed by the time of a query is skipped there. */
int drfe_kfdb_set_neighbours(drfe_kfdb* db, int32_t count, const int32_t* handles, const int32_t* nbr);
/* out2[0] stored key frames, out2[1] visible ones.  n x (visible + n) candidates always suffice for a call of n queries. */
int drfe_kfdb_size(drfe_kfdb* db, int32_t* out2);

typedef struct drfe_kfdb_loop_queries {
    int32_t n;                        /* queries; query k + 1 behaves as if run after query k */
    int32_t pad;
    const int32_t* handle;            /* n: the query key frame (stored; usually not visible yet) */
    const int64_t* id;                /* n: pKF->mnId */
    const int32_t* connected_offsets; /* n + 1, [0] == 0 */
    const int32_t* connected;         /* handles of GetConnectedKeyFrames() */
    const float* min_score;           /* n, or NULL: computed from `covisible` as src/LoopClosing.cc:139-151, from 1.0f */
    const int32_t* covisible_offsets; /* n + 1 (read when min_score is NULL) */
    const int32_t* covisible;         /* handles of GetVectorCovisibleKeyFrames() in its order, bad ones left out */
    const uint8_t* add_after;         /* n, or NULL: nonzero = KeyFrameDatabase::add(query key frame) after its query, before the next */
} drfe_kfdb_loop_queries;
typedef struct drfe_kfdb_reloc_queries {
    int32_t n;                        /* queries, as if run one after another in array order */
    int32_t pad;
    const int64_t* id;                /* n: F->mnId */
    const int32_t* word_offsets;      /* n + 1, [0] == 0: F->mBowVec of query k is [word_offsets[k], word_offsets[k + 1]) */
    const int32_t* word_ids;          /* ascending within a query */
    const double* values;
} drfe_kfdb_reloc_queries;
typedef struct drfe_kfdb_out {
    int32_t cand_capacity;            /* of candidates; DRFE_ERR_CAPACITY when the call needs more (the call then changes nothing) */
    int32_t pad;
    int32_t* cand_offsets;            /* n + 1 */
    int32_t* candidates;              /* handles, per query in the reference's order */
    int32_t* record;                  /* n x 4: key frames listed (lKFsSharingWords), scored (nscores), kept (lScoreAndMatch), and
                                         maxCommonWords */
    float* min_score;                 /* n: the minScore used (loop queries; may be NULL) */
    int32_t* uninit_reads;            /* n: reads of an mRelocScore no query has written (relocalisation queries; may be NULL) */
} drfe_kfdb_out;
/* KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates of every query.  A database with a context runs a call
 * of DRFE_KFDB_DEVICE_FROM queries or more on the device: what put / add / erase / remove / set_neighbours changed since the last
 * device call is sent first, then the call's queries go up in one copy, all of them run in one launch sequence with no host
 * round trip between the stages, and the results return in two copies (the records and offsets, then exactly the candidates).
 * The _host forms always run on the host, the _device forms always on the device (DRFE_ERR_STATE without a context).  All three
 * return the same bytes and leave the same state.  `stream` NULL = the context's. */
int drfe_kfdb_loop_queries_host(drfe_kfdb* db, const drfe_kfdb_loop_queries* q, drfe_kfdb_out* out);
int drfe_kfdb_loop_queries_device(drfe_kfdb* db, const drfe_kfdb_loop_queries* q, drfe_kfdb_out* out, void* stream);
int drfe_kfdb_loop_queries_batch(drfe_kfdb* db, const drfe_kfdb_loop_queries* q, drfe_kfdb_out* out, void* stream);
int drfe_kfdb_reloc_queries_host(drfe_kfdb* db, const drfe_kfdb_reloc_queries* q, drfe_kfdb_out* out);
int drfe_kfdb_reloc_queries_device(drfe_kfdb* db, const drfe_kfdb_reloc_queries* q, drfe_kfdb_out* out, void* stream);
int drfe_kfdb_reloc_queries_batch(drfe_kfdb* db, const drfe_kfdb_reloc_queries* q, drfe_kfdb_out* out, void* stream);
/* TemplatedVocabulary::score(a, b) of two vectors (L1): (float)L1Scoring::score.  Host code, no database. */
int drfe_kfdb_score(int32_t na, const int32_t* ids_a, const double* values_a, int32_t nb, const int32_t* ids_b, const double* values_b,
                    float* score);
/* Counters since the database was created: stats[0] loop calls, [1] loop queries, [2] relocalisation calls, [3] relocalisation
 * queries, [4] calls run on the device, [5] uploads of the database image, [6] candidates returned, [7] uninitialised mRelocScore
 * reads. */
int drfe_kfdb_stats(drfe_kfdb* db, int64_t* stats /* 8 */);

/* Tracking::UpdateLocalMap (src/Tracking.cc:3383-3541): UpdateLocalKeyFrames, UpdateLocalPoints and UpdateLocalLines of every frame
 * of a call at once, the step of TrackLocalMap in front of drfe_frame_is_in_frustum, the map projection searches and
 * drfe_pose_opt_batch.  DESIGN.md section 25.
 *
 * A drfe_lmap is an object of its own, like a drfe_kfdb: created with a context (which must outlive it) it can run calls on that
 * context's device, created with NULL it is host-only; it owns a mutex that every entry takes.  It stores the part of the map
 * graph that the three functions read.  Per key frame: rank (the reference walks map<KeyFrame*, int> and set<KeyFrame*> in pointer
 * order; rank is that order, distinct within a store; the adaptor passes the pointer value), bad, parent, the 10 handles of
 * GetBestCovisibilityKeyFrames(10), the children (ordered by rank by the store), mvpMapPoints and mvpMapLines as handles by
 * keypoint index.  Per map point: bad and the key frames of GetObservations().  Per map line: bad.  Handles are the caller's
 * (>= 0, one space per kind; the adaptor uses mnId), -1 is null.  A set_* may name handles that are not stored yet; a query on a
 * store in which an observation, neighbour, child, parent or match names an unknown handle fails with DRFE_ERR_STATE, its message
 * names the reference, and it changes nothing.
 *
 * Kept from the reference: a bad frame point does not vote and is reported as nulled; a point that is in the frame twice votes
 * twice; bad key frames count in keyframeCounter but are never listed and never pKFmax; pKFmax by strict > in rank order from
 * max = 0; an empty counter returns early (the list stays prev_kfs, ref_kf -1, the gathers still run on it); the expansion walks
 * only the key frames the vote listed, tests size() > 80 at the top of each iteration, takes per key frame the first neighbour
 * that is neither bad nor listed, the first such child in rank order, then the parent (no bad test), and the parent's break ends
 * the whole expansion; the gathers walk the list in order, bad key frames included, matches in index order, skip null, listed and
 * bad items, and list an item where it is first met.  Parity with a build of the reference's Tracking.cc is not pinned. */
typedef struct drfe_lmap drfe_lmap;
enum { DRFE_LMAP_NEIGHBOURS = 10, DRFE_LMAP_MAX_QUERIES = 4096 };
enum { DRFE_LMAP_KEYFRAME = 0, DRFE_LMAP_POINT = 1, DRFE_LMAP_LINE = 2 };
/* queries in a call from which drfe_lmap_update_batch of a store with a context uses the device (the measured crossover, DESIGN.md
 * section 25, profiles/lmap_timing.jsonl: a call of one query loses to the host on a store of 100 key frames) */
enum { DRFE_LMAP_DEVICE_FROM = 4 };
int drfe_lmap_create(drfe_ctx* ctx /* or NULL */, drfe_lmap** out);
void drfe_lmap_destroy(drfe_lmap* db);
const char* drfe_lmap_last_error(const drfe_lmap* db);
/* bytes of device scratch a call may use (> 0; the default is 1 GiB).  A call that needs more runs in chunks of queries; when
 * one query does not fit, _device refuses with DRFE_ERR_CAPACITY and _batch runs the call on the host. */
int drfe_lmap_configure(drfe_lmap* db, int64_t scratch_bytes);
/* out[0] stored key frames up to which the vote's histogram is in LDS, [1] workgroup size of the vote, [2] entries of a key frame's
 * match row that one pass of a gather workgroup takes, [3] DRFE_LMAP_DEVICE_FROM */
int drfe_lmap_limits(int32_t* out4);
typedef struct drfe_lmap_keyframes {
    int32_t count;                    /* rows; a row replaces the stored one of its handle (the last row of a handle wins) */
    int32_t pad;
    const int32_t* handle;            /* count */
    const uint64_t* rank;             /* count */
    const uint8_t* bad;               /* count */
    const int32_t* parent;            /* count: handle or -1 */
    const int32_t* neighbours;        /* count x 10 handles in the reference's order, padded with -1 */
    const int32_t* child_offsets;     /* count + 1, [0] == 0 */
    const int32_t* children;          /* handles, in any order */
    const int32_t* point_offsets;     /* count + 1: mvpMapPoints by keypoint index, -1 = null */
    const int32_t* points;
    const int32_t* line_offsets;      /* count + 1: mvpMapLines */
    const int32_t* lines;
} drfe_lmap_keyframes;
int drfe_lmap_set_keyframes(drfe_lmap* db, const drfe_lmap_keyframes* rows);
/* map points: bad and the key-frame handles of GetObservations() (a duplicate within a row is refused) */
int drfe_lmap_set_points(drfe_lmap* db, int32_t count, const int32_t* handles, const uint8_t* bad, const int32_t* obs_offsets,
                         const int32_t* obs);
int drfe_lmap_set_lines(drfe_lmap* db, int32_t count, const int32_t* handles, const uint8_t* bad);
/* the cheap edit: the bad flags of stored items of one kind (an unknown handle: DRFE_ERR_INVALID, nothing changed) */
int drfe_lmap_set_bad(drfe_lmap* db, int kind, int32_t count, const int32_t* handles, const uint8_t* flags);
int drfe_lmap_remove(drfe_lmap* db, int kind, int32_t handle);
/* out3: stored key frames, map points, map lines.  For a call of n queries, n x key frames + all prev_kfs entries, n x map
 * points, n x map lines and all frame points always suffice as kf / mp / ml / nulled capacities. */
int drfe_lmap_size(drfe_lmap* db, int32_t* out3);

typedef struct drfe_lmap_queries {
    int32_t n;                        /* frames; each behaves as the reference's UpdateLocalMap of that frame on this graph */
    int32_t pad;
    const int64_t* frame_id;          /* n: mCurrentFrame.mnId; nonzero and strictly greater than the last id used on this store */
    const int32_t* point_offsets;     /* n + 1, [0] == 0 */
    const int32_t* points;            /* mCurrentFrame.mvpMapPoints by keypoint index, -1 = null */
    const int32_t* line_offsets;      /* n + 1 or NULL: mCurrentFrame.mvpMapLines, read only for ml_in_frame */
    const int32_t* lines;
    const int32_t* prev_kf_offsets;   /* n + 1 or NULL: mvpLocalKeyFrames as the previous frame left it */
    const int32_t* prev_kfs;
} drfe_lmap_queries;
typedef struct drfe_lmap_out {
    int32_t kf_capacity, mp_capacity, ml_capacity, nulled_capacity;   /* DRFE_ERR_CAPACITY when one is too small; nothing changes */
    int32_t* kf_offsets;              /* n + 1 */
    int32_t* kfs;                     /* mvpLocalKeyFrames, in the reference's order */
    int32_t* ref_kf;                  /* n: pKFmax, or -1 = mpReferenceKF unchanged */
    int32_t* mp_offsets;              /* n + 1 */
    int32_t* mps;                     /* mvpLocalMapPoints */
    uint8_t* mp_in_frame;             /* per local point: 1 = one of the frame's remaining map points (the ones the first loop of
                                         SearchLocalPoints, src/Tracking.cc:3278-3290, stamps with mnLastFrameSeen) */
    int32_t* ml_offsets;              /* n + 1 */
    int32_t* mls;                     /* mvpLocalMapLines */
    uint8_t* ml_in_frame;
    int32_t* nulled_offsets;          /* n + 1 */
    int32_t* nulled;                  /* keypoint indices whose map point was bad (set to NULL at src/Tracking.cc:3459), ascending */
    int32_t* record;                  /* n x 4: size of keyframeCounter, local key frames after the vote loop, key frames added by
                                         the expansion loop, votes of pKFmax */
} drfe_lmap_out;
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context), _batch on the device from
 * DRFE_LMAP_DEVICE_FROM queries.  All three return the same bytes.  What the setters changed since the last device call is sent
 * before the next one (counted in stats[3]); then one staging block goes up, the offsets and records come back, then exactly
 * the lists.  `stream` NULL = the context's. */
int drfe_lmap_update_host(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* out);
int drfe_lmap_update_device(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* out, void* stream);
int drfe_lmap_update_batch(drfe_lmap* db, const drfe_lmap_queries* q, drfe_lmap_out* out, void* stream);
/* Counters since the store was created: stats[0] calls, [1] queries, [2] calls run on the device, [3] uploads of the image,
 * [4] local key frames returned, [5] local points returned, [6] local lines returned, [7] frame points nulled. */
int drfe_lmap_stats(drfe_lmap* db, int64_t* stats /* 8 */);

/* KeyFrame::UpdateConnections (src/KeyFrame.cc:366-500, with AddConnection :200-213 and UpdateBestCovisibles :215-234) of every
 * key frame of a call, on the same store.  DESIGN.md section 26.
 *
 * Per key frame the store holds, besides the rows above, its connection state: first_connection (the caller passes
 * mbFirstConnection && mnId != 0), the weights row (mConnectedKeyFrameWeights as (handle, weight) pairs, in any order, a handle
 * once, weight > 0) and the ordered row (mvpOrderedConnectedKeyFrames with mvOrderedWeights, in the reference's order; the store
 * keeps it as given, because the reference's list cannot be derived from the weights).  A key frame without it has empty rows and
 * first_connection 0.  drfe_lmap_set_keyframes on a stored handle leaves it alone; drfe_lmap_remove drops it.  An entry that names
 * an unknown key frame fails the next query with DRFE_ERR_STATE, like every other reference.
 *
 * A call names key frames s_0 .. s_{n-1} (at most DRFE_LMAP_MAX_QUERIES), each once (a handle named twice: DRFE_ERR_INVALID), and
 * gives what the reference's calls made one after another in that order give.  Kept from the reference: an entry of mvpMapPoints that is neither null nor bad adds
 * a vote to every key frame of its observations but the one whose handle is the called one's; a point that is in the row twice
 * votes twice; bad key frames are counted, connected and become parents like any other; lines and planes do not vote; an empty
 * counter changes nothing of the called key frame; pKFmax by strict > in rank order from nmax = 0; every counter entry of at least
 * DRFE_LMAP_CONNECT_TH votes is listed, or pKFmax alone when none is; each listed key frame gets AddConnection, which sets its
 * entry and re-sorts ALL of its weights when the entry was absent or different and does nothing otherwise; the called key frame's
 * weights become the whole counter, its ordered list the listed pairs only, by descending weight and among equal weights by
 * descending rank; with first_connection set its parent becomes the front of that list (no bad test), the parent gains it as a
 * child, the flag clears; nothing is ever erased from another key frame's rows. */
enum { DRFE_LMAP_CONNECT_TH = 15 };
/* key frames in a call from which drfe_lmap_connect_batch of a store with a context uses the device (the measured crossover,
 * DESIGN.md section 26, profiles/conn_timing.jsonl: calls of 1 and 4 key frames lose to the host at every measured store size) */
enum { DRFE_LMAP_CONNECT_DEVICE_FROM = 16 };
typedef struct drfe_lmap_connections {
    int32_t count;                    /* rows; a row replaces the stored connection state of its handle (the last row wins) */
    int32_t pad;
    const int32_t* handle;            /* count: stored or not yet stored key frames */
    const uint8_t* first_connection;  /* count */
    const int32_t* weight_offsets;    /* count + 1, [0] == 0 */
    const int32_t* weight_kfs;        /* key-frame handles, one mention per row */
    const int32_t* weight_w;          /* > 0 */
    const int32_t* ordered_offsets;   /* count + 1 */
    const int32_t* ordered_kfs;
    const int32_t* ordered_w;         /* > 0 */
} drfe_lmap_connections;
int drfe_lmap_set_connections(drfe_lmap* db, const drfe_lmap_connections* rows);
/* What drfe_lmap_get_connections and the connect entries fill per key frame.  Weights rows are in ascending rank. */
typedef struct drfe_lmap_conn_rows {
    int32_t weights_capacity, ordered_capacity;   /* entries; DRFE_ERR_CAPACITY when one is too small */
    int32_t* weight_offsets;          /* rows + 1 */
    int32_t* weight_kfs;
    int32_t* weight_w;
    int32_t* ordered_offsets;         /* rows + 1 */
    int32_t* ordered_kfs;
    int32_t* ordered_w;
    int32_t* parent;                  /* rows: handle or -1 */
    uint8_t* first_connection;        /* rows */
} drfe_lmap_conn_rows;
/* the stored state of `count` key frames (an unknown handle: DRFE_ERR_INVALID); `children_*` may be NULL, else the child lists in
 * ascending rank with their own capacity */
int drfe_lmap_get_connections(drfe_lmap* db, int32_t count, const int32_t* handles, drfe_lmap_conn_rows* out,
                              int32_t children_capacity, int32_t* children_offsets, int32_t* children);
typedef struct drfe_lmap_connect_out {
    int32_t counter_capacity, touched_capacity;   /* counter entries of the call; touched key frames */
    /* per called key frame */
    int32_t* counter_offsets;         /* n + 1 */
    int32_t* counter_kfs;             /* KFcounter in rank order: GetConnectedKeyFrames() right after its own call */
    int32_t* counter_votes;
    int32_t* record;                  /* n x 4: size of the counter, listed key frames after the fallback, nmax, pKFmax or -1 */
    int32_t* new_parent;              /* n: the parent the first connection set, or -1 */
    /* per touched key frame (called, or listed by a called one), in ascending rank */
    int32_t* n_touched;               /* 1 */
    int32_t* touched;                 /* touched_capacity handles */
    drfe_lmap_conn_rows rows;         /* the final state; its arrays hold touched_capacity (+ 1) rows */
    uint8_t* flags;                   /* touched_capacity: bit 0 the weights row, bit 1 the ordered row, bit 2 the parent differs
                                         from what was stored */
} drfe_lmap_connect_out;
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context; DRFE_ERR_CAPACITY when the call's
 * counters do not fit the configured scratch), _batch on the device from DRFE_LMAP_CONNECT_DEVICE_FROM key frames when the call
 * fits.  All three return the same bytes and leave the same store.  When a capacity is too small the call returns
 * DRFE_ERR_CAPACITY and nothing changes.  On success the call commits: the rows, parent and first_connection of every touched key
 * frame, its neighbours (the first 10 of its ordered row, padded with -1) when the ordered row changed, and the new parents' child
 * lists; the next drfe_lmap_update_* reads the new graph.  For a call of n key frames, n x (key frames - 1) counter entries and
 * min(key frames, n x key frames) touched rows always suffice; a touched row has at most key frames - 1 entries. */
int drfe_lmap_connect_host(drfe_lmap* db, int32_t n, const int32_t* handles, drfe_lmap_connect_out* out);
int drfe_lmap_connect_device(drfe_lmap* db, int32_t n, const int32_t* handles, drfe_lmap_connect_out* out, void* stream);
int drfe_lmap_connect_batch(drfe_lmap* db, int32_t n, const int32_t* handles, drfe_lmap_connect_out* out, void* stream);
/* out[0] DRFE_LMAP_CONNECT_TH, [1] DRFE_LMAP_CONNECT_DEVICE_FROM, [2] keys of one tile of the device's list sort, [3] workgroups of
 * the touched-row launch */
int drfe_lmap_connect_limits(int32_t* out4);
/* Counters since the store was created: stats[0] connect calls, [1] called key frames, [2] calls run on the device, [3] counter
 * entries returned, [4] listed key frames (AddConnection calls), [5] touched key frames returned, [6] first connections made,
 * [7] called key frames with an empty counter. */
int drfe_lmap_connect_stats(drfe_lmap* db, int64_t* stats /* 8 */);

/* LoopClosing::CorrectLoop's Sim3 propagation (src/LoopClosing.cc:480-562) on the same store: the corrected Sim3 of every key frame
 * connected to the current one, the correction of every map point they see, and the new key-frame poses.  DESIGN.md section 27.
 *
 * The geometry it reads is optional; a store without it behaves as before.  Per store: mnScaleLevels and mvScaleFactors.  Per key
 * frame: Tcw as SetPose last received it; Ow and Twc are derived as SetPose derives them.  Per map point: GetWorldPos(), the
 * reference key frame, ref_level (the octave of the reference key frame's key point, 0 when the reference key frame is not among
 * the observations, as in drfe_upkeep_items) and the stamps mnCorrectedByKF / mnCorrectedReference as handles (0 when not given,
 * as the reference's constructors leave them).  A setter row replaces the stored one, may name a handle that is not stored yet,
 * and is uploaded before the next device call; drfe_lmap_remove drops the geometry with the item. */
int drfe_lmap_set_scales(drfe_lmap* db, int32_t n_levels, const float* scale_factors);
/* *n_levels is set; the factors are written when capacity holds them (DRFE_ERR_CAPACITY otherwise) */
int drfe_lmap_get_scales(drfe_lmap* db, int32_t capacity, int32_t* n_levels, float* scale_factors);
int drfe_lmap_set_poses(drfe_lmap* db, int32_t count, const int32_t* handles, const float* Tcw /* 16 each, row-major */);
/* Tcw, Ow (3 each) and Twc (16 each) of key frames with a pose; each array may be NULL.  A handle without one: DRFE_ERR_INVALID */
int drfe_lmap_get_poses(drfe_lmap* db, int32_t count, const int32_t* handles, float* Tcw, float* Ow, float* Twc);
typedef struct drfe_lmap_point_geometry {
    int32_t count;                    /* rows; the last row of a handle wins */
    int32_t pad;
    const int32_t* handle;            /* count */
    const float* world;               /* 3 each */
    const int32_t* ref_kf;            /* count: key-frame handle */
    const int32_t* ref_level;         /* count */
    const int32_t* corrected_by;      /* count, or NULL = 0 */
    const int32_t* corrected_ref;     /* count, or NULL = 0 */
} drfe_lmap_point_geometry;
int drfe_lmap_set_point_geometry(drfe_lmap* db, const drfe_lmap_point_geometry* rows);
/* the stored rows; each array may be NULL.  A handle without geometry: DRFE_ERR_INVALID */
int drfe_lmap_get_point_geometry(drfe_lmap* db, int32_t count, const int32_t* handles, float* world, int32_t* ref_kf,
                                 int32_t* ref_level, int32_t* corrected_by, int32_t* corrected_ref);

/* A call names cur, the handle of mpCurrentKF; Scw = mg2oScw as double[8] (the quaternion's coeffs x y z w, t, s: the layout of
 * drfe_sim3_opt_problems::S12); and n handles, GetVectorCovisibleKeyFrames() plus the current key frame, in any order, each once
 * and cur among them (DRFE_ERR_INVALID otherwise; at most DRFE_LMAP_MAX_QUERIES).
 *
 * Kept from the reference.  The called key frames are processed in rank order, the iteration order of KeyFrameAndPose, whatever
 * order the caller passed.  Per key frame i: NonCorrected = Sim3(Quaterniond(Riw), tiw, 1); for i != cur Tic = Tiw * Twc_cur as a
 * float 4x4 product, Sic from it and Corrected = Sic * Scw; for cur Corrected = Scw as given; Swi = Corrected.inverse(); the new
 * pose is toCvSE3(r.toRotationMatrix(), t * (1. / s)).  Each key frame's match row is walked in index order: a null or bad entry
 * or one with corrected_by == cur is skipped (so with cur == 0 and untouched stamps no point moves), otherwise the point moves to
 * (float)Swi.map(Siw.map((double)X)) and its stamps become cur and i: a point is moved once, by the first (key frame, index) that
 * meets it.  UpdateNormalAndDepth of a moved point runs on the new position over its observations in stored order; an observing
 * or reference key frame counts with its corrected centre exactly when it is a called key frame strictly before the claimant in
 * rank order, with its stored centre otherwise - the claimant itself included, whose SetPose comes after its points.  A point
 * without observations still moves; its normal and distances are not computed (status 0, zeros).  Bad key frames are not tested
 * anywhere; map lines and planes are untouched.
 *
 * The integer graph is unchanged, so drfe_lmap_connect_* of the same handles afterwards gives what the reference's interleaved
 * UpdateConnections calls give, when the handles are passed to it in rank order (ascending walk_pos). */
typedef struct drfe_lmap_correct_out {
    int32_t points_capacity;          /* moved points; the total length of the called match rows always suffices */
    int32_t pad;
    /* per called key frame, in the caller's order */
    int32_t* walk_pos;                /* n: its position in rank order among the called */
    double* corrected;                /* n x 8: CorrectedSim3 */
    double* non_corrected;            /* n x 8: NonCorrectedSim3 */
    float* Tiw;                       /* n x 16: the pose SetPose receives */
    /* per moved point, in walk order */
    int32_t* n_points;                /* 1 */
    int32_t* points;                  /* handles */
    int32_t* claimed_by;              /* the key frame that moved it: mnCorrectedReference */
    float* world;                     /* 3 each: the new position */
    float* normal;                    /* 3 each */
    float* max_distance;
    float* min_distance;
    uint8_t* status;                  /* DRFE_UPKEEP_NORMAL when normal and distances were computed, else 0 */
} drfe_lmap_correct_out;
/* key frames in a call from which drfe_lmap_correct_batch of a store with a context uses the device (the measured crossover,
 * DESIGN.md section 27, profiles/loop_correct_timing.jsonl) */
enum { DRFE_LMAP_CORRECT_DEVICE_FROM = 16 };
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context; DRFE_ERR_CAPACITY when the
 * longest called row does not fit the configured scratch), _batch on the device from DRFE_LMAP_CORRECT_DEVICE_FROM key frames when
 * the call fits.  All three return the same bytes and leave the same store.  A refused call changes nothing: DRFE_ERR_STATE, with
 * a message that names the item, when a called key frame, a point the walk would move, one of its observers or its reference key
 * frame lacks geometry or is unknown, when the scales are missing, or when the ref_level of such a point with observations is
 * out of range; DRFE_ERR_CAPACITY when points_capacity is too small.  On success the call commits poses, positions and stamps
 * into the store, and on the device into the resident image in place. */
int drfe_lmap_correct_host(drfe_lmap* db, int32_t cur, const double* Scw, int32_t n, const int32_t* handles, drfe_lmap_correct_out* out);
int drfe_lmap_correct_device(drfe_lmap* db, int32_t cur, const double* Scw, int32_t n, const int32_t* handles,
                             drfe_lmap_correct_out* out, void* stream);
int drfe_lmap_correct_batch(drfe_lmap* db, int32_t cur, const double* Scw, int32_t n, const int32_t* handles,
                            drfe_lmap_correct_out* out, void* stream);
/* out[0] entries of a match row that one claim workgroup takes, [1] DRFE_LMAP_CORRECT_DEVICE_FROM, [2] bytes of scratch per
 * match-row entry of a chunk, [3] workgroup size */
int drfe_lmap_correct_limits(int32_t* out4);
/* the scratch a device call of these handles takes: out[0] bytes with which it runs as one chunk, [1] the least bytes with which
 * it runs at all (one key frame a chunk), [2] the part every chunk shares */
int drfe_lmap_correct_scratch(drfe_lmap* db, int32_t n, const int32_t* handles, int64_t* out3);
/* Counters since the store was created: stats[0] correct calls, [1] called key frames, [2] calls run on the device, [3] points
 * moved, [4] moved points without observations, [5] match-row entries walked, [6] chunks run on the device, [7] uploads of the
 * geometry. */
int drfe_lmap_correct_stats(drfe_lmap* db, int64_t* stats /* 8 */);

/* LocalMapping::KeyFrameCulling (src/LocalMapping.cc:1226-1285) with KeyFrame::SetBadFlag (src/KeyFrame.cc:574-683) underneath it,
 * on the same store: the one entry that takes something away.  DESIGN.md section 28.  Parity with a build of the reference's
 * LocalMapping.cc and KeyFrame.cc is not pinned.
 *
 * The attributes it reads are optional; a store without them behaves as before.  Per key frame: mThDepth, a flags byte (bit 0
 * mbNotErase, bit 1 mnId == 0, bit 2 mbToBeErased) and three arrays parallel to its match row: mvKeysUn[i].octave, mvDepth[i] and
 * mvuRight[i] >= 0.  Per map point: the nObs counter as the reference holds it (it is not derived from the observations) and
 * mit->second of every stored observation, parallel to them.  A setter row replaces the stored one, may name a handle that is not
 * stored yet, and is uploaded before the next device call in a block of its own: an edit of the attributes does not send the
 * graph again.  Attributes whose arrays do not have the length of the stored row count as missing.  drfe_lmap_remove drops them
 * with the item. */
typedef struct drfe_lmap_cull_attributes {
    int32_t n_kfs, n_points;
    const int32_t* kf_handle;         /* n_kfs */
    const float* th_depth;            /* n_kfs */
    const uint8_t* kf_flags;          /* n_kfs */
    const int32_t* row_offsets;       /* n_kfs + 1 */
    const int32_t* octave;            /* by row_offsets */
    const float* depth;
    const uint8_t* stereo;
    const int32_t* point_handle;      /* n_points */
    const int32_t* n_obs;             /* n_points */
    const int32_t* obs_offsets;       /* n_points + 1 */
    const int32_t* obs_index;         /* by obs_offsets */
} drfe_lmap_cull_attributes;
int drfe_lmap_set_cull_attributes(drfe_lmap* db, const drfe_lmap_cull_attributes* rows);
/* The stored attributes of the named items (one without: DRFE_ERR_INVALID); the handle arrays are read, the others written when
 * row_capacity / obs_capacity hold them (DRFE_ERR_CAPACITY otherwise).  n_kfs or n_points may be 0. */
typedef struct drfe_lmap_cull_attributes_out {
    int32_t n_kfs, n_points, row_capacity, obs_capacity;
    const int32_t* kf_handle;
    float* th_depth;
    uint8_t* kf_flags;
    int32_t* row_offsets;
    int32_t* octave;
    float* depth;
    uint8_t* stereo;
    const int32_t* point_handle;
    int32_t* n_obs;
    int32_t* obs_offsets;
    int32_t* obs_index;
} drfe_lmap_cull_attributes_out;
int drfe_lmap_get_cull_attributes(drfe_lmap* db, drfe_lmap_cull_attributes_out* out);

/* A call names n handles: GetVectorCovisibleKeyFrames() of the current key frame, in that order (at most DRFE_LMAP_MAX_QUERIES).
 * The walk order is the caller's, not rank order.  A handle named twice, an unknown one or a key frame that is already bad is
 * refused with DRFE_ERR_INVALID.  The mbNewPlane early return, map lines and planes, Map::EraseKeyFrame and
 * KeyFrameDatabase::erase stay with the caller, which gets the culled list; the decision reads none of them.
 *
 * Kept from the reference, per called key frame in order.  One with flag bit 1 is skipped (action 3).  Its match row is walked in
 * index order; null and bad entries are skipped; with monocular == 0 an entry with depth > th_depth || depth < 0 is skipped (as
 * written: a NaN depth counts); every other entry adds to nMPs.  Only when the point's n_obs > 3 is its observer list looked at:
 * the key frame itself is skipped, an observer counts when octave(observer, obs_index) <= octave + 1, and three of them make the
 * entry redundant.  The verdict is nRedundant > 0.9 * nMPs with the product in double.
 *
 * A verdict on a key frame with flag bit 0 only sets its bit 2 (action 2).  Otherwise (action 1) every key frame of its weights
 * row that holds it loses the entry and gets its ordered row sorted again from all its weights (descending weight, descending
 * rank among equals: AddConnection's rule), and its neighbours refreshed from the first ten.  Every non-null entry of its match
 * row, bad or not, in index order, gets EraseObservation: when the point's observations hold the key frame, n_obs drops by 2
 * where stereo[obs_index] is set and by 1 otherwise, the observation goes, the point's reference key frame - when the store has
 * its geometry and it was this key frame - becomes the lowest-ranked remaining observer (with none left the stored value stays
 * and the read is counted: the reference reads begin() of an empty map), and with n_obs <= 2 the point goes bad: its observations
 * are cleared and every remaining observer's match-row entry at its obs_index is set to null, whatever stands there.  The key
 * frame's own weights and ordered rows are cleared.  The spanning tree follows as written: parent candidates start as the key
 * frame's parent; per round every child that is not bad, in rank order, has its ordered row compared with the candidates and
 * the pair with the greatest weight wins (strict >, from -1; the weight is the child's own for that key frame, 0 when it has
 * none), the winning child takes that parent, becomes a candidate and leaves the children; a round without a winner sends every
 * remaining child, bad ones included, to the key frame's parent and leaves them in its child set.  The parent loses the key frame
 * as a child, Tcp = Tcw * Twc(parent) is the float 4x4 product of section 27 when both have poses, and the key frame is bad.
 * Later key frames of the call see all of it.
 *
 * A call is refused with DRFE_ERR_STATE and a message that names the item, and changes nothing, when a called key frame that is
 * not the origin, a point in its row or an observer of such a point lacks attributes, when an obs_index of such a point lies
 * outside its observer's row, or when a key frame the walk culls has no parent (the reference would dereference null). */
typedef struct drfe_lmap_cull_out {
    int32_t touched_capacity, children_capacity, nulled_capacity, points_capacity, obs_capacity;
    int32_t pad;
    /* per called key frame, in the caller's order */
    int32_t* record;                  /* n x 4: nMPs, nRedundant, verdict, action (0 kept, 1 culled, 2 deferred by mbNotErase,
                                         3 skipped origin) */
    float* Tcp;                       /* n x 16: mTcp of a culled key frame, zeros otherwise */
    uint8_t* has_Tcp;                 /* n: 1 when Tcp was computed */
    int32_t* n_culled;                /* 1 */
    int32_t* culled;                  /* n: the culled key frames in order */
    /* per key frame whose rows, parent, children, match row or bad flag changed, in ascending rank: the final state */
    int32_t* n_touched;               /* 1 */
    int32_t* touched;                 /* touched_capacity handles */
    drfe_lmap_conn_rows rows;         /* its arrays hold touched_capacity (+ 1) rows */
    uint8_t* flags;                   /* touched_capacity: bit 0 the weights row, bit 1 the ordered row, bit 2 the parent, bit 3 the
                                         children differ from what was stored, bit 4 match-row entries were nulled, bit 5 it went bad */
    int32_t* children_offsets;        /* touched_capacity + 1 */
    int32_t* children;                /* children_capacity, ascending rank */
    int32_t* nulled_offsets;          /* touched_capacity + 1 */
    int32_t* nulled;                  /* nulled_capacity: the match-row indices set to null, ascending */
    /* per map point that lost an observation, in ascending handle: the final state */
    int32_t* n_points;                /* 1 */
    int32_t* points;                  /* points_capacity handles */
    int32_t* point_n_obs;
    int32_t* point_ref;               /* the reference key frame, or -1 when the store has no geometry of the point */
    uint8_t* point_bad;
    int32_t* obs_offsets;             /* points_capacity + 1 */
    int32_t* obs;                     /* obs_capacity: the remaining observations in stored order */
    int32_t* obs_index;               /* obs_capacity */
} drfe_lmap_cull_out;
/* key frames in a call from which drfe_lmap_cull_batch of a store with a context uses the device.  Measured (DESIGN.md section 28,
 * profiles/cull_timing.jsonl) the device entry wins from 4 key frames a call when nothing is culled and does not win at every
 * store size when a tenth of the call is culled, so there is no such size: the constant stands above DRFE_LMAP_MAX_QUERIES and
 * _batch runs on the host; _device is there to be called. */
enum { DRFE_LMAP_CULL_DEVICE_FROM = 4097 };
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context; DRFE_ERR_CAPACITY when the working
 * state and the longest called row do not fit the configured scratch), _batch on the device from DRFE_LMAP_CULL_DEVICE_FROM key
 * frames when the call fits.  All three return the same bytes and leave the same store.  When a capacity is too small the call
 * returns DRFE_ERR_CAPACITY and nothing changes.  On success the call commits into the rows and the image in place; a call that
 * culled nothing leaves the device image as it is, one that culled has the changed pieces sent before the next device call
 * (drfe_lmap_upload_bytes). */
int drfe_lmap_cull_host(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t monocular, drfe_lmap_cull_out* out);
int drfe_lmap_cull_device(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t monocular, drfe_lmap_cull_out* out, void* stream);
int drfe_lmap_cull_batch(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t monocular, drfe_lmap_cull_out* out, void* stream);
/* out[0] entries of a match row that one record workgroup takes, [1] DRFE_LMAP_CULL_DEVICE_FROM, [2] bytes of scratch per
 * match-row entry of a chunk, [3] threads of the walking workgroup */
int drfe_lmap_cull_limits(int32_t* out4);
/* the scratch a device call of these handles takes: out[0] bytes with which it runs as one chunk, [1] the least bytes with which
 * it runs at all (one key frame a chunk), [2] the part every chunk shares (the working state) */
int drfe_lmap_cull_scratch(drfe_lmap* db, int32_t n, const int32_t* handles, int64_t* out3);
/* Counters since the store was created: stats[0] cull calls, [1] called key frames, [2] calls run on the device, [3] key frames
 * culled, [4] deferred by mbNotErase, [5] points gone bad, [6] observers walked (the lists the decision looked at), [7] reads of
 * begin() of an empty observation map. */
int drfe_lmap_cull_stats(drfe_lmap* db, int64_t* stats /* 8 */);
/* Host-to-device bytes since the store was created, per block of the device image: out[0] the rows block (bad flags, match rows,
 * observations), [1] the graph block, [2] the geometry, [3] the culling attributes, [4] the state of the map update after a global
 * bundle adjustment (below).  After a cull call the next device call sends
 * the bad flags, 4 bytes per nulled match-row entry, the observations with their offsets when a row got shorter, the graph
 * block, and the counters and observation indices of the attributes; the match rows stay where they are. */
int drfe_lmap_upload_bytes(drfe_lmap* db, int64_t* out5);

/* The map update that ends LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:722-783) on the same store: the walk over the
 * spanning tree that gives every key frame its new pose, then the move of every map point of the map.  The adjustment itself stays
 * with the caller.  DESIGN.md section 29.  Parity with a build of the reference's LoopClosing.cc is not pinned.
 *
 * The state it reads is optional; a store that is never given it behaves as before.  Per key frame: mTcwGBA, mnBAGlobalForKF as a
 * handle (0 when never given, as the constructors leave it) and mTcwBefGBA, which only a call leaves.  Per map point: mPosGBA and
 * mnBAGlobalForKF.  The setters are what the integrator calls after Optimizer::BundleAdjustment's write-back (src/Optimizer.cc:
 * 505-546): the last row of a handle wins, a row may name a handle that is not stored yet, drfe_lmap_remove drops the state with
 * the item.  The state lies in a device block of its own: an edit of it sends neither the rows, the graph nor the geometry again. */
int drfe_lmap_set_gba_keyframes(drfe_lmap* db, int32_t count, const int32_t* handles, const float* TcwGBA /* 16 each */,
                                const int32_t* stamp);
int drfe_lmap_set_gba_points(drfe_lmap* db, int32_t count, const int32_t* handles, const float* PosGBA /* 3 each */, const int32_t* stamp);
/* each array may be NULL; has_TcwGBA and has_TcwBefGBA tell whether the matrix was ever stored (zeros otherwise).  A handle without
 * state: DRFE_ERR_INVALID */
int drfe_lmap_get_gba_keyframes(drfe_lmap* db, int32_t count, const int32_t* handles, float* TcwGBA, int32_t* stamp, float* TcwBefGBA,
                                uint8_t* has_TcwGBA, uint8_t* has_TcwBefGBA);
int drfe_lmap_get_gba_points(drfe_lmap* db, int32_t count, const int32_t* handles, float* PosGBA, int32_t* stamp, uint8_t* has_PosGBA);

/* A call names loop, nLoopKF as a handle, and the origins, mpMap->mvpKeyFrameOrigins, each once (n_origins <= 0 or a duplicate:
 * DRFE_ERR_INVALID).
 *
 * Kept from the reference.  A FIFO starts with the origins.  For the front key frame, Twc is the inverse of its pose before its
 * own SetPose; its children are walked in rank order; a child whose stamp differs from loop gets mTcwGBA = (Tcw_child * Twc) *
 * mTcwGBA_parent, two float 4x4 products, with the parent's mTcwGBA the adjustment's or itself composed a moment before, and takes
 * the stamp; every child is pushed, stamped or not; then mTcwBefGBA = the pose and SetPose(mTcwGBA).  An origin is never composed
 * and never stamped: it takes whatever mTcwGBA it holds.  isBad() is tested nowhere in the walk.  Then every map point of the
 * store, in slot order: a bad point is skipped; a point whose stamp equals loop goes to mPosGBA (kind 1); otherwise, when its
 * reference key frame's stamp after the walk differs from loop the point is skipped, else it goes through mTcwBefGBA of that key
 * frame and the inverse of its new pose (kind 2): Xc = Rcw * X + tcw, then Rwc * Xc + twc, each a float dot with the C term added in
 * double.  An unreached reference key frame that holds the stamp is used with the mTcwBefGBA an earlier call left, stale as it is.
 * The reference key frame's badness is not tested.  With loop == 0 and untouched stamps everything counts as stamped.
 * UpdateNormalAndDepth is not called, and map lines and planes are not touched although the adjustment stamps them too. */
typedef struct drfe_lmap_gba_out {
    int32_t keyframes_capacity;       /* visited key frames; the number of stored key frames always suffices */
    int32_t points_capacity;          /* moved points; the number of stored points always suffices */
    /* per visited key frame, in the reference's FIFO order */
    int32_t* n_keyframes;             /* 1 */
    int32_t* keyframes;               /* handles */
    float* Tcw;                       /* 16 each: the pose SetPose receives */
    float* TcwBef;                    /* 16 each: mTcwBefGBA */
    uint8_t* composed;                /* 1 = composed through the parent (and stamped), 0 = the mTcwGBA it held */
    /* per moved point, in ascending slot (ascending handle) */
    int32_t* n_points;                /* 1 */
    int32_t* points;                  /* handles */
    float* world;                     /* 3 each: the new position */
    uint8_t* kind;                    /* 1 = mPosGBA, 2 = through the reference key frame */
} drfe_lmap_gba_out;
/* stored points from which drfe_lmap_gba_batch of a store with a context uses the device (the measured crossover, DESIGN.md
 * section 29, profiles/gba_propagate_timing.jsonl: the smallest measured store from which the device entry wins at every stamp
 * mix, the setters that precede a call included) */
enum { DRFE_LMAP_GBA_DEVICE_FROM = 125000 };
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context; DRFE_ERR_CAPACITY when the
 * configured scratch does not hold one point slot), _batch on the device from DRFE_LMAP_GBA_DEVICE_FROM stored points when the call
 * fits.  All three return the same bytes and leave the same store.  A refused call changes nothing: DRFE_ERR_STATE, with a message
 * that names the item, when an origin is unknown; when a visited key frame has no pose; when an origin, or a visited key frame
 * that holds the stamp, has no mTcwGBA; when a key frame would be visited twice (in two children rows, an origin in a children
 * row, a cycle); when a point that is not bad has no geometry (it either moves, and its position is part of its geometry, or is
 * asked for its reference key frame); when a point of kind 1 has no mPosGBA; when a point that is not bad and does not hold the
 * stamp has an unknown reference key frame, or would move with kind 2 through a key frame without a pose, or through an unreached
 * one without a stored mTcwBefGBA; DRFE_ERR_CAPACITY when a capacity is too small.  On success the call commits poses (with Ow and
 * Twc), mTcwBefGBA, the composed mTcwGBA, the key-frame stamps and the positions into the store, and on the device into the
 * resident geometry and state blocks in place, with no upload of what it wrote. */
int drfe_lmap_gba_host(drfe_lmap* db, int32_t loop, int32_t n_origins, const int32_t* origins, drfe_lmap_gba_out* out);
int drfe_lmap_gba_device(drfe_lmap* db, int32_t loop, int32_t n_origins, const int32_t* origins, drfe_lmap_gba_out* out, void* stream);
int drfe_lmap_gba_batch(drfe_lmap* db, int32_t loop, int32_t n_origins, const int32_t* origins, drfe_lmap_gba_out* out, void* stream);
/* out[0] threads of a workgroup = point slots of one, [1] DRFE_LMAP_GBA_DEVICE_FROM, [2] the depth of unstamped chain the in-launch
 * loop handles (0 = any: one workgroup loops over the rounds), [3] bytes of scratch per point slot of a chunk, [4] bytes of scratch
 * every chunk shares, [5] lanes of a wavefront */
int drfe_lmap_gba_limits(int32_t* out6);
/* the scratch a device call takes: out[0] bytes with which it runs as one chunk, [1] the least bytes with which it runs at all
 * (one point slot a chunk), [2] the part every chunk shares */
int drfe_lmap_gba_scratch(drfe_lmap* db, int64_t* out3);
/* Counters since the store was created: stats[0] calls, [1] calls run on the device, [2] key frames visited, [3] key frames
 * composed, [4] the deepest unstamped chain seen, [5] points of kind 1, [6] points of kind 2, [7] points skipped for a reference
 * key frame without the stamp. */
int drfe_lmap_gba_stats(drfe_lmap* db, int64_t* stats /* 8 */);

/* LocalMapping::MapPointCulling and MapLineCulling (src/LocalMapping.cc:175-231) on the same store: the two walks over
 * mlpRecentAddedMapPoints and mlpRecentAddedMapLines that run for every new key frame, with MapPoint::SetBadFlag and
 * MapLine::SetBadFlag.  DESIGN.md section 31.  Parity with a build of the reference's LocalMapping.cc is not pinned.
 *
 * The state they read is optional; a store that is never given it behaves as before.  Per map point mnFound, mnVisible and
 * mnFirstKFid (nObs and mit->second are the culling attributes above).  Per map line the same three, nObs as MapLine holds it
 * (AddObservation adds 1), the observing key frames in the caller's pointer order and mit->second parallel to them (a key frame
 * twice in a row, a negative handle: DRFE_ERR_INVALID).  The last row of a handle wins and replaces the stored one, a row may name
 * a handle that is not stored yet, drfe_lmap_remove drops the state with the item.  An observation of a stored line that names an
 * unknown key frame refuses every call that reads the image, like one of a point (DRFE_ERR_STATE).  The state lies in a device
 * block of its own: an edit of it sends neither the rows, the graph nor the culling attributes again. */
typedef struct drfe_lmap_recent_attributes {
    int32_t n_points, n_lines;
    const int32_t* point_handle;
    const int32_t* point_found;
    const int32_t* point_visible;
    const int64_t* point_first_kf;
    const int32_t* line_handle;
    const int32_t* line_found;
    const int32_t* line_visible;
    const int64_t* line_first_kf;
    const int32_t* line_n_obs;
    const int32_t* line_obs_offsets;  /* n_lines + 1 */
    const int32_t* line_obs;          /* key-frame handles */
    const int32_t* line_obs_index;    /* parallel */
} drfe_lmap_recent_attributes;
int drfe_lmap_set_recent_attributes(drfe_lmap* db, const drfe_lmap_recent_attributes* rows);
/* the stored state of the named handles (one without it: DRFE_ERR_INVALID; line_obs_capacity too small: DRFE_ERR_CAPACITY) */
typedef struct drfe_lmap_recent_attributes_out {
    int32_t n_points, n_lines, line_obs_capacity;
    const int32_t* point_handle;
    int32_t* point_found;
    int32_t* point_visible;
    int64_t* point_first_kf;
    const int32_t* line_handle;
    int32_t* line_found;
    int32_t* line_visible;
    int64_t* line_first_kf;
    int32_t* line_n_obs;
    int32_t* line_obs_offsets;
    int32_t* line_obs;
    int32_t* line_obs_index;
} drfe_lmap_recent_attributes_out;
int drfe_lmap_get_recent_attributes(drfe_lmap* db, drfe_lmap_recent_attributes_out* out);
/* MapPoint::IncreaseFound / IncreaseVisible (kind DRFE_LMAP_POINT) and MapLine's (DRFE_LMAP_LINE): d_found[i] and d_visible[i] are
 * added to handle i, with wrap-around; a handle may be named more than once.  A handle without the state: DRFE_ERR_INVALID, and
 * nothing changes.  Only the four counter arrays of the block travel afterwards. */
int drfe_lmap_recent_increase(drfe_lmap* db, int kind, int32_t count, const int32_t* handles, const int32_t* d_found, const int32_t* d_visible);

/* A call names current_kf_id (mpCurrentKeyFrame->mnId, a value), monocular, and the two recent lists as handles in list order
 * (each at most DRFE_LMAP_RECENT_MAX_ENTRIES; either may be empty; a handle may stand in a list more than once, as
 * ProcessNewKeyFrame pushes once per row index).
 *
 * Kept from the reference.  Each entry in order: an item that is bad is dropped (action 1).  A point with
 * static_cast<float>(mnFound) / mnVisible < 0.25f - both converted to float, one correctly rounded division; mnVisible == 0 gives
 * inf or NaN and NaN is not less - or a line with static_cast<float>(mnFound / mnVisible) < 0.25f - the integer division, so
 * every line with 0 <= found < visible - gets SetBadFlag and is dropped (action 2).  Otherwise, with d = (int)current_kf_id -
 * (int)mnFirstKFid (both truncated to int, the difference in 64 bits): d >= 2 && Observations() <= (monocular ? 2 : 3) on the
 * stored counter gets SetBadFlag and is dropped (action 3); d >= 3 is dropped (action 4); else the entry stays (action 0).  The
 * first occurrence of a handle carries its verdict; a later occurrence of a culled item is action 1, of any other repeats its
 * action.  SetBadFlag: the item goes bad, its observations are cleared, and for every former observation in stored order the
 * observer's mvpMapPoints[idx] (mvpMapLines[idx]) becomes null whatever stands there, also another live item, also in a bad
 * observer.  nObs, found, visible and the reference key frame stay; an entry of a row that names the item without an observation
 * behind it stays; Map::EraseMapPoint / EraseMapLine stay with the caller.
 *
 * Refused, and nothing changes: an unknown handle (DRFE_ERR_INVALID); with the item's name and DRFE_ERR_STATE a listed item that
 * is not bad without the state above (a point: or without culling attributes that fit its observations), with an obs_index
 * outside its observer's row, and a listed line that is not bad with mnVisible == 0 or with INT_MIN / -1, where the reference
 * divides by zero or overflows; an output array that is too small (DRFE_ERR_CAPACITY). */
enum { DRFE_LMAP_RECENT_MAX_ENTRIES = 1 << 20 };
enum { DRFE_LMAP_RECENT_KEPT = 0, DRFE_LMAP_RECENT_WAS_BAD = 1, DRFE_LMAP_RECENT_RATIO = 2, DRFE_LMAP_RECENT_OBSERVATIONS = 3,
       DRFE_LMAP_RECENT_AGED = 4 };
/* one kind's share of a call: in the list, out what became of it */
typedef struct drfe_lmap_recent_list {
    int32_t n;                        /* list entries */
    const int32_t* handles;           /* in list order */
    int32_t erased_capacity;          /* entries of erased_kf / erased_index */
    uint8_t* action;                  /* n: per list entry */
    int32_t* n_kept;                  /* 1 */
    int32_t* kept;                    /* n: the surviving list, in list order */
    int32_t* n_culled;                /* 1 */
    int32_t* culled;                  /* n: the handles that got SetBadFlag, in list order */
    int32_t* erased_offsets;          /* n + 1: per culled item, from 0 */
    int32_t* erased_kf;               /* the erased observations in stored order: key-frame handle */
    int32_t* erased_index;            /* and index into its row */
} drfe_lmap_recent_list;
/* entries of both lists from which drfe_lmap_recent_cull_batch of a store with a context uses the device.  Measured (DESIGN.md
 * section 31, profiles/recent_cull_timing.jsonl) the device entry wins at 32 768 entries in five of six shapes and at 4 096 in one,
 * and at no length at every store size with a tenth culled and with none culled, so there is no such length: the constant stands
 * above the longest call and _batch runs on the host; _device is there to be called. */
enum { DRFE_LMAP_RECENT_DEVICE_FROM = 2 * DRFE_LMAP_RECENT_MAX_ENTRIES + 1 };
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context; DRFE_ERR_CAPACITY when the
 * configured scratch does not hold the claim words and one list entry), _batch on the device from DRFE_LMAP_RECENT_DEVICE_FROM
 * entries of both lists when the call fits.  All three return the same bytes and leave the same store.  On success the call
 * commits into the rows and the image; the device entry commits the bad flags and the nulled entries into the resident image
 * itself, so that after it only the observations with their offsets travel (drfe_lmap_upload_bytes: no match rows, no graph). */
int drfe_lmap_recent_cull_host(drfe_lmap* db, int64_t current_kf_id, int32_t monocular, drfe_lmap_recent_list* points,
                               drfe_lmap_recent_list* lines);
int drfe_lmap_recent_cull_device(drfe_lmap* db, int64_t current_kf_id, int32_t monocular, drfe_lmap_recent_list* points,
                                 drfe_lmap_recent_list* lines, void* stream);
int drfe_lmap_recent_cull_batch(drfe_lmap* db, int64_t current_kf_id, int32_t monocular, drfe_lmap_recent_list* points,
                                drfe_lmap_recent_list* lines, void* stream);
/* out[0] list entries of one workgroup of the device's entry launches, [1] erased observations of one pass of an erase workgroup,
 * [2] bytes of scratch per list entry of a chunk, [3] lanes of a wavefront, [4] DRFE_LMAP_RECENT_MAX_ENTRIES, [5]
 * DRFE_LMAP_RECENT_DEVICE_FROM */
int drfe_lmap_recent_cull_limits(int32_t* out6);
/* the scratch a device call of n_entries list entries takes: out[0] bytes with which it runs as one chunk, [1] the least bytes
 * with which it runs at all (one entry a chunk), [2] the part every chunk shares (a claim word per stored point and line) */
int drfe_lmap_recent_cull_scratch(drfe_lmap* db, int64_t n_entries, int64_t* out3);
/* Counters since the store was created: stats[0] calls, [1] list entries, [2] calls run on the device, [3] culled by ratio, [4]
 * culled by observations, [5] aged out, [6] dropped as already bad, [7] match-row entries that went from an item to null. */
int drfe_lmap_recent_cull_stats(drfe_lmap* db, int64_t* stats /* 8 */);
/* host-to-device bytes of the recent-list block since the store was created (the sixth block, next to drfe_lmap_upload_bytes) */
int drfe_lmap_recent_upload_bytes(drfe_lmap* db, int64_t* out1);

/* The fuse commit on the same store: the loop that applies a fusion search - ORBmatcher::Fuse (src/ORBmatcher.cc:845-976, and the
 * Sim3 form :1001-1101 with SearchAndFuse's loop, src/LoopClosing.cc:650-657), LSDmatcher::Fuse (src/LSDmatcher.cpp:897-1012), the
 * matched-point loop of CorrectLoop (src/LoopClosing.cc:566-581) - with MapPoint::Replace / MapLine::Replace
 * (src/MapPoint.cc:223-261, src/MapLine.cpp:178-214), AddObservation, KeyFrame::AddMapPoint, ReplaceMapPointMatch and
 * EraseMapPointMatch.  DESIGN.md section 32.  Parity with a build of the reference's ORBmatcher.cc, LSDmatcher.cpp, MapPoint.cc,
 * MapLine.cpp and LoopClosing.cc is not pinned.
 *
 * A call is an ordered list of steps, run one after another on the evolving store.  A step names a key frame, a kind
 * (DRFE_LMAP_POINT or DRFE_LMAP_LINE), a form, its candidates as handles in the caller's order (-1 = a null pointer) and best_idx per
 * candidate: the search's answer with the bestDist <= TH_LOW gate applied, any negative value = none.  It reads and writes the
 * match rows, the bad flags, the observations with mit->second and nObs (the culling attributes of a point, the recent-list state
 * of a line), mnFound / mnVisible and the per-item `replaced` field below.
 *
 * Per candidate one action byte.  0 comes first in every form: a null candidate, or no answer (in MATCHED only the null candidate).
 *
 * NEIGHBOURS, per candidate in order: a candidate that is bad, or - a point only: LSDmatcher::Fuse does not ask - that has the
 * key frame among its observations at its turn, is skipped (1).  The occupant row[k][best_idx] is read now.  Null:
 * AddObservation(k, best_idx), then row[k][best_idx] = candidate (2; 3 for a line that already observed the key frame, whose
 * AddObservation is a no-op).  Bad: nothing, and the candidate still counts (4).  The candidate itself: Replace returns at once (7).  Otherwise, on the
 * stored counters, occupant.nObs > candidate.nObs ? candidate.Replace(occupant) (5) : occupant.Replace(candidate) (6): on a tie
 * the occupant loses.  n_fused counts 2, 3, 4, 5, 6 and 7.
 *
 * LOOP (points, no null candidate): the skip set is taken once at the start of the step - bad then, or among the non-null entries
 * of row[k] then (1).  Pass 1 in order: occupant not null and not bad: recorded in replace[i] (8); bad: 4; null:
 * AddObservation and AddMapPoint (2, or 3 when the key frame already was an observer and only the row entry is written).  n_fused
 * counts 2, 3, 4 and 8.  Pass 2 in order: replace[i].Replace(candidate[i]), whatever the two are by then - an occupant recorded
 * twice is replaced twice, the second time with no observations left, and its found and visible counts are added again; the
 * candidate may have gone bad; replace[i] == candidate[i] returns at once.
 *
 * MATCHED (points): candidate i stands for row index i, best_idx is not read, n must be the row's length.  A non-null candidate
 * with an occupant: occupant.Replace(candidate), without a bad test or a comparison (6; 7 for the candidate itself); without one:
 * AddMapPoint, then AddObservation (2, or 3).  n_fused counts 2, 3, 6 and 7.
 *
 * Replace(loser, winner): the loser goes bad, its observations are taken and cleared, replaced[loser] = winner.  Per former
 * observation (kf, idx) in stored order: kf not among the winner's observers at that moment - row[kf][idx] = winner and the winner
 * gains (kf, idx) (a record with moved 1); else row[kf][idx] = null (moved 0); either is stored whatever stands in the entry.
 * The winner's mnFound / mnVisible grow by the loser's, with wrap-around.  The loser's nObs, counters and reference key frame
 * stay; a bad winner is not tested.  A gained observation adds 2 to a point's nObs when the stereo flag of (kf, idx) is set, else 1,
 * and 1 to a line's; it enters the stored list in front of the first stored observer of greater rank, at the end if there is none.
 * Map::EraseMapPoint, ComputeDistinctiveDescriptors and UpdateNormalAndDepth stay with the caller: `touched` names every winner
 * and every item that gained an observation, once each, in the order first met. */
enum { DRFE_LMAP_FUSE_NEIGHBOURS = 0, DRFE_LMAP_FUSE_LOOP = 1, DRFE_LMAP_FUSE_MATCHED = 2 };
enum { DRFE_LMAP_FUSE_NONE = 0, DRFE_LMAP_FUSE_SKIPPED = 1, DRFE_LMAP_FUSE_ADDED = 2, DRFE_LMAP_FUSE_ROW_ONLY = 3,
       DRFE_LMAP_FUSE_OCCUPANT_BAD = 4, DRFE_LMAP_FUSE_CANDIDATE_REPLACED = 5, DRFE_LMAP_FUSE_OCCUPANT_REPLACED = 6,
       DRFE_LMAP_FUSE_SELF = 7, DRFE_LMAP_FUSE_RECORDED = 8 };
enum { DRFE_LMAP_FUSE_MAX_CANDIDATES = 1 << 22 };   /* of all steps of a call */
typedef struct drfe_lmap_fuse_step {
    int32_t keyframe;                 /* handle */
    int32_t kind;                     /* DRFE_LMAP_POINT or DRFE_LMAP_LINE */
    int32_t form;                     /* DRFE_LMAP_FUSE_... */
    int32_t n;                        /* candidates */
    const int32_t* candidates;        /* n handles, -1 = null */
    const int32_t* best_idx;          /* n; may be NULL in MATCHED */
    uint8_t* action;                  /* n */
    int32_t* n_fused;                 /* 1 */
    int32_t* replace;                 /* LOOP: n handles, -1 = none; may be NULL in the other forms */
} drfe_lmap_fuse_step;
typedef struct drfe_lmap_fuse_call {
    int32_t n_steps;
    drfe_lmap_fuse_step* steps;
    int32_t replaced_capacity;        /* Replace calls that change something: the candidates that are not null and have an answer always suffice */
    int32_t record_capacity;          /* their (kf, idx) records: replaced_capacity x the stored key frames always suffices */
    int32_t touched_capacity;         /* per kind: the same count of candidates of that kind always suffices */
    int32_t* n_replaced;              /* 1 */
    int32_t* replaced_kind;           /* in execution order */
    int32_t* loser;                   /* handles */
    int32_t* winner;
    int32_t* record_offsets;          /* replaced_capacity + 1, from 0 */
    int32_t* record_kf;               /* the loser's former observations in stored order: key-frame handle */
    int32_t* record_index;            /* index into its row */
    uint8_t* record_moved;            /* 1 = the entry names the winner and the winner gained it, 0 = the entry is null */
    int32_t* n_touched;               /* 2: points, lines */
    int32_t* touched_points;          /* handles */
    int32_t* touched_lines;
} drfe_lmap_fuse_call;
/* candidates of all steps from which drfe_lmap_fuse_batch of a store with a context uses the device.  Measured (DESIGN.md
 * section 32, profiles/fuse_timing.jsonl) the device entry loses to the host entry in every one of twelve shapes (0.08x to 0.70x),
 * so there is no such number: the constant stands above the longest call and _batch runs on the host; _device is there to be
 * called. */
enum { DRFE_LMAP_FUSE_DEVICE_FROM = DRFE_LMAP_FUSE_MAX_CANDIDATES + 1 };
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context; DRFE_ERR_CAPACITY when the
 * configured scratch does not hold the call or the store has more key frames than the walk's observer bitmap), _batch on the
 * device from DRFE_LMAP_FUSE_DEVICE_FROM candidates when the call fits.  All three return the same bytes and leave the same
 * store.  Refused, and nothing changes: an unknown key frame or item handle, an unknown kind or form, more than
 * DRFE_LMAP_FUSE_MAX_CANDIDATES candidates (DRFE_ERR_INVALID); with DRFE_ERR_STATE and the name of the item a line in LOOP or
 * MATCHED, a null candidate in LOOP, a MATCHED list whose length is not the row's, a best_idx beyond row[k], a point step on a
 * key frame without culling attributes that fit its row (the stereo flags), a point that can take part - a candidate or an entry
 * of row[k] that a candidate points at, unless it is bad in a form that never touches a bad item - without culling attributes
 * that fit its observations or without recent-list counters, a line that can take part without its recent-list state, an
 * obs_index of either outside its observer's row; DRFE_ERR_CAPACITY when a capacity is too small.  The device entry commits the
 * match rows, the bad flags, nObs and the counters into the resident blocks itself: after it only the observations with their
 * offsets and indices travel (drfe_lmap_upload_bytes: no match rows, no graph). */
int drfe_lmap_fuse_host(drfe_lmap* db, drfe_lmap_fuse_call* call);
int drfe_lmap_fuse_device(drfe_lmap* db, drfe_lmap_fuse_call* call, void* stream);
int drfe_lmap_fuse_batch(drfe_lmap* db, drfe_lmap_fuse_call* call, void* stream);
/* out[0] candidates of one workgroup of the live pre-pass = threads of the walk's workgroup, [1] lanes of a wavefront, [2] entries
 * of the walk's append log, [3] records the walk holds, [4] key frames its observer bitmap holds, [5] bytes of scratch per
 * candidate tile, [6] DRFE_LMAP_FUSE_MAX_CANDIDATES, [7] DRFE_LMAP_FUSE_DEVICE_FROM */
int drfe_lmap_fuse_limits(int32_t* out8);
/* the scratch a device call of n_candidates in n_steps takes at most (a step starts a tile of its own): out[0] bytes, [1] the same
 * (the walk is one launch: there is no smaller chunk), [2] the part that does not depend on the call */
int drfe_lmap_fuse_scratch(drfe_lmap* db, int64_t n_candidates, int64_t n_steps, int64_t* out3);
/* Counters since the store was created: stats[0] calls, [1] candidates, [2] calls run on the device, [3] observations added to an
 * empty entry, [4] Replace calls that changed something, [5] records moved, [6] records erased, [7] device calls whose walk handed
 * the rest of the call back to the host (its append log or its record room was full). */
int drfe_lmap_fuse_stats(drfe_lmap* db, int64_t* stats /* 8 */);
/* mpReplaced by handle, -1 until a Replace sets it; drfe_lmap_set_points / set_lines of a handle resets it, drfe_lmap_remove
 * drops it.  Host state only.  An unknown handle: DRFE_ERR_INVALID. */
int drfe_lmap_get_replaced(drfe_lmap* db, int kind, int32_t count, const int32_t* handles, int32_t* out);
/* What the store holds by handle, for a caller that compares it with its objects: the match row of a key frame (kind
 * DRFE_LMAP_POINT or DRFE_LMAP_LINE; *n its length, DRFE_ERR_CAPACITY when capacity is smaller), and the bad flag and observing
 * key frames of an item in stored order (a line without recent-list state has none). */
int drfe_lmap_get_match_row(drfe_lmap* db, int kind, int32_t keyframe, int32_t capacity, int32_t* n, int32_t* out);
int drfe_lmap_get_observers(drfe_lmap* db, int kind, int32_t handle, int32_t capacity, uint8_t* bad, int32_t* n, int32_t* out);

/* The item loops of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:113-173) on the same store, with MapPoint::AddObservation
 * and UpdateNormalAndDepth (src/MapPoint.cc:124-138, :370-417) and MapLine::AddObservation (src/MapLine.cpp:91-100).  DESIGN.md
 * section 33.  Parity with a build of the reference's LocalMapping.cc, MapPoint.cc and MapLine.cpp is not pinned.
 *
 * A call names n key frames in queue order (at most DRFE_LMAP_MAX_QUERIES), each once (a handle named twice: DRFE_ERR_INVALID),
 * already stored with their match rows.  The call is the item loops for key frame 0, then key frame 1, and so on, on the evolving
 * store.  Per called key frame k its point row is walked in index order i, then its line row; one action byte per entry:
 *
 *   0 NULL    a null entry.
 *   1 BAD     the item is bad.
 *   2 RECENT  k is among the item's observers at that moment: the handle is appended to recent_points (recent_lines), once per
 *             row index, as the reference pushes; nothing else changes.
 *   3 ADDED   the item gains the observation (k, i).  A point's nObs grows by 2 when the stereo flag of (k, i) in the key frame's
 *             culling attributes is set, else by 1; a line's by 1.  The new observer enters the stored list in front of the first
 *             stored observer of greater rank, at the end if there is none, one addition after another (the fuse commit's rule).
 *
 * So an item that stands twice in one row is ADDED at its first index and RECENT at the second, and an item that already observed
 * k is RECENT at every occurrence.  The bad flags, the match rows and the poses do not change.
 *
 * UpdateNormalAndDepth of an ADDED point runs right after its addition, on the stored position, over the observer list as it stands
 * then - the stored list plus the additions of this and earlier called key frames, in list order - with the stored camera centres,
 * the stored reference key frame and ref_level and the stored scales (the geometry of drfe_lmap_set_poses /
 * _set_point_geometry / _set_scales); float sums in list order.  It is reported per ADDED entry, the way drfe_lmap_correct_out
 * reports it: a point added by two called key frames is reported twice, the second time over one more observer.  The stored
 * geometry holds no normal, so nothing of it is written.  With normal == NULL this part is skipped, no geometry is read and the
 * call is integer-only.  The store holds no line geometry: UpdateAverageDir stays with drfe_map_line_upkeep_*, as do
 * ComputeDistinctiveDescriptors of both kinds, the plane list, ComputeBoW, Map::AddKeyFrame and UpdateConnections
 * (drfe_lmap_connect_*); added_* names every ADDED entry in walk order, which is what the upkeep batch needs.
 *
 * Several key frames in one call: the reference runs UpdateConnections(k) before the next key frame's additions.  A call of several
 * key frames followed by one drfe_lmap_connect_* of all of them lets an earlier key frame's vote see a later one's new
 * observations; a caller who wants the reference's interleaving calls once per key frame.  The result is the same whenever no
 * item is ADDED by two called key frames. */
enum { DRFE_LMAP_INSERT_NULL = 0, DRFE_LMAP_INSERT_BAD = 1, DRFE_LMAP_INSERT_RECENT = 2, DRFE_LMAP_INSERT_ADDED = 3 };
typedef struct drfe_lmap_insert_call {
    int32_t n;                        /* called key frames */
    int32_t pad;
    const int32_t* handles;           /* n, in queue order */
    int32_t action_capacity[2];       /* entries of point_action, line_action: the total length of the called rows of that kind */
    int32_t added_capacity[2];        /* ADDED points, lines; the total length of the called rows of that kind always suffices */
    int32_t recent_capacity[2];       /* RECENT points, lines; the same bound */
    /* per called key frame: its entries are point_action[point_offsets[j] .. point_offsets[j + 1]), row order */
    int32_t* point_offsets;           /* n + 1, from 0 */
    uint8_t* point_action;
    int32_t* line_offsets;            /* n + 1 */
    uint8_t* line_action;
    int32_t* n_added;                 /* 2: points, lines */
    /* per ADDED point entry, in walk order */
    int32_t* added_points;            /* handles */
    int32_t* added_point_kf;          /* the called key frame */
    int32_t* added_point_index;       /* the row index */
    float* normal;                    /* 3 each, or NULL: no UpdateNormalAndDepth, the next three are not written */
    float* max_distance;
    float* min_distance;
    uint8_t* status;                  /* DRFE_UPKEEP_NORMAL */
    /* per ADDED line entry, in walk order */
    int32_t* added_lines;
    int32_t* added_line_kf;
    int32_t* added_line_index;
    int32_t* n_recent;                /* 2 */
    int32_t* recent_points;           /* handles in push order */
    int32_t* recent_lines;
} drfe_lmap_insert_call;
/* row entries of both kinds in a call from which drfe_lmap_insert_batch of a store with a context uses the device.  Measured
 * (profiles/insert_timing.jsonl) the device entry beats the host entry at 64 called key frames on stores
 * of 100 and 1 000 key frames (0.75x to 0.96x of its time) but loses at 4 000 key frames with nine tenths of the entries added,
 * and at 1 and 4 called key frames on the smaller stores: there is no call size from which it wins at every store size, so the
 * constant stands above the longest call and _batch runs on the host; _device is there to be called. */
enum { DRFE_LMAP_INSERT_DEVICE_FROM = 0x7fffffff };
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context; DRFE_ERR_CAPACITY when the
 * configured scratch does not hold the call with one key frame a chunk), _batch on the device from DRFE_LMAP_INSERT_DEVICE_FROM row
 * entries when the call fits.  All three return the same bytes and leave the same store.  Refused, and nothing changes: an
 * unknown or repeated key-frame handle, more than DRFE_LMAP_MAX_QUERIES key frames (DRFE_ERR_INVALID); with DRFE_ERR_STATE and the
 * name of the item a called key frame with a point entry that is ADDED but without culling attributes that fit its row (the stereo
 * flags), a point entry that is not bad without culling attributes that fit its observations, a line entry that is not bad
 * without its recent-list state, and - when normals are asked for and a point is ADDED - missing scales, a missing position of an
 * ADDED point, a missing pose of one of its observers or of its reference key frame, a reference key frame of -1 or unknown, a
 * ref_level out of range; DRFE_ERR_CAPACITY when an output array is too small.  The host entry commits into the rows and the
 * image; the device entry commits nObs into the resident attribute and recent-list blocks itself.  The observation arrays are
 * spliced on the host in both, so after a device call only the observations with their offsets and indices travel
 * (drfe_lmap_upload_bytes, drfe_lmap_recent_upload_bytes: no match rows, no graph, no geometry).  Because it commits as it goes,
 * the device entry settles every refusal before its first launch: at once when every stored key frame and point has culling
 * attributes that fit, every stored point and line its recent-list state and - with normals - every stored item its geometry,
 * and when added_capacity and recent_capacity are at least the called rows' lengths; otherwise by running the host's walk first,
 * so that such a call costs the host's work and the device's. */
int drfe_lmap_insert_host(drfe_lmap* db, drfe_lmap_insert_call* call);
int drfe_lmap_insert_device(drfe_lmap* db, drfe_lmap_insert_call* call, void* stream);
int drfe_lmap_insert_batch(drfe_lmap* db, drfe_lmap_insert_call* call, void* stream);
/* out[0] row entries of one workgroup of the device's entry launches, [1] lanes of a wavefront, [2] bytes of scratch per stored
 * point and line and key frame of a chunk (its claim word), [3] the most workgroups of the normals launch, [4] its workgroup size,
 * [5] DRFE_LMAP_MAX_QUERIES, [6] DRFE_LMAP_INSERT_DEVICE_FROM, [7] 0 */
int drfe_lmap_insert_limits(int32_t* out8);
/* the scratch a device call of these handles takes: out[0] bytes with which it runs as one chunk, [1] the least bytes with which
 * it runs at all (one key frame a chunk), [2] the part every chunk shares (the lists, the records and, with normals, a bit per
 * stored point and called key frame) */
int drfe_lmap_insert_scratch(drfe_lmap* db, int32_t n, const int32_t* handles, int32_t normals, int64_t* out3);
/* Counters since the store was created: stats[0] calls, [1] called key frames, [2] calls run on the device, [3] points added, [4]
 * lines added, [5] recent pushes of points, [6] of lines, [7] chunks run on the device. */
int drfe_lmap_insert_stats(drfe_lmap* db, int64_t* stats /* 8 */);

/* ---- map-point and map-line creation on the map store, appended in place ---- */
/* The tail of LocalMapping::CreateNewMapPoints and CreateNewMapLines2 (reference src/LocalMapping.cc:522-535, :1019-1031), which
 * also ends StereoInitialization, CreateInitialMapMonocular, CreateInitialMapMonoWithLine and both loops of CreateNewKeyFrame in
 * Tracking.cc: a new item, AddObservation per observer (src/MapPoint.cc:124-138, src/MapLine.cpp:91-100), AddMapPoint / AddMapLine
 * into the observers' match rows (src/KeyFrame.cc:287-291, :849-853) and, for a point, UpdateNormalAndDepth
 * (src/MapPoint.cc:376-417).  DESIGN.md section 34.  Parity with a build of the reference's files is not pinned.
 *
 * A call is an ordered list of point creations and one of line creations; the two kinds touch different rows and items, so the
 * call is the point creations one after another, then the line creations, on the evolving store.  A creation holds a new handle,
 * 1 or 2 observations (key frame, row index) in the caller's order, the reference key frame, mnFirstKFid and, for a point, its
 * world position.  The new item is not bad, has found 1, visible 1, first_kf as given, no adjustment state and no mpReplaced; a
 * point gets the geometry (position, ref_kf, level, corrected_by 0, corrected_ref 0).
 *
 * Per observation in order: a key frame that is already among the item's observers is skipped as an observer (two observations on
 * one key frame keep the first); else it enters the observer list in rank order (the fuse commit's rule) with its index, and nObs
 * grows by 2 when the stereo flag of (key frame, index) in the key frame's culling attributes is set, else by 1; a line's by 1.
 * Either way row[key frame][index] = the new handle, whatever stood there: the displaced item keeps its observation and its nObs,
 * as in the reference, and its handle (or -1) is reported per observation.  When two creations of a call name the same entry the
 * later one holds it after the call, and its report names the earlier one.
 *
 * UpdateNormalAndDepth of a created point runs right after, over its own observers in rank order with the stored camera centres
 * and scales: level is the octave, in the reference key frame's culling attributes, of the index the point observes it with.
 * normal, max_distance, min_distance and status are reported per created point, the way drfe_lmap_insert_call reports them; the
 * stored geometry gets level.  With normal == NULL this part is skipped and level is still stored.  The store holds no line
 * geometry: UpdateAverageDir and both kinds' ComputeDistinctiveDescriptors stay with drfe_map_*_upkeep_*, Map::AddMapPoint and
 * the push onto mlpRecentAdded* with the caller.
 *
 * In place: when the store's image is current after the entry's own build, and the new handles of a kind are above every stored
 * handle of that kind and ascending in call order, the new items take the next slots at the end of everything the store keeps by
 * slot and the rows are written by handle and by slot; no image is rebuilt and no resident block is sent again as a whole.  The
 * sections of the resident blocks the call appends to are granted room (twice what the call needs when they lack it: a relayout,
 * which sends that block once and is counted), so that the next device call of any kind uploads the appended tails and the
 * touched row entries only.  A call whose handles do not qualify commits into the rows by handle, leaves the image stale for the
 * next call to rebuild, and is counted. */
typedef struct drfe_lmap_create_call {
    int32_t n_points, n_lines;
    /* per point creation */
    const int32_t* point_handle;
    const int32_t* point_n_obs;       /* 1 or 2 */
    const int32_t* point_obs_kf;      /* 2 each; the second is not read when n_obs is 1 */
    const int32_t* point_obs_index;   /* 2 each */
    const int32_t* point_ref_kf;      /* one of the observations' key frames */
    const int64_t* point_first_kf;
    const float* point_world;         /* 3 each */
    /* per line creation */
    const int32_t* line_handle;
    const int32_t* line_n_obs;
    const int32_t* line_obs_kf;
    const int32_t* line_obs_index;
    const int32_t* line_ref_kf;
    const int64_t* line_first_kf;
    /* out */
    int32_t displaced_capacity[2];    /* entries of point_displaced, line_displaced: 2 per creation */
    int32_t record_capacity;          /* entries of the four arrays below: 1 per point creation */
    int32_t pad;
    int32_t* point_displaced;         /* 2 each: the handle that stood in the row entry or -1; -1 for an observation not given */
    int32_t* line_displaced;
    float* normal;                    /* 3 each, or NULL: no UpdateNormalAndDepth, the next three are not written */
    float* max_distance;
    float* min_distance;
    uint8_t* status;                  /* DRFE_UPKEEP_NORMAL */
} drfe_lmap_create_call;
/* creations of both kinds in a call from which drfe_lmap_create_batch of a store with a context uses the device.  Measured
 * (profiles/create_timing.jsonl: a call followed by one update on the device) the device entry loses at one
 * creation on stores of 100, 1 000 and 4 000 key frames (0.85x to 0.97x of the host entry's speed) and wins at 64 on all three
 * (1.6x, 1.9x, 2.3x), at 512 (3.8x to 4.3x) and at 4 096 (5.1x to 6.3x): 64 is the smallest measured call size from which it wins
 * at every store size.  Most of the margin is the host entry's upload of one copy per touched row entry. */
enum { DRFE_LMAP_CREATE_DEVICE_FROM = 64 };
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context; DRFE_ERR_CAPACITY when the
 * configured scratch does not hold the call with one tile of creations a chunk), _batch on the device from
 * DRFE_LMAP_CREATE_DEVICE_FROM creations when the call fits.  All three return the same bytes and leave the same store.  Refused,
 * and nothing changes: DRFE_ERR_INVALID for a handle the store already holds, a handle that stands twice in the call, a negative
 * handle, an unknown key frame, an index outside the key frame's row, 0 or more than 2 observations, a reference key frame that is
 * not among the creation's observations; DRFE_ERR_STATE with the item's name for a named key frame of a point without culling
 * attributes that fit its row and, with normals, missing scales, a missing pose of an observer, an octave outside the scales;
 * DRFE_ERR_CAPACITY for an output array that is too small.  The host settles every refusal before the first launch.  The device
 * entry needs handles that qualify for the append (else it runs on the host: there is no slot to write); it writes the new slots
 * of the rows, attribute, recent-list and (when current) geometry blocks and the row entries in place, so that only the records
 * come back and the next call of any kind uploads nothing of them (drfe_lmap_upload_bytes); the adjustment block gets its tail
 * with the next call that needs it. */
int drfe_lmap_create_host(drfe_lmap* db, drfe_lmap_create_call* call);
int drfe_lmap_create_device(drfe_lmap* db, drfe_lmap_create_call* call, void* stream);
int drfe_lmap_create_batch(drfe_lmap* db, drfe_lmap_create_call* call, void* stream);
/* out[0] creations of one workgroup of the device's launches (a chunk is a whole number of them), [1] lanes of a wavefront, [2]
 * bytes of scratch per stored row entry (its claim word), [3] bytes of scratch per creation of a chunk, [4] the workgroup size,
 * [5] 0, [6] DRFE_LMAP_CREATE_DEVICE_FROM, [7] 0 */
int drfe_lmap_create_limits(int32_t* out8);
/* the scratch a device call of n_points and n_lines creations takes: out[0] bytes with which each kind runs as one chunk, [1] the
 * least bytes with which it runs at all (one workgroup of creations a chunk), [2] the part every chunk shares (the claim words) */
int drfe_lmap_create_scratch(drfe_lmap* db, int32_t n_points, int32_t n_lines, int64_t* out3);
/* Counters since the store was created: stats[0] calls, [1] calls run on the device, [2] points created, [3] lines created,
 * [4] row entries displaced, [5] calls that left the image stale, [6] block relayouts, [7] chunks run on the device. */
int drfe_lmap_create_stats(drfe_lmap* db, int64_t* stats /* 8 */);

/* What surrounds the solver of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2894-3205, called at src/LoopClosing.cc:613)
 * on the same store: before it the vertices and the ordered edge list with their double Sim3 measurements (:2910-3080), after it
 * the pose of every key frame and the move of every map point with UpdateNormalAndDepth (:3088-3131).  The solver itself, a sparse
 * Cholesky with an ordering, stays with the caller, as the adjustment of section 29 does.  DESIGN.md section 35.  Parity with a
 * build of g2o's sim3.h is not pinned (no Eigen here): g2o::Sim3's product, inverse and map are read as in sections 22 and 27.
 * The store holds no line or plane geometry: map lines and planes (:3134-3204) are not touched, and the commit returns
 * vCorrectedSwc per key frame so that the caller moves them.
 *
 * mspLoopEdges per key frame, as handles.  The state is optional: a store that is never given it has empty rows and behaves as
 * before.  Rows are CSR (offsets[0] = 0, count + 1 entries); a row replaces the stored one and the last row of a handle wins; a
 * negative handle or a member named twice in a row: DRFE_ERR_INVALID, nothing changed.  A row may name key frames that are not
 * stored (yet); drfe_lmap_remove of a key frame drops its row.  The state lies in a device block of its own: an edit of it sends
 * no other block again (drfe_lmap_essential_upload_bytes). */
int drfe_lmap_set_loop_edges(drfe_lmap* db, int32_t count, const int32_t* handles, const int32_t* offsets, const int32_t* edges);
/* the rows of `count` stored key frames (an unknown handle: DRFE_ERR_INVALID), each in ascending rank, members that are not stored
 * last in ascending handle; offsets gets count + 1 entries; DRFE_ERR_CAPACITY when capacity holds fewer than offsets[count] */
int drfe_lmap_get_loop_edges(drfe_lmap* db, int32_t count, const int32_t* handles, int32_t capacity, int32_t* offsets, int32_t* edges);
/* host-to-device bytes of the loop-edge block since the store was created (the seventh block, next to drfe_lmap_upload_bytes) */
int drfe_lmap_essential_upload_bytes(drfe_lmap* db, int64_t* out1);

/* const int minFeat = 100 of the reference; not an argument */
enum { DRFE_LMAP_ESSENTIAL_MIN_FEAT = 100 };
/* drfe_lmap_essential_edges_call.kind */
enum { DRFE_LMAP_ESSENTIAL_LOOP_CONNECTION = 0, DRFE_LMAP_ESSENTIAL_SPANNING_TREE = 1, DRFE_LMAP_ESSENTIAL_LOOP_EDGE = 2,
       DRFE_LMAP_ESSENTIAL_COVISIBILITY = 3 };

/* The edge builder.  Handles are mnId, as everywhere on this store: every `mnId <` of the reference and the (min, max) pair of
 * sInsertedEdges are on handles.
 *
 * Kept from the reference.  The key frames of the map are the stored key frames that are not bad, in rank order; a stored bad key
 * frame gets no vertex and is walked by none of the loops.  vScw of a vertex is its `corrected` row when the table names it, else
 * Sim3(Rcw, tcw, 1.0) of the stored pose; `fixed` is set exactly for loop_kf.  Loop-connection edges come first, keys in rank
 * order and members in rank order: a member j of key i is skipped when (i != cur_kf || j != loop_kf) && GetWeight(i, j) < 100,
 * GetWeight read from i's stored weights row, 0 when absent; Sji = vScw[j] * vScw[i].inverse(); the pair enters the inserted set
 * only with its edge; non_corrected is not used.  Then one pass per key frame in rank order, Swi the inverse of its non_corrected
 * row when the table names it, else of vScw[i], and Sjw of the other end likewise: the parent edge when there is a parent; the
 * stored loop edges with a smaller handle in rank order; the edges of GetCovisiblesByWeight(100), which is the prefix of the
 * stored ordered row with weight >= 100, EMPTY when that prefix is the whole row (upper_bound returning end(),
 * src/KeyFrame.cc:268-270), in stored order, less every entry that is the parent, a child, a loop edge, bad, not of a smaller
 * handle or in the inserted set.
 *
 * Refused, and nothing is counted: DRFE_ERR_INVALID for a handle that stands twice in the table, a key that stands twice in
 * lc_handles or a member twice in its row; DRFE_ERR_STATE for loop_kf or cur_kf unknown, for a key or member of the loop
 * connections that is not stored, for a key frame of the map without a pose that the table does not name, and, with a message that
 * names the edge, for every edge the reference would add to a null vertex: a parent, a loop edge of a smaller handle or a kept
 * loop-connection member that is bad (a loop edge: or not stored), and a kept member of a bad key; DRFE_ERR_CAPACITY for an output
 * array that is too small.  A call never changes the store. */
typedef struct drfe_lmap_essential_edges_call {
    int32_t loop_kf, cur_kf;
    /* LoopClosing::KeyFrameAndPose, both tables over the same handles, each once; a handle that is not stored is ignored */
    int32_t n_sim3;
    int32_t n_lc;                     /* keys of LoopConnections */
    const int32_t* sim3_handles;
    const double* corrected;          /* 8 each, the layout of drfe_lmap_correct_out: qx qy qz qw tx ty tz s */
    const double* non_corrected;
    const int32_t* lc_handles;        /* n_lc, any order */
    const int32_t* lc_offsets;        /* n_lc + 1 */
    const int32_t* lc_kfs;            /* the members, any order */
    int32_t vertices_capacity;        /* the number of stored key frames always suffices */
    int32_t edges_capacity;           /* lc_offsets[n_lc] + the stored key frames + the entries of their loop-edge rows and of
                                       * their ordered rows always suffices */
    /* per vertex, in rank order */
    int32_t* n_vertices;              /* 1 */
    int32_t* vertices;                /* handles */
    double* Scw;                      /* 8 each: the estimate the vertex is given */
    uint8_t* fixed;
    /* per edge, in the order of the reference's addEdge: the host solver sums in it */
    int32_t* n_edges;                 /* 1 */
    int32_t* from;                    /* vertex 0, i */
    int32_t* to;                      /* vertex 1, j */
    double* measurement;              /* 8 each: Sji */
    uint8_t* kind;
} drfe_lmap_essential_edges_call;

/* The tail.  The call names every stored key frame that is not bad once (one missing, or a named bad one: DRFE_ERR_STATE; an
 * unknown or repeated handle: DRFE_ERR_INVALID) with the Scw the edges call returned and `optimised`, the estimates after the
 * solver.
 *
 * Kept from the reference.  Per key frame vCorrectedSwc = optimised.inverse() and the pose toCvSE3(r.toRotationMatrix(), t * (1. /
 * s)), Ow and Twc as SetPose derives them.  Then every stored point in slot order, bad ones skipped: nIDr = corrected_ref when
 * corrected_by == cur_kf, else the reference key frame's handle; the new position is (float) vCorrectedSwc[nIDr].map(vScw[nIDr].map(
 * (double) X)); an nIDr that is a stored key frame the call does not name goes through default-constructed Sim3s by the same
 * arithmetic (which turns -0.0 into 0.0).  Then UpdateNormalAndDepth at the new position over the observations in stored order,
 * every named observer at its new centre and every other at its stored one, ref_level and the scales as drfe_lmap_correct_* uses
 * them; a point without observations still moves, with status 0.  The stamps are not changed.
 *
 * Refused with DRFE_ERR_STATE and the item's name, and nothing changes: a point that is not bad without geometry, with an unknown
 * reference key frame, with an nIDr that is not a stored key frame (an out-of-range read in the reference), with ref_level out of
 * range or no scales, and, when it has observations, an observer or reference key frame the call does not name that has no pose.
 * DRFE_ERR_CAPACITY when points_capacity is too small.  On success the call commits poses and positions into the rows and, on the
 * device, into the resident geometry block in place, with no upload of what it wrote. */
typedef struct drfe_lmap_essential_commit_call {
    int32_t cur_kf;
    int32_t n;
    const int32_t* handles;
    const double* Scw;                /* n x 8 */
    const double* optimised;          /* n x 8 */
    int32_t points_capacity;          /* the number of stored points always suffices */
    int32_t pad;
    /* per named key frame, in the caller's order */
    float* Tiw;                       /* 16 each: what SetPose received */
    double* Swc;                      /* 8 each: vCorrectedSwc, for the caller's map lines and planes */
    /* per moved point, in ascending slot (ascending handle) */
    int32_t* n_points;                /* 1 */
    int32_t* points;                  /* handles */
    int32_t* ref;                     /* nIDr */
    float* world;                     /* 3 each */
    float* normal;                    /* 3 each */
    float* max_distance;
    float* min_distance;
    uint8_t* status;                  /* DRFE_UPKEEP_NORMAL, or 0 for a point without observations */
} drfe_lmap_essential_commit_call;

/* stored key frames from which drfe_lmap_essential_edges_batch, and stored points from which drfe_lmap_essential_commit_batch, of
 * a store with a context use the device: the measured crossovers (profiles/essential_timing.jsonl: the
 * smallest measured shape from which the device entry wins at every mix, the setters that precede a call included).  INT32_MAX:
 * the device entry won at no measured shape, _batch stays on the host.
 * Measured host time over device time: edges 0.35x to 0.52x at 100, 0.66x to 0.82x at 1000, 1.01x to 2.01x at 4000 key frames;
 * commit 1.72x to 1.93x at 12500, 2.18x to 2.51x at 125000, 2.02x to 2.27x at 500000 points. */
enum { DRFE_LMAP_ESSENTIAL_EDGES_DEVICE_FROM = 2147483647, DRFE_LMAP_ESSENTIAL_COMMIT_DEVICE_FROM = 12500 };
/* _host always runs on the host, _device always on the device (DRFE_ERR_STATE without a context; DRFE_ERR_CAPACITY when the call
 * - an edges call as a whole, a commit call with one point slot a chunk - does not fit the configured scratch), _batch on the
 * device from the crossover when the call fits.  All three return the same bytes and leave the same store. */
int drfe_lmap_essential_edges_host(drfe_lmap* db, drfe_lmap_essential_edges_call* call);
int drfe_lmap_essential_edges_device(drfe_lmap* db, drfe_lmap_essential_edges_call* call, void* stream);
int drfe_lmap_essential_edges_batch(drfe_lmap* db, drfe_lmap_essential_edges_call* call, void* stream);
int drfe_lmap_essential_commit_host(drfe_lmap* db, drfe_lmap_essential_commit_call* call);
int drfe_lmap_essential_commit_device(drfe_lmap* db, drfe_lmap_essential_commit_call* call, void* stream);
int drfe_lmap_essential_commit_batch(drfe_lmap* db, drfe_lmap_essential_commit_call* call, void* stream);
/* out[0] threads of a workgroup = point slots of one, [1] lanes of a wavefront = ordered-row entries of one pass, [2]
 * DRFE_LMAP_ESSENTIAL_EDGES_DEVICE_FROM, [3] DRFE_LMAP_ESSENTIAL_COMMIT_DEVICE_FROM, [4] bytes of scratch per point slot of a
 * commit chunk, [5] per stored key frame of a commit call, [6] per edge of the bound of an edges call, [7] per stored key frame of
 * an edges call */
int drfe_lmap_essential_limits(int32_t* out8);
/* the scratch the device calls take on the store as it is: out[0] bytes of an edges call with lc_entries loop-connection members
 * (it runs as a whole), [1] the part of it that does not depend on the edges, [2] bytes with which a commit call runs as one chunk,
 * [3] the least with which it runs at all (one point slot a chunk), [4] the part every chunk shares, [5] the edges of the bound */
int drfe_lmap_essential_scratch(drfe_lmap* db, int32_t lc_entries, int64_t* out6);
/* Counters since the store was created: stats[0] edges calls, [1] commit calls, [2] calls of either run on the device, [3]
 * vertices, [4] edges, [5] points moved, [6] points moved through a default-constructed entry, [7] covisibility prefixes emptied
 * by the end() rule. */
int drfe_lmap_essential_stats(drfe_lmap* db, int64_t* stats /* 8 */);

/* ------------------------------------------------------------------------------------------------ */
/* measurement                                                                                       */
/* DRFE_STAGE_FAST = the first FAST launch (k_fast_cells_cols<8>: the cells of at most 8 rows per lane - the four large levels at
 * 640x480 - or the generic k_fast_cells over all cells); DRFE_STAGE_FAST_B = the second one (k_fast_cells_cols<12>, the rest). */
enum { DRFE_STAGE_PYRAMID = 0, DRFE_STAGE_FAST, DRFE_STAGE_QUADTREE, DRFE_STAGE_BLUR, DRFE_STAGE_DESC,
       DRFE_STAGE_GLUE, DRFE_STAGE_MATCH, DRFE_STAGE_FAST_B, DRFE_STAGE_COUNT };
/* How the FAST cells of a w x h frame split over the two launches: cells[2] and evaluated pixels[2] (sum of the cells'
 * (window - 6)^2 areas: every pixel of the detection region belongs to exactly one cell).  Host code. */
int drfe_orb_fast_partition(drfe_ctx* ctx, int w, int h, int32_t* cells, int64_t* pixels);
/* The FAST cell table of a w x h frame in launch order, DRFE_FAST_CELL_FIELDS int32 per cell: level, window x0, y0 (level
 * coordinates), window width, height, offX, offY (what is added to a candidate's window coordinates less 3), cellIdx (emission order
 * inside the level), then the lane layout of k_fast_cells_cols - ncp column pairs, rpl rows per lane, nrb row blocks -, the kernel the
 * cell runs (8 / 12: k_fast_cells_cols<8> / <12>, 0: the generic k_fast_cells) and the survivor-list capacity of that launch (0 for
 * the generic kernel).  cap = 0: only *n is set.  Host code: no kernel, no device memory. */
#define DRFE_FAST_CELL_FIELDS 13
int drfe_orb_fast_cells(drfe_ctx* ctx, int w, int h, int32_t* rows, int cap, int* n);
/* When enabled, batched calls bracket every stage with HIP events on the launch stream. */
int drfe_profile_enable(drfe_ctx* ctx, int on);
/* Milliseconds per stage of the most recent batched calls (synchronises). */
int drfe_profile_stage_ms(drfe_ctx* ctx, float* ms /* DRFE_STAGE_COUNT */);
int drfe_stream_sync(drfe_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* DRFE_H */
