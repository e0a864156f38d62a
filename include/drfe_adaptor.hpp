/* drfe_adaptor.hpp — header-only C++ adaptor: the reference's class interfaces over the C-ABI of drfe.h.
 *
 * What a DR-SLAM maintainer drops in place of src/ORBextractor.cc, src/LSDextractor.cpp and src/PlaneExtractor.cpp
 * (INTEGRATION.md): same class names, constructor arguments, methods and public members as
 *   Planar_SLAM::ORBextractor          include/ORBextractor.h:51-85
 *   LineSegment::ExtractLineSegment    include/LSDextractor.h:342-350
 *   Planar_SLAM::PlaneDetection        include/PlaneExtractor.h:61-82
 *   Planar_SLAM::PlaneDetection_CAPE   include/PlaneExtractor.h:84-115
 *   Planar_SLAM::ORBmatcher            include/ORBmatcher.h:41-84  - the reference's thirteen signatures (templates over Frame / KeyFrame / MapPoint)
 *   Planar_SLAM::LSDmatcher            include/LSDmatcher.h:21-36  - the reference's ten signatures (templates over Frame / KeyFrame / MapLine)
 *   drfe::TrackManhattanFrame          src/Tracking.cc:1336          - Tracking's Manhattan-frame tracker (host entry)
 *   Planar_SLAM::PlaneMatcher          include/PlaneMatcher.h:10-31  - SearchMapByCoefficients and bMatchStatus (host entries)
 *   drfe::FlagMatchedPlanePoints       src/Map.cc:406-431            - Map::FlagMatchedPlanePoints (host entry)
 *   drfe::UpdateCoefficientsAndPoints  src/MapPlane.cc:298-371       - both forms of MapPlane's cloud upkeep (host entries)
 *   drfe::UpkeepMapPoint / UpkeepMapLine / MapUpkeep  src/MapPoint.cc:288-411, src/MapLine.cpp:241-362 - descriptor and
 *                                      normal upkeep of map points and lines (host entries; MapUpkeep: the device batch)
 *   drfe::TriangulateNewMapPoints / TriangulateNewMapLines / Triangulation  src/LocalMapping.cc:383-538, 875-1026 - the
 *                                      per-match triangulation of CreateNewMapPoints / CreateNewMapLines2 (Triangulation: device)
 *   Planar_SLAM::PnPsolver / drfe::PnPBatch  include/PnPsolver.h - relocalisation's EPnP RANSAC as a walk over a finished
 *                                      table with Refine's results (host entry; PnPBatch: every solver of a call at once)
 *   Planar_SLAM::Sim3Solver / drfe::Sim3Batch  include/Sim3Solver.h:35-130 - the loop closer's Sim3 RANSAC as a walk over a
 *                                      finished hypothesis table (host entry; Sim3Batch: every solver of a call on the device)
 *   Planar_SLAM::Initializer           include/Initializer.h         - monocular initialisation's H / F RANSAC and reconstruction
 *                                      (the point-only Initialize; one device call, or the host entry)
 *   drfe::Line3DBatch                  src/Frame.cc:481-558          - Frame::isLineGood's mvDepthLine / mvLines3D for the
 *                                      frames of a batch (one device call; the host entry below the crossover)
 * With -DDRFE_WITH_OPENCV the container types are OpenCV's (cv::Mat, cv::KeyPoint, cv::line_descriptor::KeyLine);
 * without it (this image has no OpenCV) minimal stand-ins with the same member names and memory layout are used, so the
 * header is compiled and exercised here (tests/native/adaptor_caller.cpp, run by tests/test_gpu_native.py).
 * Compiled against nothing but drfe.h; link with -ldrfe.  Errors of the C-ABI become std::runtime_error, as the
 * reference's constructors would throw; operator() keeps the reference's silent return on an empty image. */
#ifndef DRFE_ADAPTOR_HPP
#define DRFE_ADAPTOR_HPP

#include "drfe.h"

#include <cassert>
#include <cmath>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef DRFE_WITH_OPENCV
#include <opencv2/core/core.hpp>
#include <opencv2/line_descriptor/descriptor.hpp>
namespace drfe_cv {
using Mat = cv::Mat;
using KeyPoint = cv::KeyPoint;
using KeyLine = cv::line_descriptor::KeyLine;
inline const uint8_t* mat_data(const Mat& m) { return m.data; }
inline size_t mat_step(const Mat& m) { return m.step; }
inline Mat mat_u8(int rows, int cols) { return Mat(rows, cols, CV_8U); }
}  // namespace drfe_cv
#else
namespace drfe_cv {
struct Point2f { float x, y; };
/* cv::KeyPoint: pt, size, angle, response, octave, class_id (7 x 4 bytes) */
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id; };
/* the fields of cv::line_descriptor::KeyLine, in its declaration order */
struct KeyLine {
    float angle; int class_id, octave; Point2f pt; float response, size;
    float startPointX, startPointY, endPointX, endPointY, sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
    float lineLength; int numOfPixels;
};
/* continuous single-channel 8-bit matrix: the subset of cv::Mat the adaptor touches */
struct Mat {
    int rows = 0, cols = 0; size_t step = 0; uint8_t* data = nullptr; int elem = 1;
    std::shared_ptr<std::vector<uint8_t>> own;
    Mat() {}
    Mat(int r, int c, int elemSize = 1) : rows(r), cols(c), step((size_t)c * elemSize), elem(elemSize),
                                          own(std::make_shared<std::vector<uint8_t>>((size_t)r * c * elemSize)) { data = own->data(); }
    Mat(int r, int c, uint8_t* external, size_t stepBytes, int elemSize = 1) : rows(r), cols(c), step(stepBytes), data(external), elem(elemSize) {}
    bool empty() const { return rows == 0 || cols == 0 || !data; }
    void release() { rows = cols = 0; step = 0; data = nullptr; own.reset(); }
    template <class T> T* ptr(int r) { return reinterpret_cast<T*>(data + (size_t)r * step); }
    template <class T> const T* ptr(int r) const { return reinterpret_cast<const T*>(data + (size_t)r * step); }
};
inline const uint8_t* mat_data(const Mat& m) { return m.data; }
inline size_t mat_step(const Mat& m) { return m.step; }
inline Mat mat_u8(int rows, int cols) { return Mat(rows, cols); }
}  // namespace drfe_cv
#endif

/* Eigen::Vector3d where Eigen is present (VertexType of include/PlaneExtractor.h:30, keylineFunctions of include/LSDextractor.h:349);
 * a three-double stand-in with the same operator[] / operator() / layout otherwise (this image has no Eigen) */
#ifdef DRFE_WITH_EIGEN
#include <Eigen/Dense>
namespace drfe_cv { using Vector3d = Eigen::Vector3d; }
#else
namespace drfe_cv {
struct Vector3d {
    double v[3];
    Vector3d() : v{0, 0, 0} {}
    Vector3d(double x, double y, double z) : v{x, y, z} {}
    double& operator[](int i) { return v[i]; }
    const double& operator[](int i) const { return v[i]; }
    double& operator()(int i) { return v[i]; }
    const double& operator()(int i) const { return v[i]; }
    double x() const { return v[0]; }
    double y() const { return v[1]; }
    double z() const { return v[2]; }
};
}  // namespace drfe_cv
#endif
static_assert(sizeof(drfe_cv::Vector3d) == 3 * sizeof(double), "Vector3d is three doubles");

static_assert(sizeof(drfe_cv::KeyPoint) == sizeof(drfe_keypoint), "cv::KeyPoint and drfe_keypoint must share one layout");
#ifndef DRFE_WITH_OPENCV
static_assert(sizeof(drfe_cv::KeyLine) == sizeof(drfe_keyline), "KeyLine stand-in and drfe_keyline must share one layout");
#endif

namespace Planar_SLAM {

namespace drfe_detail {
inline void check(int rc, drfe_ctx* c, const char* what)
{
    if (rc != DRFE_OK) throw std::runtime_error(std::string(what) + ": " + drfe_last_error(c));
}
struct CtxDeleter { void operator()(drfe_ctx* c) const { drfe_destroy(c); } };
using CtxPtr = std::shared_ptr<drfe_ctx>;
inline CtxPtr make_ctx(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int maxW, int maxH, int maxBatch,
                       int device)
{
    drfe_config cfg = {device, maxW, maxH, maxBatch, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST};
    drfe_ctx* c = nullptr;
    if (drfe_create(&cfg, &c) != DRFE_OK) throw std::runtime_error(std::string("drfe_create: ") + drfe_last_error(nullptr));
    return CtxPtr(c, CtxDeleter());
}
/* the context the calling thread's matchers / line extractor work on (ORBmatcher::BindThread, LSDmatcher::BindThread) */
inline drfe_ctx*& thread_ctx() { static thread_local drfe_ctx* c = nullptr; return c; }
}  // namespace drfe_detail

/* include/ORBextractor.h:51-85 */
class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    /* slots: frame slots of the context - 1 for the plain operator(), >= 2 for the pipelined Submit / Collect flow in which
     * LastFrame stays on the device for the slot-pair matchers */
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int maxWidth = 640, int maxHeight = 480,
                 int device = 0, int slots = 1)
        : nfeatures(nfeatures), scaleFactor(scaleFactor), nlevels(nlevels), iniThFAST(iniThFAST), minThFAST(minThFAST),
          mCtx(drfe_detail::make_ctx(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, maxWidth, maxHeight, slots, device))
    {
        mvScaleFactor.resize(nlevels); mvInvScaleFactor.resize(nlevels);
        mvLevelSigma2.resize(nlevels); mvInvLevelSigma2.resize(nlevels);
        drfe_detail::check(drfe_orb_scale_tables(mCtx.get(), mvScaleFactor.data(), mvInvScaleFactor.data(), mvLevelSigma2.data(),
                                                 mvInvLevelSigma2.data()), mCtx.get(), "drfe_orb_scale_tables");
        mvImagePyramid.resize(nlevels);
    }
    ~ORBextractor() {}

    /* Compute the ORB features and descriptors on an image; the mask is ignored (include/ORBextractor.h:60-65) */
    void operator()(const drfe_cv::Mat& image, const drfe_cv::Mat& /*mask*/, std::vector<drfe_cv::KeyPoint>& keypoints,
                    drfe_cv::Mat& descriptors)
    {
        if (image.empty()) return;                                       /* src/ORBextractor.cc:1046-1047 */
        const int cap = drfe_orb_max_keypoints(mCtx.get());
        keypoints.resize(cap);
        drfe_cv::Mat desc = drfe_cv::mat_u8(cap, 32);
        int n = 0;
        drfe_detail::check(drfe_orb_extract(mCtx.get(), drfe_cv::mat_data(image), image.cols, image.rows, drfe_cv::mat_step(image),
                                            reinterpret_cast<drfe_keypoint*>(keypoints.data()), desc.data, cap, &n),
                           mCtx.get(), "drfe_orb_extract");
        keypoints.resize(n);
        if (n == 0) { descriptors.release(); return; }                   /* :1064-1065 */
        descriptors = drfe_cv::mat_u8(n, 32);
        std::memcpy(descriptors.data, desc.data, (size_t)n * 32);
        /* public member mvImagePyramid (include/ORBextractor.h:85): interior ROI views of the bordered levels */
        mvPyramidStore.resize(nlevels);
        for (int l = 0; l < nlevels; ++l) {
            int bw = 0, bh = 0;
            drfe_detail::check(drfe_orb_pyramid_level(mCtx.get(), 0, l, nullptr, &bw, &bh), mCtx.get(), "drfe_orb_pyramid_level");
            mvPyramidStore[l] = drfe_cv::mat_u8(bh, bw);
            drfe_detail::check(drfe_orb_pyramid_level(mCtx.get(), 0, l, mvPyramidStore[l].data, &bw, &bh), mCtx.get(),
                               "drfe_orb_pyramid_level");
#ifdef DRFE_WITH_OPENCV
            mvImagePyramid[l] = mvPyramidStore[l](cv::Rect(19, 19, bw - 38, bh - 38));
#else
            mvImagePyramid[l] = drfe_cv::Mat(bh - 38, bw - 38, mvPyramidStore[l].data + 19 * (size_t)bw + 19, (size_t)bw);
#endif
        }
    }

    /* The same extraction without waiting for it (drfe_frame_submit / drfe_frame_collect): Frame::Frame calls Submit where it
     * started the ExtractORB thread (src/Frame.cc:124), runs ExtractLSD / ComputePlanes on the calling thread, then Collect where
     * it joined.  With a depth image (CV_16U, as Tracking hands imDepth before its convertTo) and the camera, the glue
     * (UndistortKeyPoints, ComputeStereoFromRGBD, AssignFeaturesToGrid) runs in the same submission and mvuRight / mvDepth
     * come back with the keypoints. */
    void Submit(int slot, const drfe_cv::Mat& image, const uint16_t* depth16 = nullptr, size_t depthStrideElems = 0,
                const drfe_camera* cam = nullptr)
    {
        drfe_detail::check(drfe_frame_submit(mCtx.get(), slot, drfe_cv::mat_data(image), image.cols, image.rows, drfe_cv::mat_step(image),
                                             depth16, depthStrideElems, cam), mCtx.get(), "drfe_frame_submit");
    }
    void Collect(int slot, std::vector<drfe_cv::KeyPoint>& keypoints, drfe_cv::Mat& descriptors, std::vector<float>* mvuRight = nullptr,
                 std::vector<float>* mvDepth = nullptr)
    {
        const int cap = drfe_orb_max_keypoints(mCtx.get());
        keypoints.resize(cap);
        drfe_cv::Mat desc = drfe_cv::mat_u8(cap, 32);
        if (mvuRight) mvuRight->resize(cap);
        if (mvDepth) mvDepth->resize(cap);
        int n = 0;
        drfe_detail::check(drfe_frame_collect(mCtx.get(), slot, reinterpret_cast<drfe_keypoint*>(keypoints.data()), desc.data,
                                              mvuRight ? mvuRight->data() : nullptr, mvDepth ? mvDepth->data() : nullptr, cap, &n),
                           mCtx.get(), "drfe_frame_collect");
        keypoints.resize(n);
        if (mvuRight) mvuRight->resize(n);
        if (mvDepth) mvDepth->resize(n);
        if (n == 0) { descriptors.release(); return; }
        descriptors = drfe_cv::mat_u8(n, 32);
        std::memcpy(descriptors.data, desc.data, (size_t)n * 32);
    }

    /* One submission per tracked frame (drfe_frame_submit_tracked): what Frame::Frame extracts AND what TrackWithMotionModel's
     * ORBmatcher(0.9, true).SearchByProjection(mCurrentFrame, mLastFrame, th, mono) returns (src/Tracking.cc:2181-2202), in one
     * captured graph.  TcwCur = mVelocity * mLastFrame.mTcw; lastMapPoints = mLastFrame.mvpMapPoints flattened to drfe_map_point
     * records (NULL: the RGB-D temporal points, built on the device from LastFrame's depth and TwcLast).  CollectTracked fills
     * matches[i] = index into LastFrame of the map point current keypoint i received, -1 = none, and returns nmatches. */
    void SubmitTracked(int slot, const drfe_cv::Mat& image, const uint16_t* depth16, size_t depthStrideElems, const drfe_camera& cam,
                       int lastSlot, const float* TcwCur, const float* TcwLast, const float* TwcLast, const drfe_map_point* lastMapPoints,
                       int nLast, float th, bool mono, bool checkOrientation = true)
    {
        drfe_detail::check(drfe_frame_submit_tracked(mCtx.get(), slot, drfe_cv::mat_data(image), image.cols, image.rows, drfe_cv::mat_step(image),
                                                     depth16, depthStrideElems, &cam, lastSlot, TcwCur, TcwLast, TwcLast, lastMapPoints, nLast,
                                                     th, mono ? 1 : 0, checkOrientation ? 1 : 0),
                           mCtx.get(), "drfe_frame_submit_tracked");
    }
    int CollectTracked(int slot, std::vector<drfe_cv::KeyPoint>& keypoints, drfe_cv::Mat& descriptors, std::vector<float>& mvuRight,
                       std::vector<float>& mvDepth, std::vector<int32_t>& matches)
    {
        const int cap = drfe_orb_max_keypoints(mCtx.get());
        keypoints.resize(cap); mvuRight.resize(cap); mvDepth.resize(cap); matches.assign(cap, -1);
        drfe_cv::Mat desc = drfe_cv::mat_u8(cap, 32);
        int n = 0, nmatches = 0;
        drfe_detail::check(drfe_frame_collect_tracked(mCtx.get(), slot, reinterpret_cast<drfe_keypoint*>(keypoints.data()), desc.data,
                                                      mvuRight.data(), mvDepth.data(), cap, &n, matches.data(), &nmatches),
                           mCtx.get(), "drfe_frame_collect_tracked");
        keypoints.resize(n); mvuRight.resize(n); mvDepth.resize(n); matches.resize(n);
        if (n == 0) { descriptors.release(); return 0; }
        descriptors = drfe_cv::mat_u8(n, 32);
        std::memcpy(descriptors.data, desc.data, (size_t)n * 32);
        return nmatches;
    }

    int inline GetLevels() { return nlevels; }
    float inline GetScaleFactor() { return scaleFactor; }
    std::vector<float> inline GetScaleFactors() { return mvScaleFactor; }
    std::vector<float> inline GetInverseScaleFactors() { return mvInvScaleFactor; }
    std::vector<float> inline GetScaleSigmaSquares() { return mvLevelSigma2; }
    std::vector<float> inline GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }

    std::vector<drfe_cv::Mat> mvImagePyramid;

    drfe_ctx* context() { return mCtx.get(); }        /* for the Frame glue / matcher adaptors that share the device state */

protected:
    int nfeatures; double scaleFactor; int nlevels; int iniThFAST; int minThFAST;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
    std::vector<drfe_cv::Mat> mvPyramidStore;
    drfe_detail::CtxPtr mCtx;
};

/* ---------------------------------------------------------------------------------------------------------------------------
 * ORBmatcher (include/ORBmatcher.h:41-84, src/ORBmatcher.cc) with the reference's thirteen signatures.
 *
 * The reference's matchers take Frame& / KeyFrame* / MapPoint* - objects of the map, on the host.  Every method here
 *   1. makes its frames resident in a device slot (MatcherDevice: a small LRU over the slots of one drfe_ctx; a frame that is
 *      not there yet is uploaded from its own members - mvKeys, mvKeysUn, mDescriptors, mvuRight, mvDepth - by drfe_frame_load,
 *      which rebuilds its 64 x 48 grid on the device; a frame is recognised by its type and mnId),
 *   2. flattens what the reference's loop reads through the pointers (GetWorldPos, GetDescriptor, Observations, isBad, the
 *      fields Frame::isInFrustum left on the point, ...) into the records of drfe.h,
 *   3. calls the C entry point (window gathers, Hamming distances, claim order, rotation histogram: on the device),
 *   4. turns the returned indices back into pointers and applies the graph surgery (Replace / AddObservation / AddMapPoint)
 *      in the reference's order on the host - that part touches mutex-protected map objects and stays where they live.
 * The methods are templates over the frame / keyframe / map point types and only use the member names src/ORBmatcher.cc uses, so
 * they bind to Planar_SLAM::Frame, KeyFrame and MapPoint as they are (cv::Mat members are read through .data: continuous
 * CV_32F / CV_8U matrices, as the reference creates them) and to the stand-ins of tests/native/matcher_caller.cpp.
 *
 * Threading: the reference constructs matchers on the stack of three threads (Tracking, LocalMapping, LoopClosing).  Each thread
 * binds its own MatcherDevice once (ORBmatcher::BindThread); a matcher object itself holds two scalars, as in the reference. */

namespace drfe_detail {
template <class M> inline const float* f32(const M& m) { return reinterpret_cast<const float*>(m.data); }
template <class M> inline const uint8_t* u8(const M& m) { return reinterpret_cast<const uint8_t*>(m.data); }
template <class T> struct TypeTag { static const char v; };
template <class T> const char TypeTag<T>::v = 0;
/* camera block of a Frame or KeyFrame: fx fy cx cy mbf and the image bounds (Frame: static floats; KeyFrame: const members, the
 * bounds as ints - include/KeyFrame.h:230-233) */
template <class F> inline drfe_camera camera_of(const F& f)
{
    drfe_camera c;
    c.fx = f.fx; c.fy = f.fy; c.cx = f.cx; c.cy = f.cy; c.bf = f.mbf; c.depth_factor = 0.f;
    c.min_x = (float)f.mnMinX; c.max_x = (float)f.mnMaxX; c.min_y = (float)f.mnMinY; c.max_y = (float)f.mnMaxY;
    return c;
}
template <class MP> inline void frustum_of(MP* p, drfe_frustum_point& o, uint8_t* desc32)
{
    const auto w = p->GetWorldPos(); std::memcpy(o.world, w.data, 12);
    const auto n = p->GetNormal(); std::memcpy(o.normal, n.data, 12);
    o.min_distance = p->GetMinDistanceInvariance(); o.max_distance = p->GetMaxDistanceInvariance();
    const auto d = p->GetDescriptor(); std::memcpy(desc32, d.data, 32);
}
}  // namespace drfe_detail

/* The slots of one drfe_ctx as a cache of host frames. */
class MatcherDevice {
public:
    /* ORB parameters as the extractor's (they size a slot: drfe_orb_max_keypoints, and give the scale tables the searches use) */
    MatcherDevice(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int slots = 8, int maxWidth = 640,
                  int maxHeight = 480, int device = 0)
        : mCtx(drfe_detail::make_ctx(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, maxWidth, maxHeight, slots, device)), mSlots((size_t)slots)
    {
    }
    drfe_ctx* ctx() const { return mCtx.get(); }
    /* ORBVocabulary for SearchByBoW / SearchForTriangulation: the nodes as TemplatedVocabulary::loadFromTextFile holds them */
    void UploadVocabulary(int k, int L, int scoring, int weighting, int nNodes, const int32_t* parent, const uint8_t* desc, const double* weight,
                          const uint8_t* isLeaf, int levelsup = 4)
    {
        drfe_detail::check(drfe_voc_upload(mCtx.get(), k, L, scoring, weighting, nNodes, parent, desc, weight, isLeaf), mCtx.get(), "drfe_voc_upload");
        mLevelsUp = levelsup; mHaveVoc = true;
        for (Slot& s : mSlots) s.bow = false;
    }
    /* slot of a frame, loading it when absent; `keep` (another frame's slot of the same call, or -1) is never evicted */
    template <class F> int Resident(const F& f, bool needBow = false, int keep = -1)
    {
        const void* tag = &drfe_detail::TypeTag<F>::v;
        int at = -1;
        for (size_t i = 0; i < mSlots.size(); i++) if (mSlots[i].tag == tag && mSlots[i].id == (unsigned long)f.mnId) { at = (int)i; break; }
        if (at < 0) {
            unsigned long oldest = ~0ul;
            for (size_t i = 0; i < mSlots.size(); i++) if ((int)i != keep && mSlots[i].stamp < oldest) { oldest = mSlots[i].stamp; at = (int)i; }
            if (at < 0) throw std::runtime_error("MatcherDevice: no free slot");
            const drfe_camera cam = drfe_detail::camera_of(f);
            const int n = (int)f.mvKeys.size();
            static_assert(sizeof(f.mvKeys[0]) == sizeof(drfe_keypoint), "cv::KeyPoint layout");
            drfe_detail::check(drfe_frame_load(mCtx.get(), at, reinterpret_cast<const drfe_keypoint*>(f.mvKeys.data()),
                                               reinterpret_cast<const drfe_keypoint*>(f.mvKeysUn.data()), drfe_detail::u8(f.mDescriptors),
                                               f.mvuRight.empty() ? nullptr : f.mvuRight.data(), f.mvDepth.empty() ? nullptr : f.mvDepth.data(), n, &cam),
                               mCtx.get(), "drfe_frame_load");
            mSlots[(size_t)at].tag = tag; mSlots[(size_t)at].id = (unsigned long)f.mnId; mSlots[(size_t)at].bow = false;
            mLoads++;
        }
        Slot& s = mSlots[(size_t)at];
        s.stamp = ++mClock;
        if (needBow && !s.bow) {
            if (!mHaveVoc) throw std::runtime_error("MatcherDevice: this matcher needs the vocabulary (UploadVocabulary)");
            drfe_detail::check(drfe_bow_transform_slot(mCtx.get(), mLevelsUp, at, nullptr), mCtx.get(), "drfe_bow_transform_slot");
            s.bow = true;
        }
        return at;
    }
    /* a frame whose keypoints changed in place (never in the reference; a test may) */
    void Forget() { for (Slot& s : mSlots) { s.tag = nullptr; s.stamp = 0; s.bow = false; } }
    unsigned long loads() const { return mLoads; }
private:
    struct Slot { const void* tag = nullptr; unsigned long id = 0, stamp = 0; bool bow = false; };
    drfe_detail::CtxPtr mCtx;
    std::vector<Slot> mSlots;
    unsigned long mClock = 0, mLoads = 0;
    int mLevelsUp = 4; bool mHaveVoc = false;
};

class ORBmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    /* the calling thread's device (Tracking / LocalMapping / LoopClosing bind one each at start-up) */
    static void BindThread(MatcherDevice* dev) { tls() = dev; drfe_detail::thread_ctx() = dev ? dev->ctx() : nullptr; }
    static MatcherDevice& Device()
    {
        if (!tls()) throw std::runtime_error("ORBmatcher: no MatcherDevice bound to this thread (ORBmatcher::BindThread)");
        return *tls();
    }

    /* src/ORBmatcher.cc:1712-1728 */
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b)
    {
        int dist = 0;
        for (int i = 0; i < 8; i++) {
            uint32_t pa, pb;
            std::memcpy(&pa, a + 4 * i, 4); std::memcpy(&pb, b + 4 * i, 4);
            uint32_t v = pa ^ pb;
            v = v - ((v >> 1) & 0x55555555);
            v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
            dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
        }
        return dist;
    }
    static int DescriptorDistance(const drfe_cv::Mat& a, const drfe_cv::Mat& b) { return DescriptorDistance(drfe_detail::u8(a), drfe_detail::u8(b)); }

    /* ---- src/ORBmatcher.cc:46-130 - Tracking::SearchLocalPoints: the local map into the frame ---- */
    template <class FrameT, class MapPointT>
    int SearchByProjection(FrameT& F, const std::vector<MapPointT*>& vpMapPoints, const float th = 3)
    {
        MatcherDevice& D = Device();
        const int slot = D.Resident(F), m = (int)vpMapPoints.size(), N = (int)F.mvpMapPoints.size();
        std::vector<drfe_tracked_point> tp((size_t)m);
        for (int i = 0; i < m; i++) {
            MapPointT* p = vpMapPoints[(size_t)i];
            drfe_tracked_point& t = tp[(size_t)i];
            std::memset(&t, 0, sizeof(t));
            t.track_in_view = p->mbTrackInView ? 1 : 0;
            if (!t.track_in_view) continue;
            t.bad = p->isBad() ? 1 : 0;
            if (t.bad) continue;
            t.obs_positive = p->Observations() > 0 ? 1 : 0;
            t.level = p->mnTrackScaleLevel; t.proj_x = p->mTrackProjX; t.proj_y = p->mTrackProjY; t.proj_xr = p->mTrackProjXR; t.view_cos = p->mTrackViewCos;
            const auto d = p->GetDescriptor(); std::memcpy(t.desc, d.data, 32);
        }
        /* claims the frame already holds: any index >= m (never confused with a new match, which is an index into vpMapPoints) */
        std::vector<int32_t> claim((size_t)N);
        std::vector<uint8_t> obs((size_t)N);
        for (int i = 0; i < N; i++) { MapPointT* p = F.mvpMapPoints[(size_t)i]; claim[(size_t)i] = p ? m + i : -1; obs[(size_t)i] = p && p->Observations() > 0; }
        int n = 0;
        drfe_detail::check(drfe_search_by_projection_map(D.ctx(), slot, tp.data(), m, th, mfNNratio, obs.data(), claim.data(), N, &n), D.ctx(),
                           "drfe_search_by_projection_map");
        for (int i = 0; i < N; i++) if (claim[(size_t)i] >= 0 && claim[(size_t)i] < m) F.mvpMapPoints[(size_t)i] = vpMapPoints[(size_t)claim[(size_t)i]];
        return n;
    }

    /* ---- src/ORBmatcher.cc:1396-1535 - Tracking::TrackWithMotionModel ---- */
    template <class FrameT, class LastT>
    typename std::enable_if<std::is_class<LastT>::value, int>::type
    SearchByProjection(FrameT& CurrentFrame, const LastT& LastFrame, const float th, const bool bMono)
    {
        MatcherDevice& D = Device();
        const int cur = D.Resident(CurrentFrame), last = D.Resident(LastFrame, false, cur);
        const int nl = (int)LastFrame.mvpMapPoints.size(), nc = (int)CurrentFrame.mvpMapPoints.size();
        std::vector<drfe_map_point> mp((size_t)nl);
        for (int i = 0; i < nl; i++) {
            auto* p = LastFrame.mvpMapPoints[(size_t)i];
            drfe_map_point& r = mp[(size_t)i];
            std::memset(&r, 0, sizeof(r));
            r.valid = p && !LastFrame.mvbOutlier[(size_t)i];
            if (!r.valid) continue;
            r.obs_positive = p->Observations() > 0;
            const auto w = p->GetWorldPos(); std::memcpy(r.world, w.data, 12);
            const auto d = p->GetDescriptor(); std::memcpy(r.desc, d.data, 32);
        }
        std::vector<int32_t> claim((size_t)nc);
        std::vector<uint8_t> obs((size_t)nc);
        for (int i = 0; i < nc; i++) { auto* p = CurrentFrame.mvpMapPoints[(size_t)i]; claim[(size_t)i] = p ? nl + i : -1; obs[(size_t)i] = p && p->Observations() > 0; }
        const drfe_camera cam = drfe_detail::camera_of(CurrentFrame);
        int n = 0;
        drfe_detail::check(drfe_search_by_projection_last(D.ctx(), cur, last, drfe_detail::f32(CurrentFrame.mTcw), drfe_detail::f32(LastFrame.mTcw), &cam, mp.data(), nl,
                                                          th, bMono ? 1 : 0, mbCheckOrientation ? 1 : 0, obs.data(), claim.data(), nc, &n), D.ctx(),
                           "drfe_search_by_projection_last");
        for (int i = 0; i < nc; i++) {
            const int32_t v = claim[(size_t)i];
            if (v < 0) CurrentFrame.mvpMapPoints[(size_t)i] = nullptr;        /* also a match the rotation histogram took back (:1524) */
            else if (v < nl) CurrentFrame.mvpMapPoints[(size_t)i] = LastFrame.mvpMapPoints[(size_t)v];
        }
        return n;
    }

    /* ---- src/ORBmatcher.cc:1332-1394 - the brute-force fallback of TrackWithMotionModel (src/Tracking.cc:2195-2200) ---- */
    template <class FrameT, class LastT>
    int MatchORBPoints(FrameT& CurrentFrame, const LastT& LastFrame)
    {
        MatcherDevice& D = Device();
        const int cur = D.Resident(CurrentFrame), last = D.Resident(LastFrame, false, cur);
        const int nl = (int)LastFrame.mvpMapPoints.size(), nc = (int)CurrentFrame.mvpMapPoints.size();
        std::vector<int32_t> lastMp((size_t)nl), curMp((size_t)nc);
        std::vector<uint8_t> outl((size_t)nl);
        for (int i = 0; i < nl; i++) { lastMp[(size_t)i] = LastFrame.mvpMapPoints[(size_t)i] ? i : -1; outl[(size_t)i] = LastFrame.mvbOutlier[(size_t)i] ? 1 : 0; }
        for (int i = 0; i < nc; i++) curMp[(size_t)i] = CurrentFrame.mvpMapPoints[(size_t)i] ? nl + i : -1;
        int nPair = 0;
        drfe_detail::check(drfe_match_orb_points(D.ctx(), cur, last, lastMp.data(), outl.data(), nl, curMp.data(), nc, &nPair), D.ctx(), "drfe_match_orb_points");
        for (int i = 0; i < nc; i++) if (curMp[(size_t)i] >= 0 && curMp[(size_t)i] < nl) CurrentFrame.mvpMapPoints[(size_t)i] = LastFrame.mvpMapPoints[(size_t)curMp[(size_t)i]];
        return nPair;
    }

    /* ---- src/ORBmatcher.cc:1537-1664 - Tracking::Relocalization (src/Tracking.cc:3638, :3651) ---- */
    template <class FrameT, class KeyFrameT, class MapPointT>
    int SearchByProjection(FrameT& CurrentFrame, KeyFrameT* pKF, const std::set<MapPointT*>& sAlreadyFound, const float th, const int ORBdist)
    {
        MatcherDevice& D = Device();
        const int slot = D.Resident(CurrentFrame);
        const std::vector<MapPointT*> vpMPs = pKF->GetMapPointMatches();
        const int n = (int)vpMPs.size(), nc = (int)CurrentFrame.mvpMapPoints.size();
        std::vector<drfe_frustum_point> fp((size_t)n);
        std::vector<uint8_t> descs((size_t)n * 32), skip((size_t)n), matched((size_t)nc);
        std::vector<float> angles((size_t)n);
        for (int i = 0; i < n; i++) {
            MapPointT* p = vpMPs[(size_t)i];
            std::memset(&fp[(size_t)i], 0, sizeof(drfe_frustum_point));
            skip[(size_t)i] = !p || p->isBad() || sAlreadyFound.count(p);
            angles[(size_t)i] = pKF->mvKeysUn[(size_t)i].angle;
            if (!skip[(size_t)i]) drfe_detail::frustum_of(p, fp[(size_t)i], descs.data() + 32 * (size_t)i);
        }
        for (int k = 0; k < nc; k++) matched[(size_t)k] = CurrentFrame.mvpMapPoints[(size_t)k] != nullptr;
        std::vector<int32_t> nm((size_t)nc, -1);
        int cnt = 0;
        drfe_detail::check(drfe_search_by_projection_reloc(D.ctx(), slot, drfe_detail::f32(CurrentFrame.mTcw), fp.data(), descs.data(), angles.data(), skip.data(), n,
                                                           matched.data(), nc, th, ORBdist, mbCheckOrientation ? 1 : 0, nm.data(), &cnt), D.ctx(),
                           "drfe_search_by_projection_reloc");
        for (int k = 0; k < nc; k++) if (nm[(size_t)k] >= 0) CurrentFrame.mvpMapPoints[(size_t)k] = vpMPs[(size_t)nm[(size_t)k]];
        return cnt;
    }

    /* ---- src/ORBmatcher.cc:294-407 - LoopClosing::ComputeSim3 after the Sim3 optimisation ---- */
    template <class KeyFrameT, class MatT, class MapPointT>
    int SearchByProjection(KeyFrameT* pKF, MatT Scw, const std::vector<MapPointT*>& vpPoints, std::vector<MapPointT*>& vpMatched, int th)
    {
        MatcherDevice& D = Device();
        const int slot = D.Resident(*pKF);
        const int n = (int)vpPoints.size(), nk = (int)vpMatched.size();
        std::set<MapPointT*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
        spAlreadyFound.erase(static_cast<MapPointT*>(nullptr));
        std::vector<drfe_frustum_point> fp((size_t)n);
        std::vector<uint8_t> descs((size_t)n * 32), skip((size_t)n), matched((size_t)nk);
        for (int i = 0; i < n; i++) {
            MapPointT* p = vpPoints[(size_t)i];
            std::memset(&fp[(size_t)i], 0, sizeof(drfe_frustum_point));
            skip[(size_t)i] = p->isBad() || spAlreadyFound.count(p);
            if (!skip[(size_t)i]) drfe_detail::frustum_of(p, fp[(size_t)i], descs.data() + 32 * (size_t)i);
        }
        for (int k = 0; k < nk; k++) matched[(size_t)k] = vpMatched[(size_t)k] != nullptr;
        std::vector<int32_t> nm((size_t)nk, -1);
        int cnt = 0;
        drfe_detail::check(drfe_search_by_projection_kf(D.ctx(), slot, drfe_detail::f32(Scw), fp.data(), descs.data(), skip.data(), n, matched.data(), nk, (float)th,
                                                        nm.data(), &cnt), D.ctx(), "drfe_search_by_projection_kf");
        for (int k = 0; k < nk; k++) if (nm[(size_t)k] >= 0) vpMatched[(size_t)k] = vpPoints[(size_t)nm[(size_t)k]];
        return cnt;
    }

    /* ---- src/ORBmatcher.cc:160-292 - TrackReferenceKeyFrame / Relocalization ---- */
    template <class KeyFrameT, class FrameT, class MapPointT>
    typename std::enable_if<std::is_class<FrameT>::value, int>::type
    SearchByBoW(KeyFrameT* pKF, FrameT& F, std::vector<MapPointT*>& vpMapPointMatches)
    {
        MatcherDevice& D = Device();
        const int kf = D.Resident(*pKF, true), fs = D.Resident(F, true, kf);
        const std::vector<MapPointT*> vpMapPointsKF = pKF->GetMapPointMatches();
        const int nk = (int)vpMapPointsKF.size(), nf = (int)F.mvKeys.size();
        vpMapPointMatches = std::vector<MapPointT*>((size_t)nf, static_cast<MapPointT*>(nullptr));
        std::vector<int32_t> kfMp((size_t)nk), match((size_t)nf, -1);
        for (int i = 0; i < nk; i++) { MapPointT* p = vpMapPointsKF[(size_t)i]; kfMp[(size_t)i] = (p && !p->isBad()) ? i : -1; }
        int n = 0;
        drfe_detail::check(drfe_search_by_bow(D.ctx(), kf, fs, kfMp.data(), nk, mfNNratio, mbCheckOrientation ? 1 : 0, match.data(), nf, &n), D.ctx(),
                           "drfe_search_by_bow");
        for (int j = 0; j < nf; j++) if (match[(size_t)j] >= 0) vpMapPointMatches[(size_t)j] = vpMapPointsKF[(size_t)match[(size_t)j]];
        return n;
    }

    /* ---- src/ORBmatcher.cc:526-660 - LoopClosing::ComputeSim3 ---- */
    template <class KeyFrameT, class MapPointT>
    int SearchByBoW(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12)
    {
        MatcherDevice& D = Device();
        const int s1 = D.Resident(*pKF1, true), s2 = D.Resident(*pKF2, true, s1);
        const std::vector<MapPointT*> vp1 = pKF1->GetMapPointMatches(), vp2 = pKF2->GetMapPointMatches();
        const int n1 = (int)vp1.size(), n2 = (int)vp2.size();
        vpMatches12 = std::vector<MapPointT*>((size_t)n1, static_cast<MapPointT*>(nullptr));
        std::vector<int32_t> mp1((size_t)n1), mp2((size_t)n2), match2((size_t)n2, -1);
        for (int i = 0; i < n1; i++) mp1[(size_t)i] = (vp1[(size_t)i] && !vp1[(size_t)i]->isBad()) ? i : -1;
        for (int i = 0; i < n2; i++) mp2[(size_t)i] = (vp2[(size_t)i] && !vp2[(size_t)i]->isBad()) ? i : -1;
        int n = 0;
        drfe_detail::check(drfe_search_by_bow_kf(D.ctx(), s1, s2, mp1.data(), n1, mp2.data(), n2, mfNNratio, mbCheckOrientation ? 1 : 0, match2.data(), &n), D.ctx(),
                           "drfe_search_by_bow_kf");
        for (int i2 = 0; i2 < n2; i2++) if (match2[(size_t)i2] >= 0) vpMatches12[(size_t)match2[(size_t)i2]] = vp2[(size_t)i2];
        return n;
    }

    /* ---- src/ORBmatcher.cc:409-524 - Tracking::MonocularInitialization; PointT = cv::Point2f (two floats) ---- */
    template <class FrameT, class PointT>
    int SearchForInitialization(FrameT& F1, FrameT& F2, std::vector<PointT>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize = 10)
    {
        static_assert(sizeof(PointT) == 8, "cv::Point2f is two floats");
        MatcherDevice& D = Device();
        const int s1 = D.Resident(F1), s2 = D.Resident(F2, false, s1);
        const int n1 = (int)F1.mvKeysUn.size();
        vnMatches12.assign((size_t)n1, -1);
        if ((int)vbPrevMatched.size() != n1) throw std::runtime_error("SearchForInitialization: vbPrevMatched must hold one point per keypoint of F1");
        int n = 0;
        drfe_detail::check(drfe_search_for_initialization(D.ctx(), s1, s2, reinterpret_cast<float*>(vbPrevMatched.data()), n1, windowSize, mfNNratio,
                                                          mbCheckOrientation ? 1 : 0, vnMatches12.data(), &n), D.ctx(), "drfe_search_for_initialization");
        return n;
    }

    /* ---- src/ORBmatcher.cc:661-827 - LocalMapping::CreateNewMapPoints ---- */
    template <class KeyFrameT, class MatT>
    int SearchForTriangulation(KeyFrameT* pKF1, KeyFrameT* pKF2, MatT F12, std::vector<std::pair<size_t, size_t>>& vMatchedPairs, const bool bOnlyStereo)
    {
        MatcherDevice& D = Device();
        const int s1 = D.Resident(*pKF1, true), s2 = D.Resident(*pKF2, true, s1);
        const int n1 = (int)pKF1->mvKeysUn.size(), n2 = (int)pKF2->mvKeysUn.size();
        std::vector<int32_t> mp1((size_t)n1), mp2((size_t)n2), m12((size_t)n1, -1);
        for (int i = 0; i < n1; i++) mp1[(size_t)i] = pKF1->GetMapPoint((size_t)i) ? i : -1;
        for (int i = 0; i < n2; i++) mp2[(size_t)i] = pKF2->GetMapPoint((size_t)i) ? i : -1;
        const auto Cw = pKF1->GetCameraCenter();
        const auto T2w = pKF2->GetPose();
        const drfe_camera cam2 = drfe_detail::camera_of(*pKF2);
        int n = 0;
        drfe_detail::check(drfe_search_for_triangulation(D.ctx(), s1, s2, mp1.data(), n1, mp2.data(), n2, drfe_detail::f32(F12), drfe_detail::f32(Cw), drfe_detail::f32(T2w),
                                                         &cam2, bOnlyStereo ? 1 : 0, mbCheckOrientation ? 1 : 0, m12.data(), &n), D.ctx(),
                           "drfe_search_for_triangulation");
        vMatchedPairs.clear();
        vMatchedPairs.reserve((size_t)n);
        for (int i = 0; i < n1; i++) if (m12[(size_t)i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[(size_t)i]));
        return n;
    }

    /* ---- src/ORBmatcher.cc:1106-1330 - LoopClosing::ComputeSim3 ---- */
    template <class KeyFrameT, class MapPointT, class MatT>
    int SearchBySim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12, const float& s12, const MatT& R12, const MatT& t12, const float th)
    {
        MatcherDevice& D = Device();
        const int s1 = D.Resident(*pKF1), s2 = D.Resident(*pKF2, false, s1);
        const std::vector<MapPointT*> vp1 = pKF1->GetMapPointMatches(), vp2 = pKF2->GetMapPointMatches();
        const int N1 = (int)vp1.size(), N2 = (int)vp2.size();
        std::vector<uint8_t> skip1((size_t)N1, 0), skip2((size_t)N2, 0);
        for (int i = 0; i < N1; i++) {                                     /* :1131-1142 */
            MapPointT* p = vpMatches12[(size_t)i];
            if (p) {
                skip1[(size_t)i] = 1;
                const int idx2 = p->GetIndexInKeyFrame(pKF2);
                if (idx2 >= 0 && idx2 < N2) skip2[(size_t)idx2] = 1;
            }
        }
        std::vector<drfe_frustum_point> f1((size_t)N1), f2((size_t)N2);
        std::vector<uint8_t> d1((size_t)N1 * 32), d2((size_t)N2 * 32);
        for (int i = 0; i < N1; i++) {
            MapPointT* p = vp1[(size_t)i];
            std::memset(&f1[(size_t)i], 0, sizeof(drfe_frustum_point));
            if (!p || p->isBad()) skip1[(size_t)i] = 1;
            if (!skip1[(size_t)i]) drfe_detail::frustum_of(p, f1[(size_t)i], d1.data() + 32 * (size_t)i);
        }
        for (int i = 0; i < N2; i++) {
            MapPointT* p = vp2[(size_t)i];
            std::memset(&f2[(size_t)i], 0, sizeof(drfe_frustum_point));
            if (!p || p->isBad()) skip2[(size_t)i] = 1;
            if (!skip2[(size_t)i]) drfe_detail::frustum_of(p, f2[(size_t)i], d2.data() + 32 * (size_t)i);
        }
        const auto T1w = pKF1->GetPose();
        const auto T2w = pKF2->GetPose();
        std::vector<int32_t> m12((size_t)N1, -1);
        int nFound = 0;
        drfe_detail::check(drfe_search_by_sim3(D.ctx(), s1, s2, drfe_detail::f32(T1w), drfe_detail::f32(T2w), s12, drfe_detail::f32(R12), drfe_detail::f32(t12), f1.data(),
                                               d1.data(), skip1.data(), N1, f2.data(), d2.data(), skip2.data(), N2, th, m12.data(), &nFound), D.ctx(),
                           "drfe_search_by_sim3");
        for (int i1 = 0; i1 < N1; i1++) if (m12[(size_t)i1] >= 0) vpMatches12[(size_t)i1] = vp2[(size_t)m12[(size_t)i1]];
        return nFound;
    }

    /* ---- src/ORBmatcher.cc:829-985 - LocalMapping::SearchInNeighbors.  The search of every point on the device; the loop that
     * applies it runs here in the reference's order, re-reading isBad() / IsInKeyFrame() / GetMapPoint() at each step exactly where the
     * reference reads them: an earlier Replace or AddMapPoint of this very loop changes what a later point meets (:845, :957) ---- */
    /* tracker: a LocalMapTracker (below) that keeps a store of this map; it is told the gated answers before the loop runs, and
     * its store commits the same fusion (LocalMapTracker::FuseStore) */
    template <class KeyFrameT, class MapPointT, class TrackerT = void>
    int Fuse(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const float th = 3.0, TrackerT* tracker = nullptr)
    {
        MatcherDevice& D = Device();
        const int slot = D.Resident(*pKF);
        const int n = (int)vpMapPoints.size();
        std::vector<drfe_frustum_point> fp((size_t)n);
        std::vector<uint8_t> descs((size_t)n * 32), skip((size_t)n);
        for (int i = 0; i < n; i++) {
            MapPointT* p = vpMapPoints[(size_t)i];
            std::memset(&fp[(size_t)i], 0, sizeof(drfe_frustum_point));
            skip[(size_t)i] = !p || p->isBad() || p->IsInKeyFrame(pKF);
            if (!skip[(size_t)i]) drfe_detail::frustum_of(p, fp[(size_t)i], descs.data() + 32 * (size_t)i);
        }
        std::vector<int32_t> bestIdx((size_t)n, -1), bestDist((size_t)n, 256);
        const auto Tcw = pKF->GetPose();
        drfe_detail::check(drfe_fuse_search(D.ctx(), slot, drfe_detail::f32(Tcw), fp.data(), descs.data(), skip.data(), n, th, bestIdx.data(), bestDist.data()), D.ctx(),
                           "drfe_fuse_search");
        if constexpr (!std::is_void<TrackerT>::value)
            if (tracker) {
                std::vector<int32_t> gated(bestIdx);
                for (int i = 0; i < n; i++)
                    if (bestDist[(size_t)i] > TH_LOW) gated[(size_t)i] = -1;
                tracker->FuseStore(pKF, vpMapPoints, gated.data(), DRFE_LMAP_POINT, DRFE_LMAP_FUSE_NEIGHBOURS, nullptr);
            }
        int nFused = 0;
        for (int i = 0; i < n; i++) {
            MapPointT* pMP = vpMapPoints[(size_t)i];
            if (!pMP) continue;
            if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
            if (bestIdx[(size_t)i] < 0 || bestDist[(size_t)i] > TH_LOW) continue;
            MapPointT* pMPinKF = pKF->GetMapPoint((size_t)bestIdx[(size_t)i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                    else pMPinKF->Replace(pMP);
                }
            } else {
                pMP->AddObservation(pKF, (size_t)bestIdx[(size_t)i]);
                pKF->AddMapPoint(pMP, (size_t)bestIdx[(size_t)i]);
            }
            nFused++;
        }
        return nFused;
    }

    /* ---- src/ORBmatcher.cc:981-1105 - LoopClosing::SearchAndFuse ---- */
    template <class KeyFrameT, class MatT, class MapPointT>
    int Fuse(KeyFrameT* pKF, MatT Scw, const std::vector<MapPointT*>& vpPoints, float th, std::vector<MapPointT*>& vpReplacePoint)
    {
        MatcherDevice& D = Device();
        const int slot = D.Resident(*pKF);
        const std::set<MapPointT*> spAlreadyFound = pKF->GetMapPoints();
        const int n = (int)vpPoints.size();
        std::vector<drfe_frustum_point> fp((size_t)n);
        std::vector<uint8_t> descs((size_t)n * 32), skip((size_t)n);
        for (int i = 0; i < n; i++) {
            MapPointT* p = vpPoints[(size_t)i];
            std::memset(&fp[(size_t)i], 0, sizeof(drfe_frustum_point));
            skip[(size_t)i] = p->isBad() || spAlreadyFound.count(p);
            if (!skip[(size_t)i]) drfe_detail::frustum_of(p, fp[(size_t)i], descs.data() + 32 * (size_t)i);
        }
        std::vector<int32_t> bestIdx((size_t)n, -1), bestDist((size_t)n, 256);
        drfe_detail::check(drfe_fuse_search_sim3(D.ctx(), slot, drfe_detail::f32(Scw), fp.data(), descs.data(), skip.data(), n, th, bestIdx.data(), bestDist.data()), D.ctx(),
                           "drfe_fuse_search_sim3");
        int nFused = 0;
        for (int i = 0; i < n; i++) {
            if (skip[(size_t)i] || bestIdx[(size_t)i] < 0 || bestDist[(size_t)i] > TH_LOW) continue;
            MapPointT* pMP = vpPoints[(size_t)i];
            MapPointT* pMPinKF = pKF->GetMapPoint((size_t)bestIdx[(size_t)i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) vpReplacePoint[(size_t)i] = pMPinKF;
            } else {
                pMP->AddObservation(pKF, (size_t)bestIdx[(size_t)i]);
                pKF->AddMapPoint(pMP, (size_t)bestIdx[(size_t)i]);
            }
            nFused++;
        }
        return nFused;
    }

    /* ---- slot-level forms (the frames already live in slots of `ctx`: the per-frame flow of ORBextractor::Submit / Collect) ---- */
    /* SearchByProjection(CurrentFrame, LastFrame, th, bMono) on the slots `cur` / `last` of ctx (extract + glue done):
     * lastPoints[i] = what the loop reads of LastFrame.mvpMapPoints[i]; curClaims in/out = index into lastPoints or -1 */
    int SearchByProjection(drfe_ctx* ctx, int cur, int last, const float* TcwCur, const float* TcwLast, const drfe_camera& cam,
                           const std::vector<drfe_map_point>& lastPoints, std::vector<int32_t>& curClaims, float th, bool bMono)
    {
        int n = 0;
        drfe_detail::check(drfe_search_by_projection_last(ctx, cur, last, TcwCur, TcwLast, &cam, lastPoints.data(), (int)lastPoints.size(),
                                                          th, bMono ? 1 : 0, mbCheckOrientation ? 1 : 0, nullptr, curClaims.data(),
                                                          (int)curClaims.size(), &n), ctx, "drfe_search_by_projection_last");
        return n;
    }
    /* SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) on the slots f1 / f2 of ctx (src/ORBmatcher.cc:409-524):
     * vbPrevMatched = (x, y) per F1 keypoint, updated in place; vnMatches12[i1] = index into F2's keypoints or -1 */
    int SearchForInitialization(drfe_ctx* ctx, int f1, int f2, std::vector<float>& vbPrevMatched, std::vector<int>& vnMatches12,
                                int windowSize = 10)
    {
        int n = 0;
        vnMatches12.assign(vbPrevMatched.size() / 2, -1);
        drfe_detail::check(drfe_search_for_initialization(ctx, f1, f2, vbPrevMatched.data(), (int)vnMatches12.size(), windowSize, mfNNratio,
                                                          mbCheckOrientation ? 1 : 0, vnMatches12.data(), &n), ctx,
                           "drfe_search_for_initialization");
        return n;
    }
protected:
    static MatcherDevice*& tls() { static thread_local MatcherDevice* d = nullptr; return d; }
    float mfNNratio; bool mbCheckOrientation;
};

/* include/PlaneExtractor.h:30-59 */
typedef drfe_cv::Vector3d VertexType;
const int kDepthWidth = 640;
const int kDepthHeight = 480;

/* ImagePointCloud (include/PlaneExtractor.h:42-59).  `vertices[j]` is what Frame::ComputePlanes reads
 * (planeDetector.cloud.vertices[j][0..2], src/Frame.cc:959-961) for the members of every plane - a few ten thousand of the
 * 307 200 pixels - so the container computes a vertex when it is asked for it, with PlaneDetection::readDepthImage's
 * arithmetic (src/PlaneExtractor.cpp:36-53: doubles, K's floats promoted, z > 5 -> (0, 0, 0)), instead of filling 7.4 MB per
 * frame on the host: the extractor itself builds its points on the device (k_ahc_blocks) and never reads this array. */
struct ImagePointCloud {
    struct Vertices {
        const uint16_t* depth = nullptr; size_t strideElems = 0; int w = 0, h = 0;
        float fx = 1, fy = 1, cx = 0, cy = 0, factor = 0;
        size_t size() const { return (size_t)w * h; }
        VertexType operator[](size_t pixIdx) const
        {
            const int i = (int)(pixIdx / (size_t)w), j = (int)(pixIdx % (size_t)w);
            const double z = (double)depth[(size_t)i * strideElems + j] * factor;
            if (std::isnan(z)) return VertexType(0, 0, z);
            if (z > 5.0) return VertexType(0, 0, 0);
            const double x = ((double)j - cx) * z / fx, y = ((double)i - cy) * z / fy;
            return VertexType(x, y, z);
        }
    } vertices;
    int w = kDepthWidth, h = kDepthHeight;
    inline int width() const { return w; }
    inline int height() const { return h; }
    inline bool get(const int row, const int col, double& x, double& y, double& z) const
    {
        const VertexType p = vertices[(size_t)row * w + col];
        z = p[2];
        if (z == 0 || std::isnan(z)) return false;
        x = p[0]; y = p[1];
        return true;
    }
};

/* the members of ahc::PlaneSeg Frame::ComputePlanes reads through plane_filter.extractedPlanes[i] (include/peac/AHCPlaneSeg.hpp:
 * normal, center, mse, curvature, N) */
struct ExtractedPlane { double normal[3], center[3], mse, curvature; int N; };
/* the part of ahc::PlaneFitter<ImagePointCloud> the callers touch (include/peac/AHCPlaneFitter.hpp:118): extractedPlanes */
struct PlaneFitterView { std::vector<std::shared_ptr<ExtractedPlane>> extractedPlanes; };

/* include/PlaneExtractor.h:61-82 (the live AHC extractor).  Member shape as Frame::ComputePlanes uses it (src/Frame.cc:947-979):
 *   planeDetector.readColorImage(img); planeDetector.readDepthImage(depth, K, factor); planeDetector.runPlaneDetection();
 *   planeDetector.plane_num_, .plane_vertices_[i], .cloud.vertices[j][k], .plane_filter.extractedPlanes[i]->normal / ->center,
 *   .seg_output */
class PlaneDetection {
public:
    typedef Planar_SLAM::ExtractedPlane ExtractedPlane;
    static const int kDepthWidth = 640, kDepthHeight = 480;
    ImagePointCloud cloud;
    PlaneFitterView plane_filter;
    std::vector<std::vector<int>> plane_vertices_;     /* vertex indices each plane contains */
    std::vector<std::shared_ptr<ExtractedPlane>>& extractedPlanes = plane_filter.extractedPlanes;   /* round-2 spelling, same object */
    drfe_cv::Mat seg_output;
    drfe_cv::Mat color_img_;
    int plane_num_ = 0;

    explicit PlaneDetection(drfe_ctx* ctx) : mCtx(ctx) {}
    PlaneDetection(const PlaneDetection&) = delete;
    PlaneDetection& operator=(const PlaneDetection&) = delete;

    bool readColorImage(const drfe_cv::Mat& RGBImg) { color_img_ = RGBImg; return !color_img_.empty(); }   /* kept for the caller; the extractor does not read it */

    bool readDepthImage(const drfe_cv::Mat& depthImg, const float K[9] /* mK row-major */, float depthfactor)
    {
#ifdef DRFE_WITH_OPENCV
        if (depthImg.empty() || depthImg.depth() != CV_16U) return false;
#else
        if (depthImg.empty() || depthImg.elem != 2) return false;       /* "cannot read depth image": CV_16U only */
#endif
        mDepth = depthImg; mFactor = depthfactor;
        mK4[0] = K[0]; mK4[1] = K[4]; mK4[2] = K[2]; mK4[3] = K[5];
        cloud.w = depthImg.cols; cloud.h = depthImg.rows;
        cloud.vertices.depth = mDepth.ptr<uint16_t>(0); cloud.vertices.strideElems = drfe_cv::mat_step(mDepth) / 2;
        cloud.vertices.w = depthImg.cols; cloud.vertices.h = depthImg.rows;
        cloud.vertices.fx = K[0]; cloud.vertices.fy = K[4]; cloud.vertices.cx = K[2]; cloud.vertices.cy = K[5];
        cloud.vertices.factor = depthfactor;
        return true;
    }
#ifdef DRFE_WITH_OPENCV
    bool readDepthImage(cv::Mat depthImg, cv::Mat& K, const float depthfactor)        /* the reference's signature: CV_32F 3 x 3 K */
    {
        const float k9[9] = {K.at<float>(0, 0), 0, K.at<float>(0, 2), 0, K.at<float>(1, 1), K.at<float>(1, 2), 0, 0, 1};
        return readDepthImage(static_cast<const drfe_cv::Mat&>(depthImg), k9, depthfactor);
    }
#endif
    void runPlaneDetection()
    {
        std::vector<drfe_plane> pl(64);
        std::vector<int32_t> off(65), idx((size_t)mDepth.cols * mDepth.rows);
        seg_output = drfe_cv::mat_u8(mDepth.rows, mDepth.cols);
        int np = 0;
        drfe_detail::check(drfe_planes_ahc(mCtx, mDepth.ptr<uint16_t>(0), mDepth.cols, mDepth.rows, drfe_cv::mat_step(mDepth) / 2, mK4, mFactor,
                                           pl.data(), 64, &np, seg_output.data, off.data(), idx.data()), mCtx, "drfe_planes_ahc");
        plane_num_ = np;
        plane_vertices_.assign(np, std::vector<int>());
        plane_filter.extractedPlanes.clear();
        for (int i = 0; i < np; i++) {
            plane_vertices_[i].assign(idx.begin() + off[i], idx.begin() + off[i + 1]);
            auto e = std::make_shared<ExtractedPlane>();
            std::memcpy(e->normal, pl[i].normal, 24); std::memcpy(e->center, pl[i].center, 24);
            e->mse = pl[i].mse; e->curvature = pl[i].curvature; e->N = pl[i].n_points;
            plane_filter.extractedPlanes.push_back(e);
        }
    }
private:
    drfe_ctx* mCtx; drfe_cv::Mat mDepth; float mFactor = 0; float mK4[4] = {0, 0, 0, 0};
};

/* PlaneSeg of src/CAPE/PlaneSeg.h as far as Frame::ComputePlanes_CAPE reads it (src/Frame.cc:1118-1121: normal[0..2], d), plus
 * the fields CAPE::process fills beside them */
struct PlaneSeg { double normal[3], mean[3], d; float MSE, score; int nr_pts; };
struct CylinderSeg { int nr_segments = 0; };             /* cylinder_detection is false in the reference (include/PlaneExtractor.h:112) */

/* include/PlaneExtractor.h:84-115.  Member shape as Frame::ComputePlanes_CAPE uses it (src/Frame.cc:1096-1141):
 *   readColorImage(imGrey); readDepthImage(depth /+ CV_32F metres +/, K); runPlaneDetection();
 *   nr_planes, plane_cloud[i] (the plane's points in raster order), plane_params[i].normal / .d, seg_output
 * PointCloud::Ptr of the reference is a pcl::PointCloud<pcl::PointXYZRGB>::Ptr; here plane_cloud[i] is a shared pointer to a
 * vector of float xyz triples (PCL is absent) with the same points in the same order. */
class PlaneDetection_CAPE {
public:
    struct PointT { float x, y, z; };
    struct PointCloud { std::vector<PointT> points; size_t size() const { return points.size(); } typedef std::shared_ptr<PointCloud> Ptr; };

    explicit PlaneDetection_CAPE(drfe_ctx* ctx) : mCtx(ctx) {}
    ~PlaneDetection_CAPE() {}

    bool readColorImage(const drfe_cv::Mat& RGBImg) { color_img_ = RGBImg; return !color_img_.empty(); }
    bool readDepthImage(const drfe_cv::Mat& depthImg, const float K[9] /* row-major */)
    {
#ifdef DRFE_WITH_OPENCV
        if (depthImg.empty() || depthImg.depth() != CV_32F) return false;
#else
        if (depthImg.empty() || depthImg.elem != 4) return false;        /* CV_32F metres (src/PlaneExtractor.cpp:104-112) */
#endif
        depth_img = depthImg;
        mK4[0] = K[0]; mK4[1] = K[4]; mK4[2] = K[2]; mK4[3] = K[5];
        return true;
    }
#ifdef DRFE_WITH_OPENCV
    bool readDepthImage(cv::Mat depthImg, cv::Mat& K)
    {
        K_ = K;
        const float k9[9] = {K.at<float>(0, 0), 0, K.at<float>(0, 2), 0, K.at<float>(1, 1), K.at<float>(1, 2), 0, 0, 1};
        return readDepthImage(static_cast<const drfe_cv::Mat&>(depthImg), k9);
    }
#endif
    void runPlaneDetection()
    {
        const int rows = depth_img.rows, cols = depth_img.cols;
        std::vector<drfe_cape_plane> pl(64);
        seg_output = drfe_cv::mat_u8(rows, cols);
        int np = 0;
        const size_t strideElems = drfe_cv::mat_step(depth_img) / 4;
        drfe_detail::check(drfe_planes_cape(mCtx, depth_img.ptr<float>(0), cols, rows, strideElems, mK4, PATCH_SIZE, COS_ANGLE_MAX,
                                            MAX_MERGE_DIST, pl.data(), 64, &np, seg_output.data, nullptr, nullptr, nullptr), mCtx, "drfe_planes_cape");
        nr_planes = np; nr_cylinders = 0;
        plane_params.resize(np);
        for (int i = 0; i < np; i++) {
            PlaneSeg& o = plane_params[i];
            std::memcpy(o.normal, pl[i].normal, 24); std::memcpy(o.mean, pl[i].mean, 24);
            o.d = pl[i].d; o.MSE = pl[i].mse; o.score = pl[i].score; o.nr_pts = pl[i].n_points;
        }
        /* plane_cloud: the reference APPENDS nr_planes new clouds per call and indexes them from 0 (src/PlaneExtractor.cpp:165-189
         * with plane_cloud a member that is never cleared) - frame 2's points land in frame 1's clouds.  Reproduced literally. */
        for (int i = 0; i < np; ++i) plane_cloud.push_back(std::make_shared<PointCloud>());
        for (int i = 0; i < rows; i++) {
            const uint8_t* sCode = seg_output.ptr<uint8_t>(i);
            const float* drow = depth_img.ptr<float>(i);
            for (int j = 0; j < cols; j++) {
                const int code = sCode[j];
                if (code > 0) {
                    const double z = (double)drow[j];
                    const double x = ((double)j - mK4[2]) * z / mK4[0], y = ((double)i - mK4[3]) * z / mK4[1];
                    plane_cloud[code - 1]->points.push_back(PointT{(float)(float)x, (float)(float)y, (float)(float)z});   /* double -> MatrixXf -> PointT */
                }
            }
        }
    }

    std::vector<PointCloud::Ptr> plane_cloud;
    std::vector<PlaneSeg> plane_params;
    std::vector<CylinderSeg> cylinder_params;
    int nr_planes = 0, nr_cylinders = 0;
    drfe_cv::Mat seg_output;
    drfe_cv::Mat color_img_, depth_img;
#ifdef DRFE_WITH_OPENCV
    cv::Mat K_;
#endif
    int PATCH_SIZE = 20;
    float COS_ANGLE_MAX = (float)std::cos(3.14159265358979323846 / 12);
    float MAX_MERGE_DIST = 0;
    bool cylinder_detection = false;
private:
    drfe_ctx* mCtx; float mK4[4] = {0, 0, 0, 0};
};

/* ---------------------------------------------------------------------------------------------------------------------------
 * LSDmatcher (include/LSDmatcher.h:21-36, src/LSDmatcher.cpp) with the reference's ten signatures, the same way as ORBmatcher above:
 * member templates over the frame / keyframe / map-line types that use only the member names src/LSDmatcher.cpp reads
 *   Frame:    mTcw, fx fy cx cy mbf, mnMinX .. mnMaxY, NL, mvKeylinesUn, mLdesc, mvpMapLines, mvbLineOutlier
 *   KeyFrame: fx fy cx cy mbf, mnMinX .. mnMaxY, mvKeyLines, mLineDescriptors, GetMapLineMatches(), GetMapLine(idx), GetMapLines(),
 *             AddMapLine(pML, idx), GetPose(), mnId (through MapLine::GetIndexInKeyFrame)
 *   MapLine:  isBad(), Observations(), GetWorldPos() (six doubles through operator()), GetNormal() (three), GetDescriptor(),
 *             GetMinDistanceInvariance(), GetMaxDistanceInvariance(), GetIndexInKeyFrame(pKF), AddObservation(pKF, idx), Replace(pML),
 *             mbTrackInView, mnTrackScaleLevel, mTrackViewCos, mTrackProjX1 / Y1 / X2 / Y2
 * so they bind to Planar_SLAM::Frame, KeyFrame and MapLine as they are and to the stand-ins of tests/native/linematcher_caller.cpp.
 * A line frame needs no device residency (a frame holds at most 40 key lines: they travel with the call), only a context: the one
 * bound to the calling thread (LSDmatcher::BindThread, or ORBmatcher::BindThread's device).  mvScaleFactors / mfLogScaleFactor are
 * the context's own tables (same ORB parameters as the frames': include/drfe.h drfe_orb_scale_tables).
 * Every method flattens what the reference's loop reads through the pointers, calls the C entry point (projection, GetLinesInArea,
 * Hamming distances, claim order: on the device), writes MapLine* back, and - Fuse - applies Replace / AddObservation / AddMapLine
 * on the host in the reference's order, re-reading isBad() / GetMapLine() where the reference reads them. */
namespace drfe_detail {
template <class KL> inline drfe_keyline keyline_of(const KL& k)
{
    drfe_keyline o;
    o.angle = k.angle; o.class_id = k.class_id; o.octave = k.octave; o.pt_x = k.pt.x; o.pt_y = k.pt.y; o.response = k.response; o.size = k.size;
    o.start_point_x = k.startPointX; o.start_point_y = k.startPointY; o.end_point_x = k.endPointX; o.end_point_y = k.endPointY;
    o.s_point_in_octave_x = k.sPointInOctaveX; o.s_point_in_octave_y = k.sPointInOctaveY;
    o.e_point_in_octave_x = k.ePointInOctaveX; o.e_point_in_octave_y = k.ePointInOctaveY;
    o.line_length = k.lineLength; o.num_of_pixels = k.numOfPixels;
    return o;
}
template <class V> inline std::vector<drfe_keyline> keylines_of(const V& v)
{
    std::vector<drfe_keyline> o(v.size());
    for (size_t i = 0; i < v.size(); i++) o[i] = keyline_of(v[i]);
    return o;
}
/* what the projection loops read of a MapLine: GetWorldPos (Vector6d), GetNormal (Vector3d), the distance band, GetDescriptor */
template <class ML> inline void frustum_line_of(ML* p, drfe_frustum_line& o, uint8_t* desc32)
{
    const auto P = p->GetWorldPos();
    for (int k = 0; k < 6; k++) o.world[k] = P(k);
    const auto Pn = p->GetNormal();
    for (int k = 0; k < 3; k++) o.normal[k] = Pn(k);
    o.min_distance = p->GetMinDistanceInvariance(); o.max_distance = p->GetMaxDistanceInvariance();
    const auto d = p->GetDescriptor(); std::memcpy(desc32, d.data, 32);
}
}  // namespace drfe_detail

class LSDmatcher {
public:
    static const int TH_HIGH = 100, TH_LOW = 50;                          /* src/LSDmatcher.cpp:13-14 */
    LSDmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    /* the calling thread's context: once per thread that constructs line matchers (ORBmatcher::BindThread does it too) */
    static void BindThread(drfe_ctx* ctx) { drfe_detail::thread_ctx() = ctx; }
    static drfe_ctx* Context()
    {
        drfe_ctx* c = drfe_detail::thread_ctx();
        if (!c) throw std::runtime_error("LSDmatcher: no context bound to this thread (LSDmatcher::BindThread / ORBmatcher::BindThread)");
        return c;
    }

    /* ---- src/LSDmatcher.cpp:242-279 - Tracking::TrackReferenceKeyFrame / TrackWithMotionModel / Relocalization
     * (src/Tracking.cc:2189, :2323, :2445, :2572) ---- */
    template <class KeyFrameT, class FrameT, class MapLineT>
    typename std::enable_if<std::is_class<FrameT>::value, int>::type
    SearchByDescriptor(KeyFrameT* pKF, FrameT& currentF, std::vector<MapLineT*>& vpMapLineMatches)
    {
        drfe_ctx* c = Context();
        const std::vector<MapLineT*> vpMapLinesKF = pKF->GetMapLineMatches();
        vpMapLineMatches = std::vector<MapLineT*>((size_t)currentF.NL, static_cast<MapLineT*>(nullptr));
        const int nq = pKF->mLineDescriptors.rows, nt = currentF.mLdesc.rows;
        std::vector<uint8_t> has((size_t)nq, 0);
        for (int q = 0; q < nq && q < (int)vpMapLinesKF.size(); q++) has[(size_t)q] = vpMapLinesKF[(size_t)q] != nullptr;
        std::vector<int32_t> m((size_t)nt, -1);
        int n = 0;
        drfe_detail::check(drfe_lsd_search_by_descriptor(c, drfe_detail::u8(pKF->mLineDescriptors), nq, drfe_detail::u8(currentF.mLdesc), nt, has.data(), 0,
                                                         m.data(), &n), c, "drfe_lsd_search_by_descriptor");
        for (int t = 0; t < nt && t < (int)vpMapLineMatches.size(); t++) if (m[(size_t)t] >= 0) vpMapLineMatches[(size_t)t] = vpMapLinesKF[(size_t)m[(size_t)t]];
        return n;
    }

    /* ---- src/LSDmatcher.cpp:281-314 ---- */
    template <class KeyFrameT, class MapLineT>
    int SearchByDescriptor(KeyFrameT* pKF, KeyFrameT* pKF2, std::vector<MapLineT*>& vpMapLineMatches)
    {
        drfe_ctx* c = Context();
        const std::vector<MapLineT*> vpMapLinesKF = pKF->GetMapLineMatches();
        const std::vector<MapLineT*> vpMapLinesKF2 = pKF2->GetMapLineMatches();
        vpMapLineMatches = std::vector<MapLineT*>(vpMapLinesKF.size(), static_cast<MapLineT*>(nullptr));
        const int nq = pKF->mLineDescriptors.rows, nt = pKF2->mLineDescriptors.rows;
        std::vector<uint8_t> has((size_t)nt, 0);
        for (int t = 0; t < nt && t < (int)vpMapLinesKF2.size(); t++) has[(size_t)t] = vpMapLinesKF2[(size_t)t] != nullptr;
        std::vector<int32_t> m((size_t)nq, -1);
        int n = 0;
        drfe_detail::check(drfe_lsd_search_by_descriptor(c, drfe_detail::u8(pKF->mLineDescriptors), nq, drfe_detail::u8(pKF2->mLineDescriptors), nt, has.data(), 1,
                                                         m.data(), &n), c, "drfe_lsd_search_by_descriptor");
        for (int q = 0; q < nq && q < (int)vpMapLineMatches.size(); q++) if (m[(size_t)q] >= 0) vpMapLineMatches[(size_t)q] = vpMapLinesKF2[(size_t)m[(size_t)q]];
        return n;
    }

    /* ---- src/LSDmatcher.cpp:20-139 - the motion-model search of the line tracker ---- */
    template <class FrameT, class LastT>
    typename std::enable_if<std::is_class<LastT>::value, int>::type
    SearchByProjection(FrameT& CurrentFrame, const LastT& LastFrame, const float th, const bool bMono)
    {
        drfe_ctx* c = Context();
        const int nl = (int)LastFrame.NL, nc = (int)CurrentFrame.mvKeylinesUn.size();
        std::vector<drfe_map_line> ml((size_t)nl);
        for (int i = 0; i < nl; i++) {
            auto* p = LastFrame.mvpMapLines[(size_t)i];
            drfe_map_line& r = ml[(size_t)i];
            std::memset(&r, 0, sizeof(r));
            r.valid = p && !p->isBad() && !LastFrame.mvbLineOutlier[(size_t)i];
            if (!r.valid) continue;
            r.octave = LastFrame.mvKeylinesUn[(size_t)i].octave;
            r.obs_positive = p->Observations() > 0;
            const auto P = p->GetWorldPos();
            for (int k = 0; k < 6; k++) r.world[k] = P(k);
            const auto d = p->GetDescriptor(); std::memcpy(r.desc, d.data, 32);
        }
        const std::vector<drfe_keyline> kl = drfe_detail::keylines_of(CurrentFrame.mvKeylinesUn);
        /* claims the frame already holds: any index >= nl (a new match is an index into LastFrame) */
        std::vector<int32_t> claim((size_t)nc);
        std::vector<uint8_t> obs((size_t)nc);
        for (int i = 0; i < nc; i++) { auto* p = CurrentFrame.mvpMapLines[(size_t)i]; claim[(size_t)i] = p ? nl + i : -1; obs[(size_t)i] = p && p->Observations() > 0; }
        const drfe_camera cam = drfe_detail::camera_of(CurrentFrame);
        int n = 0;
        drfe_detail::check(drfe_lsd_search_by_projection_last(c, drfe_detail::f32(CurrentFrame.mTcw), drfe_detail::f32(LastFrame.mTcw), &cam, ml.data(), nl, kl.data(),
                                                              drfe_detail::u8(CurrentFrame.mLdesc), nc, th, bMono ? 1 : 0, mfNNratio, obs.data(), claim.data(), &n), c,
                           "drfe_lsd_search_by_projection_last");
        for (int i = 0; i < nc; i++) if (claim[(size_t)i] >= 0 && claim[(size_t)i] < nl) CurrentFrame.mvpMapLines[(size_t)i] = LastFrame.mvpMapLines[(size_t)claim[(size_t)i]];
        return n;
    }

    /* ---- src/LSDmatcher.cpp:141-211 - the local map's lines into the frame, after Frame::isInFrustum(MapLine*) ---- */
    template <class FrameT, class MapLineT>
    int SearchByProjection(FrameT& F, const std::vector<MapLineT*>& vpMapLines, const float th = 3)
    {
        drfe_ctx* c = Context();
        const int m = (int)vpMapLines.size(), nc = (int)F.mvKeylinesUn.size();
        std::vector<drfe_tracked_line> tl((size_t)m);
        for (int i = 0; i < m; i++) {
            MapLineT* p = vpMapLines[(size_t)i];
            drfe_tracked_line& t = tl[(size_t)i];
            std::memset(&t, 0, sizeof(t));
            t.in_view = p && !p->isBad() && p->mbTrackInView;
            if (!t.in_view) continue;
            t.level = p->mnTrackScaleLevel; t.obs_positive = p->Observations() > 0;
            t.x1 = p->mTrackProjX1; t.y1 = p->mTrackProjY1; t.x2 = p->mTrackProjX2; t.y2 = p->mTrackProjY2; t.view_cos = p->mTrackViewCos;
            const auto d = p->GetDescriptor(); std::memcpy(t.desc, d.data, 32);
        }
        const std::vector<drfe_keyline> kl = drfe_detail::keylines_of(F.mvKeylinesUn);
        std::vector<int32_t> claim((size_t)nc);
        std::vector<uint8_t> obs((size_t)nc);
        for (int i = 0; i < nc; i++) { auto* p = F.mvpMapLines[(size_t)i]; claim[(size_t)i] = p ? m + i : -1; obs[(size_t)i] = p && p->Observations() > 0; }
        int n = 0;
        drfe_detail::check(drfe_lsd_search_by_projection_map(c, tl.data(), m, kl.data(), drfe_detail::u8(F.mLdesc), nc, th, mfNNratio, obs.data(), claim.data(), &n), c,
                           "drfe_lsd_search_by_projection_map");
        for (int i = 0; i < nc; i++) if (claim[(size_t)i] >= 0 && claim[(size_t)i] < m) F.mvpMapLines[(size_t)i] = vpMapLines[(size_t)claim[(size_t)i]];
        return n;
    }

    /* ---- src/LSDmatcher.cpp:377-502 - a keyframe against the lines of a loop candidate's neighbourhood ---- */
    template <class KeyFrameT, class MatT, class MapLineT>
    int SearchByProjection(KeyFrameT* pKF, MatT Scw, const std::vector<MapLineT*>& vpLines, std::vector<MapLineT*>& vpMatched, int th)
    {
        drfe_ctx* c = Context();
        const int n = (int)vpLines.size(), nk = (int)pKF->mvKeyLines.size();
        if ((int)vpMatched.size() < nk) throw std::runtime_error("LSDmatcher::SearchByProjection: vpMatched must hold one entry per key line of pKF");
        std::set<MapLineT*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
        spAlreadyFound.erase(static_cast<MapLineT*>(nullptr));
        std::vector<drfe_frustum_line> fl((size_t)n);
        std::vector<uint8_t> descs((size_t)n * 32), skip((size_t)n), matched((size_t)nk);
        for (int i = 0; i < n; i++) {
            MapLineT* p = vpLines[(size_t)i];
            std::memset(&fl[(size_t)i], 0, sizeof(drfe_frustum_line));
            skip[(size_t)i] = !p || p->isBad() || spAlreadyFound.count(p);
            if (!skip[(size_t)i]) drfe_detail::frustum_line_of(p, fl[(size_t)i], descs.data() + 32 * (size_t)i);
        }
        for (int k = 0; k < nk; k++) matched[(size_t)k] = vpMatched[(size_t)k] != nullptr;
        const std::vector<drfe_keyline> kl = drfe_detail::keylines_of(pKF->mvKeyLines);
        const drfe_camera cam = drfe_detail::camera_of(*pKF);
        std::vector<int32_t> nm((size_t)nk, -1);
        int cnt = 0;
        drfe_detail::check(drfe_lsd_search_by_projection_kf(c, drfe_detail::f32(Scw), &cam, fl.data(), descs.data(), skip.data(), n, kl.data(),
                                                            drfe_detail::u8(pKF->mLineDescriptors), nk, matched.data(), th, nm.data(), &cnt), c,
                           "drfe_lsd_search_by_projection_kf");
        for (int k = 0; k < nk; k++) if (nm[(size_t)k] >= 0) vpMatched[(size_t)k] = vpLines[(size_t)nm[(size_t)k]];
        return cnt;
    }

    /* ---- src/LSDmatcher.cpp:504-748 ---- */
    template <class KeyFrameT, class MapLineT, class MatT>
    int SearchBySim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapLineT*>& vpMatches12, const float& s12, const MatT& R12, const MatT& t12, const float th)
    {
        drfe_ctx* c = Context();
        const std::vector<MapLineT*> vp1 = pKF1->GetMapLineMatches(), vp2 = pKF2->GetMapLineMatches();
        const int N1 = (int)vp1.size(), N2 = (int)vp2.size();
        if ((int)pKF1->mvKeyLines.size() != N1 || (int)pKF2->mvKeyLines.size() != N2)
            throw std::runtime_error("LSDmatcher::SearchBySim3: GetMapLineMatches() must hold one entry per key line");
        std::vector<uint8_t> skip1((size_t)N1, 0), skip2((size_t)N2, 0);
        for (int i = 0; i < N1; i++) {                                     /* :533-543 */
            MapLineT* p = vpMatches12[(size_t)i];
            if (p) {
                skip1[(size_t)i] = 1;
                const int idx2 = p->GetIndexInKeyFrame(pKF2);
                if (idx2 >= 0 && idx2 < N2) skip2[(size_t)idx2] = 1;
            }
        }
        std::vector<drfe_frustum_line> f1((size_t)N1), f2((size_t)N2);
        std::vector<uint8_t> d1((size_t)N1 * 32), d2((size_t)N2 * 32);
        for (int i = 0; i < N1; i++) {
            MapLineT* p = vp1[(size_t)i];
            std::memset(&f1[(size_t)i], 0, sizeof(drfe_frustum_line));
            if (!p || p->isBad()) skip1[(size_t)i] = 1;
            if (!skip1[(size_t)i]) drfe_detail::frustum_line_of(p, f1[(size_t)i], d1.data() + 32 * (size_t)i);
        }
        for (int i = 0; i < N2; i++) {
            MapLineT* p = vp2[(size_t)i];
            std::memset(&f2[(size_t)i], 0, sizeof(drfe_frustum_line));
            if (!p || p->isBad()) skip2[(size_t)i] = 1;
            if (!skip2[(size_t)i]) drfe_detail::frustum_line_of(p, f2[(size_t)i], d2.data() + 32 * (size_t)i);
        }
        const std::vector<drfe_keyline> kl1 = drfe_detail::keylines_of(pKF1->mvKeyLines), kl2 = drfe_detail::keylines_of(pKF2->mvKeyLines);
        const auto T1w = pKF1->GetPose();
        const auto T2w = pKF2->GetPose();
        const drfe_camera cam = drfe_detail::camera_of(*pKF1);
        std::vector<int32_t> m12((size_t)N1, -1);
        int nFound = 0;
        drfe_detail::check(drfe_lsd_search_by_sim3(c, &cam, drfe_detail::f32(T1w), drfe_detail::f32(T2w), s12, drfe_detail::f32(R12), drfe_detail::f32(t12), f1.data(),
                                                   d1.data(), skip1.data(), kl1.data(), drfe_detail::u8(pKF1->mLineDescriptors), N1, f2.data(), d2.data(), skip2.data(),
                                                   kl2.data(), drfe_detail::u8(pKF2->mLineDescriptors), N2, th, m12.data(), &nFound), c, "drfe_lsd_search_by_sim3");
        for (int i1 = 0; i1 < N1; i1++) if (m12[(size_t)i1] >= 0) vpMatches12[(size_t)i1] = vp2[(size_t)m12[(size_t)i1]];
        return nFound;
    }

    /* ---- src/LSDmatcher.cpp:213-240 - Tracking::MonocularInitialization (src/Tracking.cc:1697); the reference spells it "Serach" ---- */
    template <class FrameT>
    typename std::enable_if<std::is_class<FrameT>::value, int>::type
    SerachForInitialize(FrameT& InitialFrame, FrameT& CurrentFrame, std::vector<std::pair<int, int>>& LineMatches)
    {
        drfe_ctx* c = Context();
        LineMatches.clear();
        const int nq = InitialFrame.mLdesc.rows, nt = CurrentFrame.mLdesc.rows;
        std::vector<int32_t> m((size_t)nq, -1);
        int n = 0;
        drfe_detail::check(drfe_lsd_search_by_descriptor(c, drfe_detail::u8(InitialFrame.mLdesc), nq, drfe_detail::u8(CurrentFrame.mLdesc), nt, nullptr, 1, m.data(), &n), c,
                           "drfe_lsd_search_by_descriptor");
        for (int q = 0; q < nq; q++) if (m[(size_t)q] >= 0) LineMatches.push_back(std::make_pair(q, (int)m[(size_t)q]));
        return n;
    }

    /* ---- src/LSDmatcher.cpp:334-367 - LocalMapping::CreateNewMapLines (src/LocalMapping.cc:606, :858) ---- */
    template <class KeyFrameT>
    typename std::enable_if<std::is_class<KeyFrameT>::value, int>::type
    SearchForTriangulation(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<std::pair<size_t, size_t>>& vMatchedPairs)
    {
        drfe_ctx* c = Context();
        vMatchedPairs.clear();
        const int n1 = pKF1->mLineDescriptors.rows, n2 = pKF2->mLineDescriptors.rows;
        std::vector<uint8_t> has1((size_t)n1), has2((size_t)n2);
        for (int i = 0; i < n1; i++) has1[(size_t)i] = pKF1->GetMapLine((size_t)i) != nullptr;
        for (int i = 0; i < n2; i++) has2[(size_t)i] = pKF2->GetMapLine((size_t)i) != nullptr;
        std::vector<int32_t> m((size_t)n1, -1);
        int n = 0;
        drfe_detail::check(drfe_lsd_search_for_triangulation(c, drfe_detail::u8(pKF1->mLineDescriptors), n1, drfe_detail::u8(pKF2->mLineDescriptors), n2, has1.data(),
                                                             has2.data(), m.data(), &n), c, "drfe_lsd_search_for_triangulation");
        for (int i = 0; i < n1; i++) if (m[(size_t)i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m[(size_t)i]));
        return n;
    }

    /* ---- src/LSDmatcher.cpp:884-1015 - LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1103, :1124).  The search of every line on
     * the device (it reads the keyframe's key lines and descriptors, never its MapLine assignments); the loop that applies it runs here
     * in the reference's order and re-reads isBad() / GetMapLine() at each step: an earlier Replace or AddMapLine of this very loop
     * changes what a later line meets (:907, :995).  A predicted level outside the pyramid (the reference reads mvScaleFactors out of
     * bounds there) fuses nothing. ---- */
    template <class KeyFrameT, class MapLineT, class TrackerT = void>
    int Fuse(KeyFrameT* pKF, const std::vector<MapLineT*>& vpMapLines, const float th = 3.0, TrackerT* tracker = nullptr)
    {
        drfe_ctx* c = Context();
        const int n = (int)vpMapLines.size(), nk = (int)pKF->mvKeyLines.size();
        std::vector<drfe_frustum_line> fl((size_t)n);
        std::vector<uint8_t> descs((size_t)n * 32), skip((size_t)n);
        for (int i = 0; i < n; i++) {
            MapLineT* p = vpMapLines[(size_t)i];
            std::memset(&fl[(size_t)i], 0, sizeof(drfe_frustum_line));
            skip[(size_t)i] = !p || p->isBad();
            if (!skip[(size_t)i]) drfe_detail::frustum_line_of(p, fl[(size_t)i], descs.data() + 32 * (size_t)i);
        }
        const std::vector<drfe_keyline> kl = drfe_detail::keylines_of(pKF->mvKeyLines);
        const drfe_camera cam = drfe_detail::camera_of(*pKF);
        const auto Tcw = pKF->GetPose();
        std::vector<int32_t> bestIdx((size_t)n, -1), bestDist((size_t)n, 0);
        drfe_detail::check(drfe_lsd_fuse_search(c, drfe_detail::f32(Tcw), &cam, fl.data(), descs.data(), skip.data(), n, kl.data(), drfe_detail::u8(pKF->mLineDescriptors),
                                                nk, th, bestIdx.data(), bestDist.data()), c, "drfe_lsd_fuse_search");
        /* tracker: as in ORBmatcher::Fuse */
        if constexpr (!std::is_void<TrackerT>::value)
            if (tracker) {
                std::vector<int32_t> gated(bestIdx);
                for (int i = 0; i < n; i++)
                    if (bestDist[(size_t)i] > TH_LOW) gated[(size_t)i] = -1;
                tracker->FuseStore(pKF, vpMapLines, gated.data(), DRFE_LMAP_LINE, DRFE_LMAP_FUSE_NEIGHBOURS, nullptr);
            }
        int nFused = 0;
        for (int i = 0; i < n; i++) {
            MapLineT* pML = vpMapLines[(size_t)i];
            if (!pML || pML->isBad()) continue;
            if (bestIdx[(size_t)i] < 0 || bestDist[(size_t)i] > TH_LOW) continue;
            MapLineT* pMLinKF = pKF->GetMapLine((size_t)bestIdx[(size_t)i]);
            if (pMLinKF) {
                if (!pMLinKF->isBad()) {
                    if (pMLinKF->Observations() > pML->Observations()) pML->Replace(pMLinKF);
                    else pMLinKF->Replace(pML);
                }
            } else {
                pML->AddObservation(pKF, (size_t)bestIdx[(size_t)i]);
                pKF->AddMapLine(pML, (size_t)bestIdx[(size_t)i]);
            }
            nFused++;
        }
        return nFused;
    }

    /* ---- src/LSDmatcher.cpp:750-882 ---- */
    template <class KeyFrameT, class MatT, class MapLineT>
    int Fuse(KeyFrameT* pKF, MatT Scw, const std::vector<MapLineT*>& vpLines, float th, std::vector<MapLineT*>& vpReplaceLine)
    {
        drfe_ctx* c = Context();
        const std::set<MapLineT*> spAlreadyFound = pKF->GetMapLines();
        const int n = (int)vpLines.size(), nk = (int)pKF->mvKeyLines.size();
        std::vector<drfe_frustum_line> fl((size_t)n);
        std::vector<uint8_t> descs((size_t)n * 32), skip((size_t)n);
        for (int i = 0; i < n; i++) {
            MapLineT* p = vpLines[(size_t)i];
            std::memset(&fl[(size_t)i], 0, sizeof(drfe_frustum_line));
            skip[(size_t)i] = !p || p->isBad() || spAlreadyFound.count(p);
            if (!skip[(size_t)i]) drfe_detail::frustum_line_of(p, fl[(size_t)i], descs.data() + 32 * (size_t)i);
        }
        const std::vector<drfe_keyline> kl = drfe_detail::keylines_of(pKF->mvKeyLines);
        const drfe_camera cam = drfe_detail::camera_of(*pKF);
        std::vector<int32_t> bestIdx((size_t)n, -1), bestDist((size_t)n, 0);
        drfe_detail::check(drfe_lsd_fuse_search_sim3(c, drfe_detail::f32(Scw), &cam, fl.data(), descs.data(), skip.data(), n, kl.data(), drfe_detail::u8(pKF->mLineDescriptors),
                                                     nk, th, bestIdx.data(), bestDist.data()), c, "drfe_lsd_fuse_search_sim3");
        int nFused = 0;
        for (int i = 0; i < n; i++) {
            if (skip[(size_t)i] || bestIdx[(size_t)i] < 0 || bestDist[(size_t)i] > TH_LOW) continue;
            MapLineT* pML = vpLines[(size_t)i];
            MapLineT* pMLinKF = pKF->GetMapLine((size_t)bestIdx[(size_t)i]);
            if (pMLinKF) {
                if (!pMLinKF->isBad()) vpReplaceLine[(size_t)i] = pMLinKF;
            } else {
                pML->AddObservation(pKF, (size_t)bestIdx[(size_t)i]);
                pKF->AddMapLine(pML, (size_t)bestIdx[(size_t)i]);
            }
            nFused++;
        }
        return nFused;
    }

    /* src/LSDmatcher.cpp:316-332 on two 1 x 32 CV_8U rows */
    template <class MatT>
    static typename std::enable_if<std::is_class<MatT>::value, int>::type
    DescriptorDistance(const MatT& a, const MatT& b) { return DescriptorDistance(drfe_detail::u8(a), drfe_detail::u8(b)); }

    /* ---- flat forms (descriptor rows / key lines / records handed over directly: what the templates above call, for callers that
     * hold the flattened data already - tests/native/members_caller.cpp) ---- */
    /* SearchByDescriptor(KeyFrame* pKF, Frame& currentF, vpMapLineMatches), src/LSDmatcher.cpp:242-279: descKF / descF = the LBD rows,
     * kfHasLine[i] = pKF's line i has a MapLine; matches[line of currentF] = line of pKF or -1 */
    int SearchByDescriptor(drfe_ctx* ctx, const drfe_cv::Mat& descKF, const std::vector<uint8_t>& kfHasLine, const drfe_cv::Mat& descF,
                           std::vector<int32_t>& matches)
    {
        int n = 0;
        matches.assign(descF.rows, -1);
        drfe_detail::check(drfe_lsd_search_by_descriptor(ctx, descKF.data, descKF.rows, descF.data, descF.rows, kfHasLine.data(), 0, matches.data(), &n),
                           ctx, "drfe_lsd_search_by_descriptor");
        return n;
    }
    /* SearchByDescriptor(KeyFrame*, KeyFrame*, ...) (:281-314) and SerachForInitialize(InitialFrame, CurrentFrame, LineMatches) (:213-240):
     * matches[line of the first] = line of the second or -1; trainHasLine NULL = all */
    int SearchByDescriptorKF(drfe_ctx* ctx, const drfe_cv::Mat& desc1, const drfe_cv::Mat& desc2, const std::vector<uint8_t>* trainHasLine,
                             std::vector<int32_t>& matches)
    {
        int n = 0;
        matches.assign(desc1.rows, -1);
        drfe_detail::check(drfe_lsd_search_by_descriptor(ctx, desc1.data, desc1.rows, desc2.data, desc2.rows, trainHasLine ? trainHasLine->data() : nullptr,
                                                         1, matches.data(), &n), ctx, "drfe_lsd_search_by_descriptor");
        return n;
    }
    int SerachForInitialize(drfe_ctx* ctx, const drfe_cv::Mat& descInitial, const drfe_cv::Mat& descCurrent, std::vector<std::pair<int, int>>& LineMatches)
    {
        std::vector<int32_t> m;
        const int n = SearchByDescriptorKF(ctx, descInitial, descCurrent, nullptr, m);
        LineMatches.clear();
        for (size_t i = 0; i < m.size(); i++) if (m[i] >= 0) LineMatches.push_back(std::make_pair((int)i, (int)m[i]));
        return n;
    }
    /* SearchForTriangulation(pKF1, pKF2, vMatchedPairs), :334-367 */
    int SearchForTriangulation(drfe_ctx* ctx, const drfe_cv::Mat& desc1, const drfe_cv::Mat& desc2, const std::vector<uint8_t>& has1,
                               const std::vector<uint8_t>& has2, std::vector<std::pair<size_t, size_t>>& vMatchedPairs)
    {
        int n = 0;
        std::vector<int32_t> m(desc1.rows, -1);
        drfe_detail::check(drfe_lsd_search_for_triangulation(ctx, desc1.data, desc1.rows, desc2.data, desc2.rows, has1.data(), has2.data(), m.data(), &n),
                           ctx, "drfe_lsd_search_for_triangulation");
        vMatchedPairs.clear();
        for (size_t i = 0; i < m.size(); i++) if (m[i] >= 0) vMatchedPairs.push_back(std::make_pair(i, (size_t)m[i]));
        return n;
    }
    /* SearchByProjection(CurrentFrame, LastFrame, th, bMono), :20-108: lastLines[i] = what the loop reads of LastFrame.mvpMapLines[i];
     * curMapLine in/out = index into lastLines or -1, curObs[i] = the MapLine current line i already holds has Observations() > 0 */
    int SearchByProjection(drfe_ctx* ctx, const float* TcwCur, const float* TcwLast, const drfe_camera& cam, const std::vector<drfe_map_line>& lastLines,
                           const std::vector<drfe_cv::KeyLine>& curLines, const drfe_cv::Mat& curDesc, const std::vector<uint8_t>* curObs,
                           std::vector<int32_t>& curMapLine, float th, bool bMono)
    {
        int n = 0;
        drfe_detail::check(drfe_lsd_search_by_projection_last(ctx, TcwCur, TcwLast, &cam, lastLines.data(), (int)lastLines.size(),
                                                              reinterpret_cast<const drfe_keyline*>(curLines.data()), curDesc.data, (int)curLines.size(), th,
                                                              bMono ? 1 : 0, mfNNratio, curObs ? curObs->data() : nullptr, curMapLine.data(), &n),
                           ctx, "drfe_lsd_search_by_projection_last");
        return n;
    }
    /* SearchByProjection(F, vpMapLines, th), :110-211 after Frame::isInFrustum(MapLine*) left its fields in `tracked` */
    int SearchByProjection(drfe_ctx* ctx, const std::vector<drfe_tracked_line>& tracked, const std::vector<drfe_cv::KeyLine>& curLines,
                           const drfe_cv::Mat& curDesc, const std::vector<uint8_t>* curObs, std::vector<int32_t>& curMapLine, float th = 3)
    {
        int n = 0;
        drfe_detail::check(drfe_lsd_search_by_projection_map(ctx, tracked.data(), (int)tracked.size(), reinterpret_cast<const drfe_keyline*>(curLines.data()),
                                                             curDesc.data, (int)curLines.size(), th, mfNNratio, curObs ? curObs->data() : nullptr,
                                                             curMapLine.data(), &n), ctx, "drfe_lsd_search_by_projection_map");
        return n;
    }
    /* the search of Fuse(pKF, vpMapLines, th), :884-1015: bestIdx / bestDist per map line; the caller applies `<= TH_LOW` and the
     * Replace / AddObservation surgery on its map graph */
    void FuseSearch(drfe_ctx* ctx, const float* Tcw, const drfe_camera& cam, const std::vector<drfe_frustum_line>& lines, const drfe_cv::Mat& descs,
                    const std::vector<uint8_t>& skip, const std::vector<drfe_cv::KeyLine>& kfLines, const drfe_cv::Mat& kfDesc, float th,
                    std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist)
    {
        bestIdx.assign(lines.size(), -1); bestDist.assign(lines.size(), 0);
        drfe_detail::check(drfe_lsd_fuse_search(ctx, Tcw, &cam, lines.data(), descs.data, skip.data(), (int)lines.size(),
                                                reinterpret_cast<const drfe_keyline*>(kfLines.data()), kfDesc.data, (int)kfLines.size(), th, bestIdx.data(),
                                                bestDist.data()), ctx, "drfe_lsd_fuse_search");
    }
    /* src/LSDmatcher.cpp:316-332: cv::norm(a, b, NORM_HAMMING) of two 32-byte LBD rows */
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b)
    {
        int dist = 0;
        for (int i = 0; i < 32; i++) dist += __builtin_popcount((unsigned)(a[i] ^ b[i]));
        return dist;
    }
protected:
    float mfNNratio; bool mbCheckOrientation;
};

}  // namespace Planar_SLAM

/* include/LSDextractor.h:342-350 (global namespace in the reference).
 * The reference reaches this class through `LineSegment* mpLineSegment` (include/Frame.h:157), a member no constructor ever
 * initialises: `mpLineSegment->ExtractLineSegment(...)` (src/Frame.cc:241) works there only because the method touches no member.
 * The same holds here: ExtractLineSegment reads NO member of `this` - the object is default-constructible and empty - and takes its
 * context from the calling thread's binding (LineSegment::BindThread, LSDmatcher::BindThread or ORBmatcher::BindThread), else from
 * the process-wide one (LineSegment::BindProcess: Frame::Frame starts a fresh thread for ExtractLSD on every frame, src/Frame.cc:129,
 * which has no binding of its own; calls through the process-wide context are serialised). */
class LineSegment {
public:
    LineSegment() {}
    explicit LineSegment(drfe_ctx* ctx) { BindThread(ctx); }
    static void BindThread(drfe_ctx* ctx) { Planar_SLAM::drfe_detail::thread_ctx() = ctx; }
    static void BindProcess(drfe_ctx* ctx) { std::lock_guard<std::mutex> g(process_mutex()); process_ctx() = ctx; }
    /* keylineFunctions[i] = normalised sp x ep: std::vector<Eigen::Vector3d> as in the reference (include/LSDextractor.h:349) when
     * built with -DDRFE_WITH_EIGEN, the three-double stand-in with the same element access otherwise */
    void ExtractLineSegment(const drfe_cv::Mat& img, std::vector<drfe_cv::KeyLine>& keylines, drfe_cv::Mat& ldesc,
                            std::vector<drfe_cv::Vector3d>& keylineFunctions, float /*scale*/ = 1.2f, int /*numOctaves*/ = 1)
    {
        drfe_ctx* ctx = Planar_SLAM::drfe_detail::thread_ctx();
        std::unique_lock<std::mutex> guard;
        if (!ctx) {
            guard = std::unique_lock<std::mutex>(process_mutex());
            ctx = process_ctx();
            if (!ctx) throw std::runtime_error("LineSegment: no context bound (LineSegment::BindThread / BindProcess)");
        }
        const int cap = 40;                                            /* lsdNFeatures, src/LSDextractor.cpp:20-28 */
        std::vector<drfe_keyline> kl(cap);
        drfe_cv::Mat desc = drfe_cv::mat_u8(cap, 32);
        std::vector<double> lf(3 * cap);
        int n = 0, found = 0;
        Planar_SLAM::drfe_detail::check(drfe_lsd_extract(ctx, drfe_cv::mat_data(img), img.cols, img.rows, drfe_cv::mat_step(img), cap,
                                                         kl.data(), desc.data, lf.data(), cap, &n, &found), ctx, "drfe_lsd_extract");
        keylines.resize(n);
        keylineFunctions.clear();
        for (int i = 0; i < n; i++) {
            drfe_cv::KeyLine& k = keylines[i];
            k.angle = kl[i].angle; k.class_id = kl[i].class_id; k.octave = kl[i].octave;
            k.pt.x = kl[i].pt_x; k.pt.y = kl[i].pt_y; k.response = kl[i].response; k.size = kl[i].size;
            k.startPointX = kl[i].start_point_x; k.startPointY = kl[i].start_point_y; k.endPointX = kl[i].end_point_x; k.endPointY = kl[i].end_point_y;
            k.sPointInOctaveX = kl[i].s_point_in_octave_x; k.sPointInOctaveY = kl[i].s_point_in_octave_y;
            k.ePointInOctaveX = kl[i].e_point_in_octave_x; k.ePointInOctaveY = kl[i].e_point_in_octave_y;
            k.lineLength = kl[i].line_length; k.numOfPixels = kl[i].num_of_pixels;
            keylineFunctions.push_back(drfe_cv::Vector3d(lf[3 * i], lf[3 * i + 1], lf[3 * i + 2]));
        }
        ldesc = drfe_cv::mat_u8(n, 32);
        if (n) std::memcpy(ldesc.data, desc.data, (size_t)n * 32);
    }
private:
    static drfe_ctx*& process_ctx() { static drfe_ctx* c = nullptr; return c; }
    static std::mutex& process_mutex() { static std::mutex m; return m; }
};


/* Tracking::TrackManhattanFrame (src/Tracking.cc:1336-1527) over drfe_manhattan_track_host: one call, as the reference makes it
 * (Tracking::Track chains three, :328-332).  With -DDRFE_WITH_OPENCV, R is the reference's 3x3 CV_32F cv::Mat and SN / FL are the
 * reference's SurfaceNormal / FrameLine (include/LSDextractor.h:34-41, 141-189); without it, the stand-ins below.  The overload
 * with `frame` appends what ProjectSN2MF pushes onto the frame - vSurfaceNormalx/y/z (FramePosition), vSurfacePointx/y/z
 * (cameraPosition), vVanishingLinex/y/z (the reference's four-point pair: two default points, then p, q) and
 * vVaishingLinePCx/y/z (rndpts3d) - in its order, and sets inline[i] for the normals inside a cone (bsurfacenormal_inline). */
namespace drfe {
#ifdef DRFE_WITH_OPENCV
using RotationMat = cv::Mat;
inline void rotation_get(const cv::Mat& m, float R[9]) { for (int i = 0; i < 9; i++) R[i] = m.at<float>(i / 3, i % 3); }
inline cv::Mat rotation_make(const float R[9]) { cv::Mat m(3, 3, CV_32F); for (int i = 0; i < 9; i++) m.at<float>(i / 3, i % 3) = R[i]; return m; }
#else
struct Point2i { int x, y; };
struct Point2d { double x, y; };
struct Point3f { float x, y, z; };
struct Point3d { double x, y, z; };
struct Mat33f { float v[9]; };             /* row-major 3x3 CV_32F */
using RotationMat = Mat33f;
inline void rotation_get(const Mat33f& m, float R[9]) { std::memcpy(R, m.v, sizeof(m.v)); }
inline Mat33f rotation_make(const float R[9]) { Mat33f m; std::memcpy(m.v, R, sizeof(m.v)); return m; }
struct SurfaceNormal { Point3f normal, cameraPosition; Point2i FramePosition; };
struct RandomPoint3d { Point3d pos; };
struct FrameLine { Point2d p, q; Point3d direction; std::vector<RandomPoint3d> rndpts3d; };
/* the members of Frame that ProjectSN2MF fills (include/Frame.h) */
struct ManhattanFrameOut {
    std::vector<Point2i> vSurfaceNormalx, vSurfaceNormaly, vSurfaceNormalz;
    std::vector<Point3f> vSurfacePointx, vSurfacePointy, vSurfacePointz;
    std::vector<std::vector<Point2d>> vVanishingLinex, vVanishingLiney, vVanishingLinez;
    std::vector<RandomPoint3d> vVaishingLinePCx, vVaishingLinePCy, vVaishingLinePCz;
};
#endif

namespace detail {
template <class SN, class FL>
inline RotationMat track_manhattan(const RotationMat& Rin, const std::vector<SN>& sn, const std::vector<FL>& lines,
                                   std::vector<uint16_t>* rb, std::vector<uint16_t>* lb)
{
    float R[9], Rout[9];
    rotation_get(Rin, R);
    std::vector<drfe_surface_normal> recs(sn.size());
    for (size_t i = 0; i < sn.size(); i++) {
        drfe_surface_normal& r = recs[i];
        r.normal[0] = sn[i].normal.x; r.normal[1] = sn[i].normal.y; r.normal[2] = sn[i].normal.z;
        r.camera_position[0] = sn[i].cameraPosition.x; r.camera_position[1] = sn[i].cameraPosition.y;
        r.camera_position[2] = sn[i].cameraPosition.z;
        r.frame_x = sn[i].FramePosition.x; r.frame_y = sn[i].FramePosition.y;
    }
    std::vector<double> dirs(3 * lines.size());
    for (size_t l = 0; l < lines.size(); l++) {
        dirs[3 * l] = lines[l].direction.x; dirs[3 * l + 1] = lines[l].direction.y; dirs[3 * l + 2] = lines[l].direction.z;
    }
    if (rb) rb->assign(sn.size(), 0);
    if (lb) lb->assign(lines.size(), 0);
    const int rc = drfe_manhattan_track_host(R, recs.data(), (int)recs.size(), dirs.data(), (int)lines.size(), 1, Rout, nullptr,
                                             rb ? rb->data() : nullptr, lb ? lb->data() : nullptr);
    if (rc != DRFE_OK) throw std::runtime_error("drfe_manhattan_track_host failed");
    return rotation_make(Rout);
}
}  // namespace detail

template <class SN, class FL>
inline RotationMat TrackManhattanFrame(RotationMat& mLastRcm, std::vector<SN>& vSurfaceNormal, std::vector<FL>& vVanishingDirection)
{
    return detail::track_manhattan(mLastRcm, vSurfaceNormal, vVanishingDirection, nullptr, nullptr);
}

template <class SN, class FL, class Frame>
inline RotationMat TrackManhattanFrame(RotationMat& mLastRcm, std::vector<SN>& vSurfaceNormal, std::vector<FL>& vVanishingDirection,
                                       Frame& frame, std::vector<bool>& bsurfacenormal_inline)
{
    std::vector<uint16_t> rb, lb;
    RotationMat R = detail::track_manhattan(mLastRcm, vSurfaceNormal, vVanishingDirection, &rb, &lb);
    if (bsurfacenormal_inline.size() < vSurfaceNormal.size()) bsurfacenormal_inline.resize(vSurfaceNormal.size(), false);
    for (size_t i = 0; i < rb.size(); i++)
        if (rb[i] & DRFE_MANHATTAN_INLINE_BIT) bsurfacenormal_inline[i] = true;
    for (int a = 0; a < 3; a++) {                     /* ProjectSN2MF runs axis by axis: x, then y, then z */
        auto& pos = a == 0 ? frame.vSurfaceNormalx : a == 1 ? frame.vSurfaceNormaly : frame.vSurfaceNormalz;
        auto& pts = a == 0 ? frame.vSurfacePointx : a == 1 ? frame.vSurfacePointy : frame.vSurfacePointz;
        auto& vl = a == 0 ? frame.vVanishingLinex : a == 1 ? frame.vVanishingLiney : frame.vVanishingLinez;
        auto& pc = a == 0 ? frame.vVaishingLinePCx : a == 1 ? frame.vVaishingLinePCy : frame.vVaishingLinePCz;
        for (size_t i = 0; i < rb.size(); i++)
            if (rb[i] & (1u << a)) {
                pos.push_back(vSurfaceNormal[i].FramePosition);
                pts.push_back(vSurfaceNormal[i].cameraPosition);
            }
        for (size_t l = 0; l < lb.size(); l++)
            if (lb[l] & (1u << a)) {
                typename std::decay<decltype(vl)>::type::value_type pair(2);   /* vector<Point2d> pointPair(2), then p, q pushed */
                pair.push_back(vVanishingDirection[l].p);
                pair.push_back(vVanishingDirection[l].q);
                vl.push_back(pair);
                for (const auto& p : vVanishingDirection[l].rndpts3d) pc.push_back(p);
            }
    }
    return R;
}
}  // namespace drfe

/* PlaneMatcher (include/PlaneMatcher.h:10-31, src/PlaneMatcher.cpp) over drfe_plane_match_host / drfe_plane_match_status_host,
 * and Map::FlagMatchedPlanePoints (src/Map.cc:406-431) over drfe_plane_flag_points_host: no context, no device.  Templates over
 * the frame / map-plane / map-point types that read only the members the reference reads
 *   Frame:    mnPlaneNum, mTcw (4x4 float), mvPlaneCoefficients (4x1 float each), mvpMapPlanes, mvpParallelPlanes,
 *             mvpVerticalPlanes, mbNewPlane
 *   MapPlane: isBad(), GetWorldPos() (4x1 float), mvPlanePoints->points[k].x / y / z
 *   MapPoint: GetWorldPos() (3x1 float), SetAssociatedWithPlaneFlag(bool)
 * through Mat::ptr<float>(row), which cv::Mat and the stand-in share.  The three pointer vectors are written where the reference
 * writes them and left alone elsewhere (the reference does not reset them).  PlaneMatcher::Fuse is declared in the reference
 * but never defined, so it has no counterpart.  DESIGN.md section 12. */
namespace Planar_SLAM {
namespace drfe_detail {
template <class M> inline float mat_f(const M& m, int r, int c = 0) { return m.template ptr<float>(r)[c]; }
template <class FrameT> inline void frame_planes_of(FrameT& pF, float Tcw[16], std::vector<float>& coefs)
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) Tcw[r * 4 + c] = mat_f(pF.mTcw, r, c);
    coefs.resize(4 * (size_t)pF.mnPlaneNum);
    for (int i = 0; i < pF.mnPlaneNum; i++)
        for (int k = 0; k < 4; k++) coefs[4 * (size_t)i + k] = mat_f(pF.mvPlaneCoefficients[i], k);
}
}  // namespace drfe_detail

class PlaneMatcher {
public:
    PlaneMatcher(float dTh = 0.1, float aTh = 0.86, float verTh = 0.08716, float parTh = 0.9962) : dTh(dTh), aTh(aTh), verTh(verTh), parTh(parTh) {}

    /* src/PlaneMatcher.cpp:11-91; Rwc_MF is unused, as in the reference */
    template <class FrameT, class MapPlaneT, class MatT>
    int SearchMapByCoefficients(FrameT& pF, const std::vector<MapPlaneT*>& vpMapPlanes, MatT /*Rwc_MF*/)
    {
        pF.mbNewPlane = false;
        float Tcw[16];
        std::vector<float> coefs;
        drfe_detail::frame_planes_of(pF, Tcw, coefs);
        const int M = (int)vpMapPlanes.size(), P = pF.mnPlaneNum;
        std::vector<float> mc(4 * (size_t)M, 0.f), xyz;
        std::vector<uint8_t> bad(M);
        std::vector<int32_t> off(M + 1, 0);
        for (int j = 0; j < M; j++) {
            MapPlaneT* pl = vpMapPlanes[j];
            bad[j] = pl->isBad() ? 1 : 0;
            if (!bad[j]) {                    /* a bad plane's position and cloud are never read */
                const auto pW = pl->GetWorldPos();
                for (int k = 0; k < 4; k++) mc[4 * (size_t)j + k] = drfe_detail::mat_f(pW, k);
                for (const auto& p : pl->mvPlanePoints->points) {
                    xyz.push_back(p.x); xyz.push_back(p.y); xyz.push_back(p.z);
                }
            }
            off[j + 1] = (int32_t)(xyz.size() / 3);
        }
        std::vector<int32_t> mi(P, -1), pi(P, -1), vi(P, -1);
        const drfe_plane_match_params prm = {dTh, aTh, verTh, parTh};
        int n = 0;
        if (drfe_plane_match_host(&prm, Tcw, coefs.data(), P, mc.data(), bad.data(), off.data(), xyz.data(), M, mi.data(), pi.data(),
                                  vi.data(), &n) != DRFE_OK)
            throw std::runtime_error("drfe_plane_match_host failed");
        for (int i = 0; i < P; i++) {
            if (mi[i] >= 0) pF.mvpMapPlanes[i] = vpMapPlanes[mi[i]];
            if (pi[i] >= 0) pF.mvpParallelPlanes[i] = vpMapPlanes[pi[i]];
            if (vi[i] >= 0) pF.mvpVerticalPlanes[i] = vpMapPlanes[vi[i]];
        }
        return n;
    }

    /* src/PlaneMatcher.cpp:94-201 over the planes already in mvpMapPlanes (vpMapPlanes is not read); without MF_contrast the
     * reference compares with an uninitialised angle_MF, taken as 0 here (the call then returns true) */
    template <class FrameT, class MapPlaneT, class MatT>
    bool bMatchStatus(FrameT& pF, const std::vector<MapPlaneT*>& /*vpMapPlanes*/, const bool MF_contrast, MatT Rwc_MF)
    {
        pF.mbNewPlane = false;
        float Tcw[16], R[9];
        std::vector<float> coefs;
        drfe_detail::frame_planes_of(pF, Tcw, coefs);
        const int P = pF.mnPlaneNum;
        if (P < 2) return true;
        std::vector<float> mc(4 * (size_t)P, 0.f);
        std::vector<uint8_t> matched(P, 0);
        for (int i = 0; i < P; i++) {
            auto* pl = pF.mvpMapPlanes[i];
            if (!pl || pl->isBad()) continue;
            matched[i] = 1;
            const auto pW = pl->GetWorldPos();
            for (int k = 0; k < 4; k++) mc[4 * (size_t)i + k] = drfe_detail::mat_f(pW, k);
        }
        if (MF_contrast)
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) R[r * 3 + c] = drfe_detail::mat_f(Rwc_MF, r, c);
        const drfe_plane_match_params prm = {dTh, aTh, verTh, parTh};
        int st = 1;
        if (drfe_plane_match_status_host(&prm, Tcw, coefs.data(), P, mc.data(), matched.data(), MF_contrast ? 1 : 0,
                                         MF_contrast ? R : nullptr, &st) != DRFE_OK)
            throw std::runtime_error("drfe_plane_match_status_host failed");
        return st != 0;
    }

protected:
    float dTh, aTh, verTh, parTh;
};
}  // namespace Planar_SLAM

namespace drfe {
/* Map::FlagMatchedPlanePoints(pF, dTh) (src/Map.cc:406-431) with the map's point set passed in (mspMapPoints; the caller holds
 * the map mutex): SetAssociatedWithPlaneFlag(true) on every map point within 0.5 of a matched frame plane.  dTh is unused, as
 * in the reference.  Returns the reference's (discarded) nMatches. */
template <class FrameT, class MapPointSet>
inline int FlagMatchedPlanePoints(FrameT& pF, const MapPointSet& mspMapPoints, const float& /*dTh*/)
{
    float Tcw[16];
    std::vector<float> coefs;
    Planar_SLAM::drfe_detail::frame_planes_of(pF, Tcw, coefs);
    const int P = pF.mnPlaneNum;
    std::vector<int32_t> mi(P);
    for (int i = 0; i < P; i++) mi[i] = pF.mvpMapPlanes[i] ? 0 : -1;
    std::vector<typename MapPointSet::value_type> pts(mspMapPoints.begin(), mspMapPoints.end());
    std::vector<float> xyz(3 * pts.size());
    for (size_t p = 0; p < pts.size(); p++) {
        const auto pW = pts[p]->GetWorldPos();
        for (int k = 0; k < 3; k++) xyz[3 * p + k] = Planar_SLAM::drfe_detail::mat_f(pW, k);
    }
    std::vector<uint8_t> flags(pts.size(), 0);
    int n = 0;
    if (drfe_plane_flag_points_host(Tcw, coefs.data(), P, mi.data(), xyz.data(), (int)pts.size(), flags.data(), &n) != DRFE_OK)
        throw std::runtime_error("drfe_plane_flag_points_host failed");
    for (size_t p = 0; p < pts.size(); p++)
        if (flags[p]) pts[p]->SetAssociatedWithPlaneFlag(true);
    return n;
}

/* MapPlane::UpdateCoefficientsAndPoints (src/MapPlane.cc:298-371) over drfe_map_plane_update_host / drfe_map_plane_rebuild_host:
 * the map plane's mvPlanePoints is replaced by a new cloud of the same type (a smart pointer is reseated, so holders of the old
 * cloud keep it, as in the reference; through a raw pointer the pointee is overwritten).  Reads
 *   Frame:    mTcw (4x4 float), mvPlanePoints[id].points[k].x / y / z
 *   KeyFrame: GetPoseInverse() (4x4 float), mvPlanePoints[idx].points
 *   MapPlane: mvPlanePoints (pointer to a cloud with .points), GetObservations() (pairs (KeyFrame*, index), iterated in order)
 * New points are value-initialised and get x / y / z; a PCL cloud also gets width = n, height = 1, is_dense.  The reference's
 * SAC segmentation afterwards writes only locals and has no counterpart.  Call sites: DESIGN.md section 13, INTEGRATION.md. */
namespace drfe_detail_mp {
template <class M> inline void pose16(const M& m, float T[16])
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) T[r * 4 + c] = m.template ptr<float>(r)[c];
}
template <class CloudT> inline void append_xyz(const CloudT& cl, std::vector<float>& xyz)
{
    for (const auto& p : cl.points) {
        xyz.push_back(p.x); xyz.push_back(p.y); xyz.push_back(p.z);
    }
}
template <class C> inline auto set_shape(C& c, size_t n, int) -> decltype(c.width = 0, c.height = 0, c.is_dense = true, void())
{
    c.width = (decltype(c.width))n; c.height = 1; c.is_dense = true;
}
template <class C> inline void set_shape(C&, size_t, long) {}
template <class C> inline void reseat(C*& p, C&& fresh) { *p = std::move(fresh); }
template <class P, class C> inline void reseat(P& p, C&& fresh) { p = P(new C(std::move(fresh))); }
template <class MapPlaneT> inline void replace_cloud(MapPlaneT& pMP, const std::vector<float>& xyz, int n)
{
    typedef typename std::remove_reference<decltype(*pMP.mvPlanePoints)>::type CloudT;
    typedef typename std::decay<decltype(pMP.mvPlanePoints->points[0])>::type PointT;
    CloudT fresh;
    fresh.points.assign((size_t)n, PointT());
    for (int k = 0; k < n; k++) {
        fresh.points[k].x = xyz[3 * (size_t)k]; fresh.points[k].y = xyz[3 * (size_t)k + 1]; fresh.points[k].z = xyz[3 * (size_t)k + 2];
    }
    set_shape(fresh, (size_t)n, 0);
    reseat(pMP.mvPlanePoints, std::move(fresh));
}
}  // namespace drfe_detail_mp

/* pMP->UpdateCoefficientsAndPoints(F, id) (src/MapPlane.cc:336-371) */
template <class MapPlaneT, class FrameT>
inline void UpdateCoefficientsAndPoints(MapPlaneT& pMP, const FrameT& F, int id)
{
    float Tcw[16];
    drfe_detail_mp::pose16(F.mTcw, Tcw);
    std::vector<float> fx, mx;
    drfe_detail_mp::append_xyz(F.mvPlanePoints[id], fx);
    drfe_detail_mp::append_xyz(*pMP.mvPlanePoints, mx);
    const int nf = (int)(fx.size() / 3), nm = (int)(mx.size() / 3);
    std::vector<float> out(3 * ((size_t)nf + nm) + 3);
    int n = 0;
    if (drfe_map_plane_update_host(Tcw, fx.data(), nf, mx.data(), nm, out.data(), nf + nm, &n) != DRFE_OK)
        throw std::runtime_error("drfe_map_plane_update_host failed");
    drfe_detail_mp::replace_cloud(pMP, out, n);
}

/* pMP->UpdateCoefficientsAndPoints() (src/MapPlane.cc:298-334): the observations in GetObservations()'s iteration order */
template <class MapPlaneT>
inline void UpdateCoefficientsAndPoints(MapPlaneT& pMP)
{
    const auto observations = pMP.GetObservations();
    std::vector<float> Twc, xyz;
    std::vector<int32_t> off(1, 0);
    for (const auto& ob : observations) {
        float T[16];
        drfe_detail_mp::pose16(ob.first->GetPoseInverse(), T);
        Twc.insert(Twc.end(), T, T + 16);
        drfe_detail_mp::append_xyz(ob.first->mvPlanePoints[ob.second], xyz);
        off.push_back((int32_t)(xyz.size() / 3));
    }
    const int nobs = (int)off.size() - 1, total = off.back();
    std::vector<float> out(3 * (size_t)total + 3);
    int n = 0;
    if (drfe_map_plane_rebuild_host(nobs, Twc.data(), off.data(), xyz.data(), out.data(), total, &n) != DRFE_OK)
        throw std::runtime_error("drfe_map_plane_rebuild_host failed");
    drfe_detail_mp::replace_cloud(pMP, out, n);
}

/* LocalMapping::MapPlaneCulling (src/LocalMapping.cc:233-307) over drfe_plane_map_cull_batch on resident map `map` of ctx, or, with
 * ctx == nullptr, over drfe_plane_map_cull_host (no context, no device).  vpMapPlanes is mpMap->GetAllMapPlanes() (no null
 * entries), in the order the map was uploaded in; mlpRecentAddedMapPlanes is the thread's list, edited in place.  The entry decides;
 * this function applies: each event (replaced, survivor) through MapPlane::ReplaceWithoutRebuild(survivor) - the reference's
 * Replace (src/MapPlane.cc:197-271) without its closing pMP->UpdateCoefficientsAndPoints(), a member the integration adds because
 * mObservations and mbBad are protected -, then every rebuilt cloud from the entry, then SetBadFlag() and the
 * erasures of the list walk.  Reads
 *   MapPlane: isBad(), GetWorldPos() (4x1 float), mvPlanePoints, GetObservations() (std::map<KeyFrame*, size_t>), Observations(),
 *             mnFound, mnVisible, mnFirstKFid
 *   KeyFrame: GetPoseInverse() (4x4 float), mvPlanePoints[idx].points (x y z at the head of a point), mnId
 * Observation clouds are passed in place (pointer, count, sizeof(point)): nothing is copied unless a survivor is rebuilt.
 * Returns the number of merges.  DESIGN.md section 30. */
template <class MapPlaneT, class KeyFrameT, class ListT>
inline int MapPlaneCulling(drfe_ctx* ctx, int map, const std::vector<MapPlaneT*>& vpMapPlanes, ListT& mlpRecentAddedMapPlanes,
                           KeyFrameT* pCurrentKF, double dTh, double aTh)
{
    const int P = (int)vpMapPlanes.size();
    std::map<KeyFrameT*, int32_t> rank;                      /* pointer order, as the observation maps iterate */
    for (MapPlaneT* pl : vpMapPlanes)
        for (const auto& ob : pl->GetObservations()) rank[ob.first] = 0;
    std::vector<float> Twc(16 * rank.size() + 16);
    {
        int32_t k = 0;
        for (auto& e : rank) {
            drfe_detail_mp::pose16(e.first->GetPoseInverse(), &Twc[16 * (size_t)k]);
            e.second = k++;
        }
    }
    std::vector<int32_t> found(P), visible(P), nobs(P), first(P), obsOff(P + 1, 0), obsKf, obsIdx, obsN, cloudOff(P + 1, 0);
    std::vector<const float*> obsCloud;
    std::vector<float> coefs(4 * (size_t)P + 4, 0.f), xyz;
    std::vector<uint8_t> bad(P + 1, 0);
    typedef typename std::decay<decltype(vpMapPlanes[0]->mvPlanePoints->points[0])>::type PointT;
    static_assert(sizeof(PointT) % sizeof(float) == 0, "a cloud point is a whole number of floats");
    std::map<MapPlaneT*, int32_t> index;
    for (int p = 0; p < P; p++) {
        MapPlaneT* pl = vpMapPlanes[p];
        index[pl] = p;
        found[p] = pl->mnFound; visible[p] = pl->mnVisible; nobs[p] = pl->Observations(); first[p] = (int)pl->mnFirstKFid;
        bad[p] = pl->isBad() ? 1 : 0;
        for (const auto& ob : pl->GetObservations()) {
            const auto& cl = ob.first->mvPlanePoints[ob.second];
            obsKf.push_back(rank[ob.first]);
            obsIdx.push_back((int32_t)ob.second);
            obsN.push_back((int32_t)cl.points.size());
            obsCloud.push_back(cl.points.empty() ? nullptr : &cl.points[0].x);
        }
        obsOff[p + 1] = (int32_t)obsKf.size();
        if (!ctx && !bad[p]) {                /* a bad plane's position and cloud are never read */
            const auto pW = pl->GetWorldPos();
            for (int k = 0; k < 4; k++) coefs[4 * (size_t)p + k] = pW.template ptr<float>(k)[0];
            drfe_detail_mp::append_xyz(*pl->mvPlanePoints, xyz);
        }
        cloudOff[p + 1] = (int32_t)(xyz.size() / 3);
    }
    std::vector<int32_t> recent;
    for (MapPlaneT* pl : mlpRecentAddedMapPlanes) recent.push_back(index.count(pl) ? index[pl] : -1);
    int64_t cap = 0;
    for (int32_t n : obsN) cap += n;
    if (cap > INT32_MAX) throw std::runtime_error("MapPlaneCulling: the observation clouds outgrow 2^31 points");
    drfe_plane_cull_in in = {};
    in.n_planes = P; in.n_kfs = (int32_t)rank.size(); in.n_recent = (int32_t)recent.size(); in.current_kf_id = (int)pCurrentKF->mnId;
    in.dTh = dTh; in.aTh = aTh;
    in.found = found.data(); in.visible = visible.data(); in.n_obs = nobs.data(); in.first_kf_id = first.data();
    in.obs_offsets = obsOff.data(); in.obs_kf = obsKf.data(); in.obs_idx = obsIdx.data();
    in.obs_cloud = obsCloud.data(); in.obs_cloud_n = obsN.data(); in.obs_cloud_stride = (int32_t)sizeof(PointT);
    in.Twc = Twc.data(); in.recent = recent.data();
    std::vector<int32_t> events(2 * (size_t)P + 2), oN(P + 1), oF(P + 1), oV(P + 1), rebuilt(P + 1), rOff(P + 2);
    std::vector<uint8_t> oBad(P + 1), verdicts(recent.size() + 1);
    std::vector<float> rXyz(3 * (size_t)cap + 3);
    drfe_plane_cull_out out = {};
    out.events = events.data(); out.bad = oBad.data(); out.n_obs = oN.data(); out.found = oF.data(); out.visible = oV.data();
    out.rebuilt = rebuilt.data(); out.rebuilt_offsets = rOff.data(); out.rebuilt_xyz = rXyz.data(); out.rebuilt_capacity = (int32_t)cap;
    out.verdicts = verdicts.data();
    const int rc = ctx ? drfe_plane_map_cull_batch(ctx, map, &in, 0, &out, nullptr)
                       : drfe_plane_map_cull_host(&in, coefs.data(), bad.data(), cloudOff.data(), xyz.data(), &out);
    if (rc != DRFE_OK) throw std::runtime_error(ctx ? "drfe_plane_map_cull_batch failed" : "drfe_plane_map_cull_host failed");
    for (int e = 0; e < out.n_events; e++) vpMapPlanes[events[2 * e]]->ReplaceWithoutRebuild(vpMapPlanes[events[2 * e + 1]]);
    std::vector<float> one;
    for (int k = 0; k < out.n_rebuilt; k++) {
        one.assign(rXyz.begin() + 3 * (size_t)rOff[k], rXyz.begin() + 3 * (size_t)rOff[k + 1]);
        drfe_detail_mp::replace_cloud(*vpMapPlanes[rebuilt[k]], one, rOff[k + 1] - rOff[k]);
    }
    size_t k = 0;
    for (auto lit = mlpRecentAddedMapPlanes.begin(); lit != mlpRecentAddedMapPlanes.end(); k++) {
        const int v = verdicts[k];
        if (v == DRFE_PLANE_CULL_BAD_BY_RATIO || v == DRFE_PLANE_CULL_BAD_BY_OBSERVATIONS) (*lit)->SetBadFlag();
        if (v == DRFE_PLANE_CULL_KEPT) ++lit;
        else lit = mlpRecentAddedMapPlanes.erase(lit);
    }
    return out.n_events;
}
/* MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (src/MapPoint.cc:288-411) and MapLine::ComputeDistinctiveDescriptors
 * / UpdateAverageDir (src/MapLine.cpp:241-362) over drfe_map_point_upkeep_host / drfe_map_line_upkeep_host and the batch entries.
 * Reads only public accessors:
 *   MapPoint / MapLine: isBad(), GetObservations() (pairs (KeyFrame*, index), iterated in order; a std::map), GetReferenceKeyFrame(),
 *                       GetWorldPos() (3x1 float Mat / Vector6d)
 *   KeyFrame:           isBad(), GetCameraCenter() (3x1 float Mat), mDescriptors / mLineDescriptors (rows of 32 bytes),
 *                       mvKeysUn / mvKeyLines (.octave), mvScaleFactors, mnScaleLevels
 * observations[pRefKF] is operator[] on the reference's copy: a ref keyframe missing from the observations reads keypoint 0.
 * MapPoint's mDescriptor / mNormalVector / mfMaxDistance / mfMinDistance are protected, so a point's results are returned
 * (INTEGRATION.md section 4g shows the two method bodies); MapLine's members are public and written here under its mutexes.
 * DESIGN.md section 14. */
struct MapPointUpkeep {
    int status = 0;                  /* DRFE_UPKEEP_* bits of the halves computed (0: the point is unchanged) */
    int best_obs = -1;               /* the winning observation's position in GetObservations()'s order */
    uint8_t descriptor[32] = {0};
    float normal[3] = {0, 0, 0};
    float max_distance = 0, min_distance = 0;
};
struct MapLineUpkeep {
    int status = 0;
    int best_obs = -1;
    uint8_t descriptor[32] = {0};
    double normal[3] = {0, 0, 0};
    float max_distance = 0, min_distance = 0;
};
namespace drfe_detail_mu {
template <class KF> inline const uint8_t* row_of(KF* kf, size_t idx, std::false_type) { return kf->mDescriptors.template ptr<uint8_t>((int)idx); }
template <class KF> inline const uint8_t* row_of(KF* kf, size_t idx, std::true_type) { return kf->mLineDescriptors.template ptr<uint8_t>((int)idx); }
template <class KF> inline int octave_of(KF* kf, size_t idx, std::false_type) { return kf->mvKeysUn[idx].octave; }
template <class KF> inline int octave_of(KF* kf, size_t idx, std::true_type) { return kf->mvKeyLines[idx].octave; }
template <class P> inline void world_of(const P& m, std::vector<float>& wf, std::vector<double>&, std::false_type)
{
    for (int k = 0; k < 3; k++) wf.push_back(m.template ptr<float>(k)[0]);
}
template <class P> inline void world_of(const P& v, std::vector<float>&, std::vector<double>& wd, std::true_type)
{
    for (int k = 0; k < 6; k++) wd.push_back(v(k));
}

/* the flat inputs of one call: a keyframe table built from the keyframes the items name, items in the caller's order */
struct Scene {
    std::map<const void*, int32_t> index;
    std::vector<float> center, scale, worldF;
    std::vector<double> worldD;
    std::vector<uint8_t> kfBad, bad, desc;
    std::vector<int32_t> off{0}, obsKf, refKf, refLevel;
    int nLevels = 0;
    template <class KF> int32_t kf(KF* p)
    {
        const auto r = index.emplace((const void*)p, (int32_t)kfBad.size());
        if (r.second) {
            const auto C = p->GetCameraCenter();
            for (int k = 0; k < 3; k++) center.push_back(C.template ptr<float>(k)[0]);
            kfBad.push_back(p->isBad() ? 1 : 0);
        }
        return r.first->second;
    }
    /* item x (null: a bad item without observations, left unchanged) */
    template <class Line, class ItemT> void add(ItemT* x)
    {
        const bool isBad = !x || x->isBad();
        bad.push_back(isBad ? 1 : 0);
        int32_t ref = 0, level = 0;
        if (x) {
            const auto observations = x->GetObservations();
            for (const auto& ob : observations) {
                obsKf.push_back(kf(ob.first));
                const uint8_t* r = row_of(ob.first, ob.second, Line());
                desc.insert(desc.end(), r, r + 32);
            }
            world_of(x->GetWorldPos(), worldF, worldD, Line());
            auto* pRef = x->GetReferenceKeyFrame();
            if (!isBad && !observations.empty() && pRef) {
                ref = kf(pRef);
                const auto f = observations.find(pRef);
                level = octave_of(pRef, f == observations.end() ? (size_t)0 : f->second, Line());
                if (!nLevels) {
                    nLevels = pRef->mnScaleLevels;
                    scale.assign(pRef->mvScaleFactors.begin(), pRef->mvScaleFactors.begin() + nLevels);
                }
            }
        } else {
            for (int k = 0; k < (Line::value ? 0 : 3); k++) worldF.push_back(0.f);
            for (int k = 0; k < (Line::value ? 6 : 0); k++) worldD.push_back(0.0);
        }
        off.push_back((int32_t)obsKf.size());
        refKf.push_back(ref);
        refLevel.push_back(level);
    }
    drfe_upkeep_keyframes keyframes() const
    {
        return drfe_upkeep_keyframes{(int32_t)kfBad.size(), nLevels ? nLevels : 1, center.data(), kfBad.data(), nLevels ? scale.data() : &one};
    }
    drfe_upkeep_items items(bool line) const
    {
        return drfe_upkeep_items{(int32_t)bad.size(), 0, bad.data(), off.data(), obsKf.data(), desc.data(),
                                 line ? (const void*)worldD.data() : (const void*)worldF.data(), refKf.data(), refLevel.data()};
    }
    float one = 1.f;
};
template <class R> inline drfe_upkeep_out out_of(std::vector<R>& r, std::vector<int32_t>& best, std::vector<uint8_t>& desc, std::vector<uint8_t>& st,
                                                 std::vector<float>& mx, std::vector<float>& mn, std::vector<double>& nd, std::vector<float>& nf)
{
    const size_t n = r.size();
    best.resize(n); desc.resize(32 * n); st.resize(n); mx.resize(n); mn.resize(n); nd.resize(3 * n); nf.resize(3 * n);
    return drfe_upkeep_out{best.data(), desc.data(), nullptr, mx.data(), mn.data(), st.data(), nullptr};
}
/* runs fn over the items and fills one result per item */
template <class Line, class R, class ItemT, class Fn>
inline std::vector<R> run(const std::vector<ItemT*>& v, int what, Fn fn)
{
    Scene s;
    for (ItemT* x : v) s.add<Line>(x);
    std::vector<R> r(v.size());
    std::vector<int32_t> best; std::vector<uint8_t> desc, st; std::vector<float> mx, mn, nf; std::vector<double> nd;
    drfe_upkeep_out o = out_of(r, best, desc, st, mx, mn, nd, nf);
    o.normal = Line::value ? (void*)nd.data() : (void*)nf.data();
    const drfe_upkeep_keyframes k = s.keyframes();
    const drfe_upkeep_items it = s.items(Line::value);
    fn(what, &k, &it, &o);
    for (size_t i = 0; i < r.size(); i++) {
        r[i].status = st[i];
        r[i].best_obs = best[i];
        std::memcpy(r[i].descriptor, &desc[32 * i], 32);
        for (int c = 0; c < 3; c++) r[i].normal[c] = Line::value ? (decltype(r[i].normal[0]))nd[3 * i + c] : (decltype(r[i].normal[0]))nf[3 * i + c];
        r[i].max_distance = mx[i];
        r[i].min_distance = mn[i];
    }
    return r;
}
/* the reference's writes of MapLine's public members, under its mutexes */
template <class MapLineT> inline void apply_line(MapLineT& ml, const MapLineUpkeep& r)
{
    if (r.status & DRFE_UPKEEP_DESCRIPTOR) {
        std::unique_lock<std::mutex> lock(ml.mMutexFeatures);
        drfe_cv::Mat d = drfe_cv::mat_u8(1, 32);
        std::memcpy(d.data, r.descriptor, 32);
        ml.mLDescriptor = d;
    }
    if (r.status & DRFE_UPKEEP_NORMAL) {
        std::unique_lock<std::mutex> lock(ml.mMutexPos);
        ml.mfMaxDistance = r.max_distance;
        ml.mfMinDistance = r.min_distance;
        for (int k = 0; k < 3; k++) ml.mNormalVector(k) = r.normal[k];
    }
}
}  // namespace drfe_detail_mu

/* pMP->ComputeDistinctiveDescriptors() (what = DRFE_UPKEEP_DESCRIPTOR), pMP->UpdateNormalAndDepth() (DRFE_UPKEEP_NORMAL) or
 * both, on the host: the results for the caller to assign */
template <class MapPointT>
inline MapPointUpkeep UpkeepMapPoint(MapPointT& mp, int what = DRFE_UPKEEP_DESCRIPTOR | DRFE_UPKEEP_NORMAL)
{
    const std::vector<MapPointT*> v(1, &mp);
    return drfe_detail_mu::run<std::false_type, MapPointUpkeep>(v, what, [](int w, const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, drfe_upkeep_out* o) {
        if (drfe_map_point_upkeep_host(w, k, it, o) != DRFE_OK) throw std::runtime_error("drfe_map_point_upkeep_host failed");
    })[0];
}

/* pML->ComputeDistinctiveDescriptors() / UpdateAverageDir() on the host, written into the line's public members */
template <class MapLineT>
inline MapLineUpkeep UpkeepMapLine(MapLineT& ml, int what = DRFE_UPKEEP_DESCRIPTOR | DRFE_UPKEEP_NORMAL)
{
    const std::vector<MapLineT*> v(1, &ml);
    const MapLineUpkeep r = drfe_detail_mu::run<std::true_type, MapLineUpkeep>(v, what, [](int w, const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, drfe_upkeep_out* o) {
        if (drfe_map_line_upkeep_host(w, k, it, o) != DRFE_OK) throw std::runtime_error("drfe_map_line_upkeep_host failed");
    })[0];
    drfe_detail_mu::apply_line(ml, r);
    return r;
}

/* The device batch for the loops over many points or lines (LocalMapping::ProcessNewKeyFrame, SearchInNeighbors, keyframe
 * creation, loop correction, map load).  Owns its own drfe_ctx: a context is not re-entrant, and LocalMapping runs on its own
 * thread, so an extractor's or matcher's context must not be borrowed.  Null entries are left unchanged (status 0). */
class MapUpkeep {
public:
    explicit MapUpkeep(int device = 0) : mCtx(Planar_SLAM::drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, device)) {}
    drfe_ctx* ctx() const { return mCtx.get(); }
    template <class MapPointT>
    std::vector<MapPointUpkeep> Points(const std::vector<MapPointT*>& v, int what = DRFE_UPKEEP_DESCRIPTOR | DRFE_UPKEEP_NORMAL)
    {
        drfe_ctx* c = mCtx.get();
        std::lock_guard<std::mutex> lock(mMutex);
        return drfe_detail_mu::run<std::false_type, MapPointUpkeep>(v, what, [c](int w, const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, drfe_upkeep_out* o) {
            Planar_SLAM::drfe_detail::check(drfe_map_point_upkeep_batch(c, w, k, it, o, nullptr), c, "drfe_map_point_upkeep_batch");
        });
    }
    /* the lines' members written as UpkeepMapLine does */
    template <class MapLineT>
    std::vector<MapLineUpkeep> Lines(const std::vector<MapLineT*>& v, int what = DRFE_UPKEEP_DESCRIPTOR | DRFE_UPKEEP_NORMAL)
    {
        drfe_ctx* c = mCtx.get();
        std::vector<MapLineUpkeep> r;
        {
            std::lock_guard<std::mutex> lock(mMutex);
            r = drfe_detail_mu::run<std::true_type, MapLineUpkeep>(v, what, [c](int w, const drfe_upkeep_keyframes* k, const drfe_upkeep_items* it, drfe_upkeep_out* o) {
                Planar_SLAM::drfe_detail::check(drfe_map_line_upkeep_batch(c, w, k, it, o, nullptr), c, "drfe_map_line_upkeep_batch");
            });
        }
        for (size_t i = 0; i < v.size(); i++)
            if (v[i]) drfe_detail_mu::apply_line(*v[i], r[i]);
        return r;
    }

private:
    Planar_SLAM::drfe_detail::CtxPtr mCtx;
    std::mutex mMutex;
};

/* LocalMapping::CreateNewMapPoints / CreateNewMapLines2's per-match body (src/LocalMapping.cc:383-538, 875-1026; RGB-D / stereo,
 * mbMonocular == false) over drfe_triangulate_points_host / drfe_triangulate_lines_host and the batch entries.  Reads
 *   KeyFrame: GetPose() (4x4 float Mat: Tcw), GetPoseInverse() (Twc, what UnprojectStereo / obtain3DLine read), GetCameraCenter(),
 *             fx, fy, cx, cy, invfx, invfy, mb, mbf, mfScaleFactor, mnScaleLevels, mvScaleFactors, mvLevelSigma2,
 *             points: mvKeysUn, mvKeys (.pt, .octave), mvuRight, mvDepth; lines: mvKeyLines, mvDepthLine, mvLines3D
 * and returns the accepted matches in vMatchedIndices order with the point (or the line's endpoints), so the reference loop body
 * shrinks to object creation.  The baseline test is the caller's loop's too: a skipped pair returns
 * nothing.  DESIGN.md section 15. */
struct TriangulatedPoint { size_t idx1, idx2; float x3D[3]; };
struct TriangulatedLine { size_t idx1, idx2; float sp[3], ep[3]; };
namespace drfe_detail_tri {
template <class M> inline void rows34(const M& m, float o[12])
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) o[r * 4 + c] = m.template ptr<float>(r)[c];
}
/* the flat inputs of one call: keyframes in first-use order, their features, the pairs */
struct Call {
    std::map<const void*, int32_t> index;
    std::vector<drfe_tri_keyframe> kf;
    std::vector<float> scale, sigma2, a, b, c, d;      /* points: un, raw, u_right, depth; lines: ends, depth */
    std::vector<double> l3;
    std::vector<int32_t> off{0}, octave, kf1, kf2, moff{0}, matches;
    int nLevels = 0;
    template <class KF> int32_t add(KF* p, bool line)
    {
        const auto r = index.emplace((const void*)p, (int32_t)kf.size());
        if (!r.second) return r.first->second;
        drfe_tri_keyframe k;
        rows34(p->GetPose(), k.Tcw);
        rows34(p->GetPoseInverse(), k.Twc);
        const auto O = p->GetCameraCenter();
        for (int q = 0; q < 3; q++) k.Ow[q] = O.template ptr<float>(q)[0];
        k.fx = p->fx; k.fy = p->fy; k.cx = p->cx; k.cy = p->cy; k.invfx = p->invfx; k.invfy = p->invfy;
        k.mb = p->mb; k.mbf = p->mbf; k.scale_factor = p->mfScaleFactor;
        kf.push_back(k);
        if (!nLevels) nLevels = p->mnScaleLevels;
        for (int q = 0; q < nLevels; q++) { scale.push_back(p->mvScaleFactors[q]); sigma2.push_back(p->mvLevelSigma2[q]); }
        if (line) {
            for (size_t i = 0; i < p->mvKeyLines.size(); i++) {
                const auto& kl = p->mvKeyLines[i];
                a.insert(a.end(), {kl.startPointX, kl.startPointY, kl.endPointX, kl.endPointY});
                octave.push_back(kl.octave);
                b.push_back(p->mvDepthLine[i]);
                for (int q = 0; q < 6; q++) l3.push_back(p->mvLines3D[i](q));
            }
        } else {
            for (size_t i = 0; i < p->mvKeysUn.size(); i++) {
                a.insert(a.end(), {p->mvKeysUn[i].pt.x, p->mvKeysUn[i].pt.y});
                b.insert(b.end(), {p->mvKeys[i].pt.x, p->mvKeys[i].pt.y});
                octave.push_back(p->mvKeysUn[i].octave);
                c.push_back(p->mvuRight[i]);
                d.push_back(p->mvDepth[i]);
            }
        }
        off.push_back((int32_t)octave.size());
        return r.first->second;
    }
    template <class KF, class Pairs> void pair(KF* p1, KF* p2, const Pairs& vMatchedIndices, bool line)
    {
        kf1.push_back(add(p1, line));
        kf2.push_back(add(p2, line));
        for (const auto& m : vMatchedIndices) { matches.push_back((int32_t)m.first); matches.push_back((int32_t)m.second); }
        moff.push_back((int32_t)(matches.size() / 2));
    }
    drfe_tri_keyframes keyframes() const
    {
        return drfe_tri_keyframes{(int32_t)kf.size(), nLevels, kf.data(), scale.data(), sigma2.data()};
    }
    drfe_tri_keypoints keypoints() const { return drfe_tri_keypoints{off.data(), a.data(), b.data(), octave.data(), c.data(), d.data()}; }
    drfe_tri_keylines keylines() const { return drfe_tri_keylines{off.data(), a.data(), octave.data(), b.data(), l3.data()}; }
    drfe_tri_pairs pairs() const { return drfe_tri_pairs{(int32_t)kf1.size(), 0, kf1.data(), kf2.data(), moff.data(), matches.data()}; }
};
inline void set_world(TriangulatedPoint& r, const float* x) { std::memcpy(r.x3D, x, 3 * sizeof(float)); }
inline void set_world(TriangulatedLine& r, const float* x) { std::memcpy(r.sp, x, 3 * sizeof(float)); std::memcpy(r.ep, x + 3, 3 * sizeof(float)); }
/* runs fn(keyframes, features, pairs, out) and returns the accepted matches of each pair in order */
template <class R, bool Line, class Fn> inline std::vector<std::vector<R>> run(const Call& cl, Fn fn)
{
    const size_t M = cl.matches.size() / 2;
    std::vector<uint8_t> st(M);
    std::vector<float> x((Line ? 6 : 3) * M + 1);
    drfe_tri_out o{st.data(), nullptr, x.data(), nullptr, nullptr};
    const drfe_tri_keyframes k = cl.keyframes();
    const drfe_tri_pairs p = cl.pairs();
    fn(&k, &p, &o);
    std::vector<std::vector<R>> out(cl.kf1.size());
    for (size_t q = 0; q < cl.kf1.size(); q++)
        for (int32_t m = cl.moff[q]; m < cl.moff[q + 1]; m++) {
            if ((st[m] & 0x7F) != DRFE_TRI_ACCEPTED) continue;
            R r;
            r.idx1 = (size_t)cl.matches[2 * (size_t)m];
            r.idx2 = (size_t)cl.matches[2 * (size_t)m + 1];
            set_world(r, &x[(Line ? 6 : 3) * (size_t)m]);
            out[q].push_back(r);
        }
    return out;
}
}  // namespace drfe_detail_tri

/* the accepted (idx1, idx2, x3D) of CreateNewMapPoints for one pair (pKF1 = mpCurrentKeyFrame, pKF2 = the neighbour), on the host */
template <class KF, class Pairs>
inline std::vector<TriangulatedPoint> TriangulateNewMapPoints(KF* pKF1, KF* pKF2, const Pairs& vMatchedIndices)
{
    drfe_detail_tri::Call cl;
    cl.pair(pKF1, pKF2, vMatchedIndices, false);
    return drfe_detail_tri::run<TriangulatedPoint, false>(cl, [&cl](const drfe_tri_keyframes* k, const drfe_tri_pairs* p, drfe_tri_out* o) {
        const drfe_tri_keypoints f = cl.keypoints();
        if (drfe_triangulate_points_host(0, k, &f, p, o) != DRFE_OK) throw std::runtime_error("drfe_triangulate_points_host failed");
    })[0];
}

/* the accepted (idx1, idx2, sp, ep) of CreateNewMapLines2 for one pair, on the host */
template <class KF, class Pairs>
inline std::vector<TriangulatedLine> TriangulateNewMapLines(KF* pKF1, KF* pKF2, const Pairs& vMatchedIndices)
{
    drfe_detail_tri::Call cl;
    cl.pair(pKF1, pKF2, vMatchedIndices, true);
    return drfe_detail_tri::run<TriangulatedLine, true>(cl, [&cl](const drfe_tri_keyframes* k, const drfe_tri_pairs* p, drfe_tri_out* o) {
        const drfe_tri_keylines f = cl.keylines();
        if (drfe_triangulate_lines_host(0, k, &f, p, o) != DRFE_OK) throw std::runtime_error("drfe_triangulate_lines_host failed");
    })[0];
}

/* The device batch: many independent pairs in one call (other keyframes, other sequences; not the neighbours of one keyframe
 * in turn, whose matching depends on the points made for the previous neighbour).  Owns its own drfe_ctx, as MapUpkeep. */
class Triangulation {
public:
    explicit Triangulation(int device = 0) : mCtx(Planar_SLAM::drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, device)) {}
    drfe_ctx* ctx() const { return mCtx.get(); }
    template <class KF, class Pairs>
    std::vector<std::vector<TriangulatedPoint>> Points(const std::vector<KF*>& kf1, const std::vector<KF*>& kf2, const std::vector<Pairs>& matches)
    {
        drfe_detail_tri::Call cl;
        for (size_t q = 0; q < kf1.size(); q++) cl.pair(kf1[q], kf2[q], matches[q], false);
        drfe_ctx* c = mCtx.get();
        std::lock_guard<std::mutex> lock(mMutex);
        return drfe_detail_tri::run<TriangulatedPoint, false>(cl, [&cl, c](const drfe_tri_keyframes* k, const drfe_tri_pairs* p, drfe_tri_out* o) {
            const drfe_tri_keypoints f = cl.keypoints();
            Planar_SLAM::drfe_detail::check(drfe_triangulate_points_batch(c, 0, k, &f, p, o, nullptr), c, "drfe_triangulate_points_batch");
        });
    }
    template <class KF, class Pairs>
    std::vector<std::vector<TriangulatedLine>> Lines(const std::vector<KF*>& kf1, const std::vector<KF*>& kf2, const std::vector<Pairs>& matches)
    {
        drfe_detail_tri::Call cl;
        for (size_t q = 0; q < kf1.size(); q++) cl.pair(kf1[q], kf2[q], matches[q], true);
        drfe_ctx* c = mCtx.get();
        std::lock_guard<std::mutex> lock(mMutex);
        return drfe_detail_tri::run<TriangulatedLine, true>(cl, [&cl, c](const drfe_tri_keyframes* k, const drfe_tri_pairs* p, drfe_tri_out* o) {
            const drfe_tri_keylines f = cl.keylines();
            Planar_SLAM::drfe_detail::check(drfe_triangulate_lines_batch(c, 0, k, &f, p, o, nullptr), c, "drfe_triangulate_lines_batch");
        });
    }

private:
    Planar_SLAM::drfe_detail::CtxPtr mCtx;
    std::mutex mMutex;
};

}  // namespace drfe

/* ---------------------------------------------------------------------------------------------------------------------------
 * Sim3Solver (include/Sim3Solver.h:35-130, src/Sim3Solver.cc) over drfe_sim3_ransac_host / drfe_sim3_ransac_batch: the first
 * iterate() or find() fills the solver's whole hypothesis table, every call after that walks it with the reference's cursor,
 * bNoMore and vbInliers[mvnIndices1[i]] semantics.  drfe::Sim3Batch fills the tables of many solvers with one device call.
 * The reference draws from the process-wide rand(); a solver here owns its stream (SetSeed, default 0).  DESIGN.md section 16. */
namespace drfe {
class Sim3Batch;
namespace drfe_detail_sim3 {
inline drfe_cv::Mat mat32(int rows, int cols, const float* v)
{
#ifdef DRFE_WITH_OPENCV
    drfe_cv::Mat m(rows, cols, CV_32F);
#else
    drfe_cv::Mat m(rows, cols, 4);
#endif
    for (int r = 0; r < rows; r++) std::memcpy(m.template ptr<float>(r), v + (size_t)r * cols, (size_t)cols * sizeof(float));
    return m;
}
/* one solver's inputs and, once filled, its table */
struct Problem {
    float Tcw1[12], Tcw2[12], K1[4], K2[4];
    uint8_t fixScale = 1;
    double probability = 0.99;
    int32_t minInliers = 6, maxIterations = 300;
    uint32_t seed = 0;
    std::vector<float> Xw1, Xw2, sig1, sig2;
    bool filled = false;
    int32_t iterations = 0, hypotheses = 0, words = 0;
    std::vector<int32_t> sample, inliers, best;
    std::vector<float> R12, t12, s12, T12;
    std::vector<uint8_t> returns;
    std::vector<uint64_t> mask;
    int n() const { return (int)sig1.size(); }
};
/* fills the tables of `ps` through fn(const drfe_sim3_problems*, drfe_sim3_out*) */
template <class Fn> inline void fill(const std::vector<Problem*>& ps, Fn fn)
{
    const size_t n = ps.size();
    std::vector<float> Tcw1, Tcw2, K1, K2, Xw1, Xw2, sig1, sig2;
    std::vector<uint8_t> fix;
    std::vector<double> prob;
    std::vector<int32_t> minI, maxI, off{0};
    std::vector<uint32_t> seed;
    std::vector<size_t> row0, mask0;
    size_t rows = 0, words = 0;
    for (Problem* p : ps) {
        Tcw1.insert(Tcw1.end(), p->Tcw1, p->Tcw1 + 12); Tcw2.insert(Tcw2.end(), p->Tcw2, p->Tcw2 + 12);
        K1.insert(K1.end(), p->K1, p->K1 + 4); K2.insert(K2.end(), p->K2, p->K2 + 4);
        fix.push_back(p->fixScale); prob.push_back(p->probability); minI.push_back(p->minInliers); maxI.push_back(p->maxIterations);
        seed.push_back(p->seed);
        Xw1.insert(Xw1.end(), p->Xw1.begin(), p->Xw1.end()); Xw2.insert(Xw2.end(), p->Xw2.begin(), p->Xw2.end());
        sig1.insert(sig1.end(), p->sig1.begin(), p->sig1.end()); sig2.insert(sig2.end(), p->sig2.begin(), p->sig2.end());
        off.push_back((int32_t)sig1.size());
        const size_t cap = (size_t)(p->maxIterations > 1 ? p->maxIterations : 1);
        p->words = (p->n() + 63) / 64;
        row0.push_back(rows); mask0.push_back(words);
        rows += cap; words += cap * (size_t)p->words;
    }
    const drfe_sim3_problems in{(int32_t)n, 0, Tcw1.data(), Tcw2.data(), K1.data(), K2.data(), fix.data(), prob.data(), minI.data(),
                                maxI.data(), seed.data(), off.data(), Xw1.data(), Xw2.data(), sig1.data(), sig2.data()};
    std::vector<int32_t> its(n + 1), hyp(n + 1), sample(3 * rows + 1), inl(rows + 1), best(rows + 1);
    std::vector<float> R(9 * rows + 1), t(3 * rows + 1), s(rows + 1), T(12 * rows + 1);
    std::vector<uint8_t> ret(rows + 1);
    std::vector<uint64_t> mask(words + 1);
    drfe_sim3_out out{its.data(), hyp.data(), sample.data(), R.data(), t.data(), s.data(), T.data(), inl.data(), ret.data(), best.data(),
                      mask.data()};
    fn(&in, &out);
    for (size_t q = 0; q < n; q++) {
        Problem* p = ps[q];
        const size_t h = (size_t)hyp[q], a = row0[q];
        p->iterations = its[q];
        p->hypotheses = hyp[q];
        p->sample.assign(sample.begin() + 3 * a, sample.begin() + 3 * (a + h));
        p->R12.assign(R.begin() + 9 * a, R.begin() + 9 * (a + h));
        p->t12.assign(t.begin() + 3 * a, t.begin() + 3 * (a + h));
        p->s12.assign(s.begin() + a, s.begin() + a + h);
        p->T12.assign(T.begin() + 12 * a, T.begin() + 12 * (a + h));
        p->inliers.assign(inl.begin() + a, inl.begin() + a + h);
        p->best.assign(best.begin() + a, best.begin() + a + h);
        p->returns.assign(ret.begin() + a, ret.begin() + a + h);
        p->mask.assign(mask.begin() + mask0[q], mask.begin() + mask0[q] + h * (size_t)p->words);
        p->filled = true;
    }
}
inline void fill_host(const std::vector<Problem*>& ps)
{
    fill(ps, [](const drfe_sim3_problems* in, drfe_sim3_out* out) {
        if (drfe_sim3_ransac_host(in, out) != DRFE_OK) throw std::runtime_error("drfe_sim3_ransac_host failed");
    });
}
}  // namespace drfe_detail_sim3
}  // namespace drfe

namespace Planar_SLAM {

template <class KeyFrameT, class MapPointT>
class Sim3Solver {
public:
    /* :41-116.  The map-graph part (isBad, GetIndexInKeyFrame, mvnIndices1) runs here, the arithmetic in the entries. */
    Sim3Solver(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12, const bool bFixScale = true)
        : mN1((int)vpMatched12.size())
    {
        mP.fixScale = bFixScale ? 1 : 0;
        const std::vector<MapPointT*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        drfe::drfe_detail_tri::rows34(pKF1->GetPose(), mP.Tcw1);
        drfe::drfe_detail_tri::rows34(pKF2->GetPose(), mP.Tcw2);
        const float k1[4] = {pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy}, k2[4] = {pKF2->fx, pKF2->fy, pKF2->cx, pKF2->cy};
        std::memcpy(mP.K1, k1, sizeof(k1));
        std::memcpy(mP.K2, k2, sizeof(k2));
        for (int i1 = 0; i1 < mN1; i1++) {
            if (!vpMatched12[i1]) continue;
            MapPointT* pMP1 = vpKeyFrameMP1[i1];
            MapPointT* pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            mP.sig1.push_back(pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave]);
            mP.sig2.push_back(pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave]);
            const auto X1 = pMP1->GetWorldPos();
            const auto X2 = pMP2->GetWorldPos();
            for (int q = 0; q < 3; q++) {
                mP.Xw1.push_back(X1.template ptr<float>(q)[0]);
                mP.Xw2.push_back(X2.template ptr<float>(q)[0]);
            }
            mvnIndices1.push_back((size_t)i1);
        }
        SetRansacParameters();
    }
    /* the deviation: the stream this solver draws from (the reference shares the process's rand()) */
    void SetSeed(uint32_t seed) { mP.seed = seed; mP.filled = false; mCursor = 0; mBest = -1; }
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mP.probability = probability;
        mP.minInliers = minInliers;
        mP.maxIterations = maxIterations;
        mP.filled = false;
        mCursor = 0;                    /* mnIterations = 0.  (The reference keeps mnBestInliers across a second call; here a call after iterate() starts a fresh table.) */
    }
    drfe_cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers)
    {
        bool bFlag;
        Fill();
        return iterate(mP.iterations, bFlag, vbInliers12, nInliers);
    }
    /* :144-211 as a walk over the table */
    drfe_cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        bNoMore = false;
        vbInliers = std::vector<bool>((size_t)mN1, false);
        nInliers = 0;
        if (mP.n() < mP.minInliers) { bNoMore = true; return drfe_cv::Mat(); }
        Fill();
        int nCurrentIterations = 0;
        while (mCursor < mP.hypotheses && nCurrentIterations < nIterations) {
            const int h = mCursor;
            nCurrentIterations++;
            mCursor++;
            mBest = mP.best[(size_t)h];
            if (mP.returns[(size_t)h]) {
                nInliers = mP.inliers[(size_t)h];
                const uint64_t* m = &mP.mask[(size_t)h * (size_t)mP.words];
                for (int i = 0; i < mP.n(); i++)
                    if ((m[i >> 6] >> (i & 63)) & 1) vbInliers[mvnIndices1[(size_t)i]] = true;
                return drfe::drfe_detail_sim3::mat32(4, 4, T44(h).data());
            }
        }
        if (mCursor >= mP.hypotheses) bNoMore = true;
        return drfe_cv::Mat();
    }
    drfe_cv::Mat GetEstimatedRotation() const { return mBest < 0 ? drfe_cv::Mat() : drfe::drfe_detail_sim3::mat32(3, 3, &mP.R12[9 * (size_t)mBest]); }
    drfe_cv::Mat GetEstimatedTranslation() const { return mBest < 0 ? drfe_cv::Mat() : drfe::drfe_detail_sim3::mat32(3, 1, &mP.t12[3 * (size_t)mBest]); }
    float GetEstimatedScale() const { return mBest < 0 ? 0.f : mP.s12[(size_t)mBest]; }
    /* beyond the reference: the compacted correspondences, and the table itself */
    const std::vector<size_t>& Indices1() const { return mvnIndices1; }
    const drfe::drfe_detail_sim3::Problem& Table() { Fill(); return mP; }

private:
    friend class drfe::Sim3Batch;
    void Fill()
    {
        if (mP.filled) return;
        drfe::drfe_detail_sim3::fill_host({&mP});
    }
    std::vector<float> T44(int h) const
    {
        std::vector<float> T(16, 0.f);
        std::memcpy(T.data(), &mP.T12[12 * (size_t)h], 12 * sizeof(float));
        T[15] = 1.f;
        return T;
    }
    drfe::drfe_detail_sim3::Problem mP;
    std::vector<size_t> mvnIndices1;
    int mN1, mCursor = 0, mBest = -1;
};

}  // namespace Planar_SLAM

namespace drfe {

/* The device batch: the tables of all solvers of one ComputeSim3 call (or of many) filled by one drfe_sim3_ransac_batch call; the
 * solvers' iterate() / find() then only walk.  Owns its own drfe_ctx, as Triangulation. */
class Sim3Batch {
public:
    explicit Sim3Batch(int device = 0) : mCtx(Planar_SLAM::drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, device)) {}
    drfe_ctx* ctx() const { return mCtx.get(); }
    template <class SolverT> void Fill(const std::vector<SolverT*>& solvers)
    {
        std::vector<drfe_detail_sim3::Problem*> ps;
        for (SolverT* s : solvers)
            if (s) ps.push_back(&s->mP);
        drfe_ctx* c = mCtx.get();
        std::lock_guard<std::mutex> lock(mMutex);
        drfe_detail_sim3::fill(ps, [c](const drfe_sim3_problems* in, drfe_sim3_out* out) {
            Planar_SLAM::drfe_detail::check(drfe_sim3_ransac_batch(c, in, out, nullptr), c, "drfe_sim3_ransac_batch");
        });
    }

private:
    Planar_SLAM::drfe_detail::CtxPtr mCtx;
    std::mutex mMutex;
};

}  // namespace drfe

/* ---------------------------------------------------------------------------------------------------------------------------
 * PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) over drfe_pnp_ransac_host / drfe_pnp_ransac_batch: the first iterate() or
 * find() fills the solver's whole table, every call after that walks it with the reference's cursor, its `||` loop condition,
 * bNoMore and vbInliers[mvKeyPointIndices[i]] semantics.  A table has iterations + tail rows (tail: SetTail, default 5, what
 * Relocalization's iterate(5, ..) can read past mRansacMaxIts in one call); a walk that runs off them refills the table on the
 * host with a larger tail - the seed fixes every row, so the rows already walked do not change.  drfe::PnPBatch fills the tables
 * of many solvers with one call.  The reference draws from the process-wide rand(); a solver here owns its stream (SetSeed,
 * default 0).  DESIGN.md section 17. */
namespace drfe {
class PnPBatch;
namespace drfe_detail_pnp {
/* one solver's inputs and, once filled, its table */
struct Problem {
    float K[4];
    double probability = 0.99;
    int32_t minInliers = 8, maxIterations = 300, tail = 5;
    float epsilon = 0.4f, th2 = 5.991f;
    uint32_t seed = 0;
    std::vector<float> p2d, Xw, sig;
    bool filled = false;
    int32_t iterations = 0, minInliersAdj = 0, hypotheses = 0, refines = 0, words = 0;
    std::vector<int32_t> sample, inliers, best, refInliers;
    std::vector<double> R, t, refR, refT;
    std::vector<uint8_t> returns;
    std::vector<uint64_t> mask, refMask;
    int n() const { return (int)sig.size(); }
};
/* fills the tables of `ps` through fn(const drfe_pnp_problems*, drfe_pnp_out*) */
template <class Fn> inline void fill(const std::vector<Problem*>& ps, Fn fn)
{
    const size_t n = ps.size();
    std::vector<float> K, eps, th2, p2d, Xw, sig;
    std::vector<double> prob;
    std::vector<int32_t> minI, maxI, tail, off{0};
    std::vector<uint32_t> seed;
    std::vector<size_t> row0, mask0;
    size_t rows = 0, words = 0;
    for (Problem* p : ps) {
        K.insert(K.end(), p->K, p->K + 4);
        prob.push_back(p->probability); minI.push_back(p->minInliers); maxI.push_back(p->maxIterations); tail.push_back(p->tail);
        eps.push_back(p->epsilon); th2.push_back(p->th2); seed.push_back(p->seed);
        p2d.insert(p2d.end(), p->p2d.begin(), p->p2d.end()); Xw.insert(Xw.end(), p->Xw.begin(), p->Xw.end());
        sig.insert(sig.end(), p->sig.begin(), p->sig.end());
        off.push_back((int32_t)sig.size());
        const size_t cap = (size_t)(p->maxIterations > 1 ? p->maxIterations : 1) + (size_t)(p->tail > 0 ? p->tail : 0);
        p->words = (p->n() + 63) / 64;
        row0.push_back(rows); mask0.push_back(words);
        rows += cap; words += cap * (size_t)p->words;
    }
    const drfe_pnp_problems in{(int32_t)n, 0, K.data(), prob.data(), minI.data(), maxI.data(), eps.data(), th2.data(), tail.data(),
                               seed.data(), off.data(), p2d.data(), Xw.data(), sig.data()};
    std::vector<int32_t> its(n + 1), mins(n + 1), hyp(n + 1), refs(n + 1), sample(4 * rows + 1), inl(rows + 1), best(rows + 1),
        rinl(rows + 1);
    std::vector<double> R(9 * rows + 1), t(3 * rows + 1), rR(9 * rows + 1), rt(3 * rows + 1);
    std::vector<uint8_t> ret(rows + 1);
    std::vector<uint64_t> mask(words + 1), rmask(words + 1);
    drfe_pnp_out out{its.data(), mins.data(), hyp.data(), refs.data(), sample.data(), R.data(), t.data(), inl.data(), mask.data(),
                     best.data(), ret.data(), rR.data(), rt.data(), rinl.data(), rmask.data()};
    fn(&in, &out);
    for (size_t q = 0; q < n; q++) {
        Problem* p = ps[q];
        const size_t h = (size_t)hyp[q], a = row0[q], mw = h * (size_t)p->words;
        p->iterations = its[q]; p->minInliersAdj = mins[q]; p->hypotheses = hyp[q]; p->refines = refs[q];
        p->sample.assign(sample.begin() + 4 * a, sample.begin() + 4 * (a + h));
        p->R.assign(R.begin() + 9 * a, R.begin() + 9 * (a + h));
        p->t.assign(t.begin() + 3 * a, t.begin() + 3 * (a + h));
        p->refR.assign(rR.begin() + 9 * a, rR.begin() + 9 * (a + h));
        p->refT.assign(rt.begin() + 3 * a, rt.begin() + 3 * (a + h));
        p->inliers.assign(inl.begin() + a, inl.begin() + a + h);
        p->refInliers.assign(rinl.begin() + a, rinl.begin() + a + h);
        p->best.assign(best.begin() + a, best.begin() + a + h);
        p->returns.assign(ret.begin() + a, ret.begin() + a + h);
        p->mask.assign(mask.begin() + mask0[q], mask.begin() + mask0[q] + mw);
        p->refMask.assign(rmask.begin() + mask0[q], rmask.begin() + mask0[q] + mw);
        p->filled = true;
    }
}
inline void fill_host(const std::vector<Problem*>& ps)
{
    fill(ps, [](const drfe_pnp_problems* in, drfe_pnp_out* out) {
        if (drfe_pnp_ransac_host(in, out) != DRFE_OK) throw std::runtime_error("drfe_pnp_ransac_host failed");
    });
}
}  // namespace drfe_detail_pnp
}  // namespace drfe

namespace Planar_SLAM {

template <class FrameT, class MapPointT>
class PnPsolver {
public:
    /* :67-110.  The map-graph part (isBad, mvKeyPointIndices) runs here, the arithmetic in the entries. */
    PnPsolver(const FrameT& F, const std::vector<MapPointT*>& vpMapPointMatches) : mNMatches(vpMapPointMatches.size())
    {
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            MapPointT* pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;
            const auto& kp = F.mvKeysUn[i];
            mP.p2d.push_back(kp.pt.x);
            mP.p2d.push_back(kp.pt.y);
            mP.sig.push_back(F.mvLevelSigma2[kp.octave]);
            const auto Pos = pMP->GetWorldPos();
            for (int q = 0; q < 3; q++) mP.Xw.push_back(Pos.template ptr<float>(q)[0]);
            mvKeyPointIndices.push_back(i);
        }
        const float k[4] = {F.fx, F.fy, F.cx, F.cy};
        std::memcpy(mP.K, k, sizeof(k));
        SetRansacParameters();
    }
    /* the deviation: the stream this solver draws from (the reference shares the process's rand()) */
    void SetSeed(uint32_t seed) { mP.seed = seed; Reset(); }
    /* rows a table holds past mRansacMaxIts: what one iterate(nIterations, ..) of the caller can read there */
    void SetTail(int tail) { mP.tail = tail; Reset(); }
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                             float th2 = 5.991)
    {
        if (minSet != 4) throw std::invalid_argument("PnPsolver: minSet is 4");     /* the reference's only caller and its default */
        mP.probability = probability;
        mP.minInliers = minInliers;
        mP.maxIterations = maxIterations;
        mP.epsilon = epsilon;
        mP.th2 = th2;
        Reset();
    }
    drfe_cv::Mat find(std::vector<bool>& vbInliers, int& nInliers)
    {
        bool bFlag;
        Fill();
        return iterate(mP.iterations, bFlag, vbInliers, nInliers);
    }
    /* :165-258 as a walk over the table */
    drfe_cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        Fill();
        if (mP.n() < mP.minInliersAdj) { bNoMore = true; return drfe_cv::Mat(); }
        int nCurrentIterations = 0;
        while (mCursor < mP.iterations || nCurrentIterations < nIterations) {
            if (mCursor >= mP.hypotheses) Refill(nIterations - nCurrentIterations);
            const size_t h = (size_t)mCursor;
            nCurrentIterations++;
            mCursor++;
            if (mP.returns[h]) {
                const size_t b = (size_t)mP.best[h];
                nInliers = mP.refInliers[b];
                Inliers(&mP.refMask[b * (size_t)mP.words], vbInliers);
                return T44(&mP.refR[9 * b], &mP.refT[3 * b]);
            }
        }
        if (mCursor >= mP.iterations) {
            bNoMore = true;
            const int b = mCursor > 0 ? mP.best[(size_t)mCursor - 1] : -1;
            if (b >= 0) {
                nInliers = mP.inliers[(size_t)b];
                Inliers(&mP.mask[(size_t)b * (size_t)mP.words], vbInliers);
                return T44(&mP.R[9 * (size_t)b], &mP.t[3 * (size_t)b]);
            }
        }
        return drfe_cv::Mat();
    }
    /* beyond the reference: the compacted correspondences, the table itself, and how many times a walk ran off it */
    const std::vector<size_t>& KeyPointIndices() const { return mvKeyPointIndices; }
    const drfe::drfe_detail_pnp::Problem& Table() { Fill(); return mP; }
    int Refills() const { return mRefills; }

private:
    friend class drfe::PnPBatch;
    void Reset() { mP.filled = false; mCursor = 0; }
    void Fill()
    {
        if (mP.filled) return;
        drfe::drfe_detail_pnp::fill_host({&mP});
    }
    void Refill(int need)
    {
        if (mP.tail >= DRFE_PNP_MAX_TAIL) throw std::runtime_error("PnPsolver: iterate() past DRFE_PNP_MAX_TAIL rows after mRansacMaxIts");
        int tail = mP.tail * 2 > mP.tail + need ? mP.tail * 2 : mP.tail + need;
        mP.tail = tail < DRFE_PNP_MAX_TAIL ? tail : DRFE_PNP_MAX_TAIL;
        mP.filled = false;
        mRefills++;
        Fill();
    }
    void Inliers(const uint64_t* m, std::vector<bool>& vbInliers) const
    {
        vbInliers = std::vector<bool>(mNMatches, false);
        for (int i = 0; i < mP.n(); i++)
            if ((m[i >> 6] >> (i & 63)) & 1) vbInliers[mvKeyPointIndices[(size_t)i]] = true;
    }
    /* Rcw.convertTo(CV_32F), tcw.convertTo(CV_32F) into cv::Mat::eye(4, 4, CV_32F) */
    static drfe_cv::Mat T44(const double* R, const double* t)
    {
        float T[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
        for (int r = 0; r < 3; r++) {
            for (int q = 0; q < 3; q++) T[r * 4 + q] = (float)R[r * 3 + q];
            T[r * 4 + 3] = (float)t[r];
        }
        return drfe::drfe_detail_sim3::mat32(4, 4, T);
    }
    drfe::drfe_detail_pnp::Problem mP;
    std::vector<size_t> mvKeyPointIndices;
    size_t mNMatches;
    int mCursor = 0, mRefills = 0;
};

/* ---------------------------------------------------------------------------------------------------------------------------
 * Initializer (include/Initializer.h, src/Initializer.cc) over drfe_init_ransac_host / drfe_init_ransac_batch: the reference's
 * constructor (ReferenceFrame, sigma, iterations) and its point-only Initialize(CurrentFrame, vMatches12, R21, t21, vP3D,
 * vbTriangulated).  One Initialize is one solver of one call; it goes to the device entry when a call of one solver reaches
 * DRFE_INIT_DEVICE_FROM (not measured yet, so the constant is INT32_MAX), to the host entry otherwise (same
 * bits); UseDevice() overrides the constant.  The device entry runs on the thread's bound context (ORBmatcher::BindThread) or on one the object
 * makes on first use.  The reference seeds rand() with srand(0) once per process; here every Initialize draws from srand(seed)
 * (SetSeed, default 0: a process's first Initialize).  FrameT: mK (CV_32F 3x3, continuous), mvKeysUn.  DESIGN.md section 19. */
template <class FrameT>
class Initializer {
public:
    Initializer(const FrameT& ReferenceFrame, float sigma = 1.0, int iterations = 200)
        : mSigma(sigma), mMaxIterations(iterations), mUseDevice(1 >= DRFE_INIT_DEVICE_FROM)
    {
        std::memcpy(mK, reinterpret_cast<const float*>(ReferenceFrame.mK.data), sizeof(mK));
        for (const auto& k : ReferenceFrame.mvKeysUn) { mKeys1.push_back(k.pt.x); mKeys1.push_back(k.pt.y); }
    }
    void SetSeed(uint32_t seed) { mSeed = seed; }
    void UseDevice(bool on) { mUseDevice = on; }
    /* what the last Initialize left besides its results: DRFE_INIT_BRANCH_*, DRFE_INIT_* flags, RH */
    int Branch() const { return mBranch; }
    int Flags() const { return mFlags; }
    float RH() const { return mRH; }

    template <class Point3T>
    bool Initialize(const FrameT& CurrentFrame, const std::vector<int>& vMatches12, drfe_cv::Mat& R21, drfe_cv::Mat& t21,
                    std::vector<Point3T>& vP3D, std::vector<bool>& vbTriangulated)
    {
        const int32_t n1 = (int32_t)(mKeys1.size() / 2), n2 = (int32_t)CurrentFrame.mvKeysUn.size();
        if ((int32_t)vMatches12.size() > n1) throw std::invalid_argument("Initializer::Initialize: more matches than reference keys");
        std::vector<float> keys2;
        for (const auto& k : CurrentFrame.mvKeysUn) { keys2.push_back(k.pt.x); keys2.push_back(k.pt.y); }
        std::vector<int32_t> m12((size_t)n1, -1);
        for (size_t i = 0; i < vMatches12.size(); i++) m12[i] = vMatches12[i] >= 0 ? vMatches12[i] : -1;
        const int32_t it = mMaxIterations > 0 ? mMaxIterations : 0, off1[2] = {0, n1}, off2[2] = {0, n2};
        int N = 0;
        for (int32_t m : m12) N += m >= 0;
        const size_t rows = (size_t)it, words = rows * (size_t)((N + 63) / 64), k1 = (size_t)n1;
        drfe_init_problems P = {1, 0, mK, &mSigma, &it, &mSeed, off1, off2, mKeys1.data(), keys2.data(), m12.data()};
        int32_t sc[7] = {0};
        float SH, SF, R[9], t[3], mcos[8], mpar[8], mR[72], mt[24];
        int32_t mgood[8], mstatus[8];
        std::vector<float> p3d(3 * k1 + 1), H(9 * rows + 1), F(9 * rows + 1), sh(rows + 1), sf(rows + 1), mp3d(24 * k1 + 1);
        std::vector<uint8_t> tri(k1 + 1), mvb(8 * k1 + 1);
        std::vector<int32_t> sample(8 * rows + 1), bh(rows + 1), bf(rows + 1);
        std::vector<uint64_t> mh(words + 1), mf(words + 1);
        drfe_init_out O = {&sc[0], &sc[1], &sc[2], &SH, &SF, &mRH, &sc[3], &sc[4], &sc[5], &sc[6], R, t, p3d.data(), tri.data(),
                           sample.data(), H.data(), F.data(), sh.data(), sf.data(), bh.data(), bf.data(), mh.data(), mf.data(),
                           mR, mt, mgood, mcos, mpar, mstatus, mvb.data(), mp3d.data()};
        if (mUseDevice) {
            drfe_ctx* c = drfe_detail::thread_ctx();
            if (!c) {
                if (!mCtx) mCtx = drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, 0);
                c = mCtx.get();
            }
            drfe_detail::check(drfe_init_ransac_batch(c, &P, &O, nullptr), c, "drfe_init_ransac_batch");
        } else if (drfe_init_ransac_host(&P, &O) != DRFE_OK)
            throw std::runtime_error("drfe_init_ransac_host: invalid argument");
        mBranch = sc[3];
        mFlags = sc[6];
        if (!sc[5]) {
            /* ReconstructF empties R21 and t21 before it decides; ReconstructH leaves them */
            if (mBranch == DRFE_INIT_BRANCH_F) { R21 = drfe_cv::Mat(); t21 = drfe_cv::Mat(); }
            return false;
        }
        R21 = drfe::drfe_detail_sim3::mat32(3, 3, R);
        t21 = drfe::drfe_detail_sim3::mat32(3, 1, t);
        vP3D.resize(k1);
        vbTriangulated.assign(k1, false);
        for (size_t i = 0; i < k1; i++) {
            vP3D[i].x = p3d[3 * i]; vP3D[i].y = p3d[3 * i + 1]; vP3D[i].z = p3d[3 * i + 2];
            vbTriangulated[i] = tri[i] != 0;
        }
        return true;
    }

private:
    float mK[9], mSigma;
    int mMaxIterations;
    uint32_t mSeed = 0;
    bool mUseDevice;
    int mBranch = 0, mFlags = 0;
    float mRH = 0;
    std::vector<float> mKeys1;
    drfe_detail::CtxPtr mCtx;
};

}  // namespace Planar_SLAM

namespace drfe {

/* The batch: the tables of all solvers of one Relocalization call (or of many) filled by one call; the solvers' iterate() /
 * find() then only walk.  A call of fewer than `deviceFrom` solvers goes to the host entry (same bits): below the crossover
 * measured in DESIGN.md section 17 the device's fixed cost per call is larger than the host's whole work.  Owns its own
 * drfe_ctx, as Sim3Batch. */
class PnPBatch {
public:
    explicit PnPBatch(int device = 0, int deviceFrom = DRFE_PNP_DEVICE_FROM)
        : mCtx(Planar_SLAM::drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, device)), mDeviceFrom(deviceFrom) {}
    drfe_ctx* ctx() const { return mCtx.get(); }
    template <class SolverT> void Fill(const std::vector<SolverT*>& solvers)
    {
        std::vector<drfe_detail_pnp::Problem*> ps;
        for (SolverT* s : solvers)
            if (s) ps.push_back(&s->mP);
        if ((int)ps.size() < mDeviceFrom) { drfe_detail_pnp::fill_host(ps); return; }
        drfe_ctx* c = mCtx.get();
        std::lock_guard<std::mutex> lock(mMutex);
        drfe_detail_pnp::fill(ps, [c](const drfe_pnp_problems* in, drfe_pnp_out* out) {
            Planar_SLAM::drfe_detail::check(drfe_pnp_ransac_batch(c, in, out, nullptr), c, "drfe_pnp_ransac_batch");
        });
    }

private:
    Planar_SLAM::drfe_detail::CtxPtr mCtx;
    int mDeviceFrom;
    std::mutex mMutex;
};

/* Frame::isLineGood (src/Frame.cc:481-558) for the frames of a batch: mvDepthLine and mvLines3D of every frame from its
 * mvKeylinesUn and its CV_32F depth image, by one drfe_lines_is_good_batch call.  A call of fewer than
 * `deviceFrom` frames loops the host entry drfe_lines_is_good (same bits).  The frames share one camera and one image size (the
 * first frame's mK, cx, cy, invfx, invfy); kAsF64 = 0 is the reference as shipped, 1 the lifting as it was meant (include/drfe.h);
 * seeds[f] is frame f's srand() state, 1 without.  Returns the accepted lines.  Owns its own drfe_ctx, as Sim3Batch.
 * FrameT: mvKeylinesUn, mK (CV_32F 3x3, continuous), cx, cy, invfx, invfy, mvDepthLine (vector<float>), mvLines3D (vector of
 * Vector6d: operator()(int)). */
class Line3DBatch {
public:
    explicit Line3DBatch(int device = 0, int deviceFrom = DRFE_LINE3D_DEVICE_FROM, int kAsF64 = 0)
        : mCtx(Planar_SLAM::drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, device)), mDeviceFrom(deviceFrom), mKAsF64(kAsF64) {}
    drfe_ctx* ctx() const { return mCtx.get(); }
    template <class FrameT>
    int Fill(const std::vector<FrameT*>& frames, const std::vector<drfe_cv::Mat>& depth, const std::vector<uint32_t>* seeds = nullptr)
    {
        const size_t F = frames.size();
        if (!F) return 0;
        if (depth.size() != F || (seeds && seeds->size() != F)) throw std::invalid_argument("Line3DBatch::Fill: one depth image and one seed per frame");
        const int w = depth[0].cols, h = depth[0].rows;
        size_t cap = 1;
        for (const FrameT* f : frames) cap = std::max(cap, f->mvKeylinesUn.size());
        std::vector<drfe_keyline> kl(F * cap);
        std::vector<int32_t> n(F), good(F, 0);
        std::vector<float> depthLine(F * cap);
        std::vector<double> l3(F * cap * 6);
        for (size_t f = 0; f < F; f++) {
            if (depth[f].cols != w || depth[f].rows != h || depth[f].empty()) throw std::invalid_argument("Line3DBatch::Fill: depth images of one size");
            n[f] = (int32_t)frames[f]->mvKeylinesUn.size();
            for (int i = 0; i < n[f]; i++) kl[f * cap + i] = Planar_SLAM::drfe_detail::keyline_of(frames[f]->mvKeylinesUn[i]);
        }
        const FrameT& F0 = *frames[0];
        const float* K = reinterpret_cast<const float*>(F0.mK.data);
        if (F < (size_t)mDeviceFrom) {
            for (size_t f = 0; f < F; f++) {
                const int rc = drfe_lines_is_good(&kl[f * cap], n[f], depth[f].template ptr<float>(0), w, h, depth[f].step / sizeof(float), K,
                                                  mKAsF64, F0.cx, F0.cy, F0.invfx, F0.invfy, seeds ? (*seeds)[f] : 1u, &depthLine[f * cap],
                                                  &l3[f * cap * 6], nullptr, &good[f]);
                if (rc != DRFE_OK) throw std::runtime_error("drfe_lines_is_good: invalid argument");
            }
        } else {
            std::lock_guard<std::mutex> lock(mMutex);
            mDepth.resize(F * (size_t)w * h);          /* the images of a batch lie anywhere: packed here, uploaded by the call */
            for (size_t f = 0; f < F; f++)
                for (int r = 0; r < h; r++) std::memcpy(&mDepth[(f * h + r) * w], depth[f].template ptr<float>(r), (size_t)w * sizeof(float));
            drfe_line3d_frames in = {};
            in.nframes = (int32_t)F; in.cap = (int32_t)cap; in.lines = kl.data(); in.n_lines = n.data();
            in.depth = mDepth.data(); in.frame_stride = (size_t)w * h; in.stride = (size_t)w; in.w = w; in.h = h;
            in.depth_on_device = 0; in.k_as_f64 = mKAsF64;
            std::memcpy(in.K, K, sizeof(in.K));
            in.cx = F0.cx; in.cy = F0.cy; in.invfx = F0.invfx; in.invfy = F0.invfy;
            in.seeds = seeds ? seeds->data() : nullptr;
            drfe_line3d_out out = {depthLine.data(), l3.data(), nullptr, good.data()};
            Planar_SLAM::drfe_detail::check(drfe_lines_is_good_batch(mCtx.get(), &in, &out, nullptr), mCtx.get(), "drfe_lines_is_good_batch");
        }
        int total = 0;
        for (size_t f = 0; f < F; f++) {
            FrameT& fr = *frames[f];
            fr.mvDepthLine.resize((size_t)n[f]);
            fr.mvLines3D.resize((size_t)n[f]);
            for (int i = 0; i < n[f]; i++) {
                fr.mvDepthLine[i] = depthLine[f * cap + i];
                for (int q = 0; q < 6; q++) fr.mvLines3D[i](q) = l3[(f * cap + i) * 6 + q];
            }
            total += good[f];
        }
        return total;
    }

private:
    Planar_SLAM::drfe_detail::CtxPtr mCtx;
    int mDeviceFrom, mKAsF64;
    std::vector<float> mDepth;
    std::mutex mMutex;
};

}  // namespace drfe

namespace drfe {

/* Optimizer::PoseOptimization (src/Optimizer.cc:601-1338) for one frame or for the frames of a batch (Relocalization's candidates,
 * the frames of a batched tracker): Add() flattens what the reference reads of a frame, Run() optimises every added frame by one
 * drfe_pose_opt_batch call (or, below `deviceFrom` frames, by the host entry: same bits) and writes back what the reference
 * writes: SetPose(Tcw), mvbOutlier, mvbLineOutlier, mvbPlaneOutlier, mvbParPlaneOutlier, mvbVerPlaneOutlier (only the entries of
 * matched features, as the reference).  Result(i) is the i-th added frame's return value.  An object belongs to one thread.  The plane settings are the reference's
 * Config values (Plane.AngleInfo, DistanceInfo, ParallelInfo, VerticalInfo, Chi, VPChi).  DESIGN.md section 20.
 * FrameT: mTcw (4x4 float), fx fy cx cy mbf, N, mvKeysUn, mvuRight, mvInvLevelSigma2, mvpMapPoints, mvbOutlier, NL,
 * mvKeyLineFunctions (three doubles through operator()), mvpMapLines, mvbLineOutlier, mnPlaneNum, mvPlaneCoefficients,
 * mvpMapPlanes, mvpParallelPlanes, mvpVerticalPlanes, mvbPlaneOutlier, mvbParPlaneOutlier, mvbVerPlaneOutlier, SetPose(Mat).
 * MapPoint / MapPlane: GetWorldPos() (3x1 / 4x1 float); MapLine: mWorldPos (six doubles through operator()). */
struct PlaneSettings { double angleInfo = 0.5, distanceInfo = 50, parallelInfo = 0.1, verticalInfo = 0.1, chi = 100, vpChi = 50; };

/* TransOnly: the same batch over Optimizer::TranslationOptimization (src/Optimizer.cc:3211-3980, drfe_trans_opt_host / _batch,
 * DESIGN.md section 21), spelled drfe::TransOptBatch<FrameT>.  It reads and writes the same members; the map geometry goes in
 * world coordinates and the entry rotates it by mTcw's rotation; only the points count towards the three correspondences below
 * which the reference returns before SetPose; it switches entries at DRFE_TRANSOPT_DEVICE_FROM. */
template <class FrameT, bool TransOnly = false>
class PoseOptBatch {
public:
    explicit PoseOptBatch(const PlaneSettings& settings = PlaneSettings(), int device = 0,
                          int deviceFrom = TransOnly ? (int)DRFE_TRANSOPT_DEVICE_FROM : (int)DRFE_POSEOPT_DEVICE_FROM)
        : mSettings(settings), mDevice(device), mDeviceFrom(deviceFrom) { Clear(); }
    /* true / false: the device / the host entry whatever the number of frames */
    void UseDevice(bool on) { mDeviceFrom = on ? 0 : 2147483647; }
    void SetSettings(const PlaneSettings& s) { mSettings = s; }
    void Clear()
    {
        mFrames.clear(); mStruct.clear(); mTcw.clear(); mK.clear(); mBf.clear();
        mObs.clear(); mUr.clear(); mInvSigma2.clear(); mXw.clear(); mPointIdx.clear();
        mLineFn.clear(); mLineEnds.clear(); mLineIdx.clear();
        mPlaneMeas.clear(); mPlaneWorld.clear(); mPlaneMask.clear();
        mPointOff.assign(1, 0); mLineOff.assign(1, 0); mPlaneOff.assign(1, 0);
        mReturns.clear();
    }
    size_t size() const { return mFrames.size(); }
    void Add(FrameT* pFrame, bool bStruct)
    {
        using Planar_SLAM::drfe_detail::mat_f;
        FrameT& F = *pFrame;
        mFrames.push_back(pFrame);
        mStruct.push_back(bStruct ? 1 : 0);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) mTcw.push_back(mat_f(F.mTcw, r, c));
        mK.push_back(F.fx); mK.push_back(F.fy); mK.push_back(F.cx); mK.push_back(F.cy);
        mBf.push_back(F.mbf);
        for (int i = 0; i < F.N; i++) {
            auto* pMP = F.mvpMapPoints[(size_t)i];
            if (!pMP) continue;
            const auto& kp = F.mvKeysUn[(size_t)i];
            mObs.push_back(kp.pt.x); mObs.push_back(kp.pt.y);
            mUr.push_back(F.mvuRight[(size_t)i]);
            mInvSigma2.push_back(F.mvInvLevelSigma2[(size_t)kp.octave]);
            const auto Xw = pMP->GetWorldPos();
            for (int k = 0; k < 3; k++) mXw.push_back(mat_f(Xw, k));
            mPointIdx.push_back(i);
        }
        mPointOff.push_back((int32_t)mPointIdx.size());
        for (int i = 0; i < F.NL; i++) {
            auto* pML = F.mvpMapLines[(size_t)i];
            if (!pML) continue;
            for (int k = 0; k < 3; k++) mLineFn.push_back(F.mvKeyLineFunctions[(size_t)i](k));
            for (int k = 0; k < 6; k++) mLineEnds.push_back(pML->mWorldPos(k));
            mLineIdx.push_back(i);
        }
        mLineOff.push_back((int32_t)mLineIdx.size());
        for (int i = 0; i < F.mnPlaneNum; i++) {           /* every detected plane is a slot; an empty one has mask 0 */
            uint8_t mask = 0;
            float world[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            auto put = [&](decltype(F.mvpMapPlanes[0]) pMP, int which) {
                if (!pMP) return;
                const auto W = pMP->GetWorldPos();
                for (int k = 0; k < 4; k++) world[4 * which + k] = mat_f(W, k);
                mask |= (uint8_t)(1 << which);
            };
            put(F.mvpMapPlanes[(size_t)i], 0);
            put(F.mvpParallelPlanes[(size_t)i], 1);
            put(F.mvpVerticalPlanes[(size_t)i], 2);
            for (int k = 0; k < 4; k++) mPlaneMeas.push_back(mat_f(F.mvPlaneCoefficients[(size_t)i], k));
            mPlaneWorld.insert(mPlaneWorld.end(), world, world + 12);
            mPlaneMask.push_back(mask);
        }
        mPlaneOff.push_back((int32_t)mPlaneMask.size());
    }
    /* optimises every added frame and writes the frames back; the batch is empty afterwards but for Result() */
    void Run()
    {
        const size_t n = mFrames.size();
        std::vector<float> Tcw(16 * n);
        std::vector<int32_t> rounds(n), its(n), trials(n);
        std::vector<uint8_t> po(mPointIdx.size() + 1), lo(mLineIdx.size() + 1), pl(mPlaneMask.size() + 1), pp(mPlaneMask.size() + 1),
            pv(mPlaneMask.size() + 1);
        mReturns.assign(n, 0);
        drfe_pose_opt_problems in = {};
        in.n = (int32_t)n;
        in.Tcw = mTcw.data(); in.K = mK.data(); in.bf = mBf.data(); in.b_struct = mStruct.data();
        in.point_offsets = mPointOff.data(); in.obs = mObs.data(); in.u_right = mUr.data(); in.inv_sigma2 = mInvSigma2.data();
        in.Xw = mXw.data();
        in.line_offsets = mLineOff.data(); in.line_fn = mLineFn.data(); in.line_ends = mLineEnds.data();
        in.plane_offsets = mPlaneOff.data(); in.plane_meas = mPlaneMeas.data(); in.plane_world = mPlaneWorld.data();
        in.plane_mask = mPlaneMask.data();
        const double st[7] = {mSettings.angleInfo, mSettings.distanceInfo, mSettings.parallelInfo, mSettings.verticalInfo, mSettings.chi,
                              mSettings.vpChi, 0.0};
        std::memcpy(in.plane_settings, st, sizeof(st));
        drfe_pose_opt_out out = {Tcw.data(), mReturns.data(), rounds.data(), its.data(), trials.data(), nullptr,
                                 po.data(), lo.data(), pl.data(), pp.data(), pv.data()};
        struct ClearOnExit {                           /* also when an entry refuses the call: the batch never keeps stale frames */
            PoseOptBatch* b; std::vector<int32_t>* ret;
            ~ClearOnExit() { std::vector<int32_t> r; r.swap(*ret); b->Clear(); b->mReturns.swap(r); }
        } clearOnExit{this, &mReturns};
        if (n) {
            if ((int64_t)n < (int64_t)mDeviceFrom) {
                const int rc = TransOnly ? drfe_trans_opt_host(&in, &out) : drfe_pose_opt_host(&in, &out);
                if (rc != DRFE_OK) {
                    mReturns.clear();
                    throw std::runtime_error(TransOnly ? "drfe_trans_opt_host: invalid argument" : "drfe_pose_opt_host: invalid argument");
                }
            } else {
                if (!mCtx) mCtx = Planar_SLAM::drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, mDevice);
                if (TransOnly)
                    Planar_SLAM::drfe_detail::check(drfe_trans_opt_batch(mCtx.get(), &in, &out, nullptr), mCtx.get(), "drfe_trans_opt_batch");
                else
                    Planar_SLAM::drfe_detail::check(drfe_pose_opt_batch(mCtx.get(), &in, &out, nullptr), mCtx.get(), "drfe_pose_opt_batch");
            }
        }
        for (size_t f = 0; f < n; f++) {
            FrameT& F = *mFrames[f];
            for (int32_t k = mPointOff[f]; k < mPointOff[f + 1]; k++) F.mvbOutlier[(size_t)mPointIdx[(size_t)k]] = po[(size_t)k] != 0;
            for (int32_t k = mLineOff[f]; k < mLineOff[f + 1]; k++) F.mvbLineOutlier[(size_t)mLineIdx[(size_t)k]] = lo[(size_t)k] != 0;
            for (int32_t k = mPlaneOff[f]; k < mPlaneOff[f + 1]; k++) {
                const size_t i = (size_t)(k - mPlaneOff[f]);
                const uint8_t m = mPlaneMask[(size_t)k];
                if (m & DRFE_POSE_OPT_PLANE_MATCHED) F.mvbPlaneOutlier[i] = pl[(size_t)k] != 0;
                if (mStruct[f] && (m & DRFE_POSE_OPT_PLANE_PARALLEL)) F.mvbParPlaneOutlier[i] = pp[(size_t)k] != 0;
                if (mStruct[f] && (m & DRFE_POSE_OPT_PLANE_VERTICAL)) F.mvbVerPlaneOutlier[i] = pv[(size_t)k] != 0;
            }
            const int nInitial = (mPointOff[f + 1] - mPointOff[f]) + (TransOnly ? 0 : (mLineOff[f + 1] - mLineOff[f]) + PlaneEdges(f));
            if (nInitial >= 3) {                       /* below three correspondences the reference returns before SetPose */
                F.SetPose(drfe_detail_sim3::mat32(4, 4, &Tcw[16 * f]));
            }
        }
    }
    int Result(size_t i) const { return mReturns.at(i); }
    drfe_ctx* ctx() const { return mCtx.get(); }

private:
    int PlaneEdges(size_t f) const
    {
        int e = 0;
        for (int32_t k = mPlaneOff[f]; k < mPlaneOff[f + 1]; k++) {
            const uint8_t m = mPlaneMask[(size_t)k];
            e += (m & 1) + (mStruct[f] ? ((m >> 1) & 1) + ((m >> 2) & 1) : 0);
        }
        return e;
    }
    PlaneSettings mSettings;
    int mDevice, mDeviceFrom;
    Planar_SLAM::drfe_detail::CtxPtr mCtx;
    std::vector<FrameT*> mFrames;
    std::vector<uint8_t> mStruct, mPlaneMask;
    std::vector<float> mTcw, mK, mBf, mObs, mUr, mInvSigma2, mXw, mPlaneMeas, mPlaneWorld;
    std::vector<double> mLineFn, mLineEnds;
    std::vector<int32_t> mPointOff, mLineOff, mPlaneOff, mPointIdx, mLineIdx, mReturns;
};

template <class FrameT> using TransOptBatch = PoseOptBatch<FrameT, true>;

/* Optimizer::OptimizeSim3 (src/Optimizer.cc:3982-4177) for one loop candidate or for the live candidates of one round of
 * LoopClosing::ComputeSim3's loop (src/LoopClosing.cc:333-388): Add() flattens what the reference reads of a candidate, leaving out
 * a match as its `continue`s do (vpMatches1[i] NULL, either map point NULL or bad, i2 < 0); Run() optimises every added candidate
 * by one drfe_sim3_opt_batch call (or, below `deviceFrom` candidates, by the host entry: same bits) and writes back what the
 * reference writes: vpMatches1[i] = NULL for the matches either classification rejects, and g2oS12.  Result(i) is the i-th added
 * candidate's return value, Scw(i) its mScw = toCvMat(g2oS12 * Sim3(R2w, t2w, 1)), T12(i) toCvMat(g2oS12).  An object belongs to
 * one thread.  DESIGN.md section 22.  No g2o here:
 * Sim3T: rotation() with x() y() z() w(), translation() with operator[], scale(), each also as a reference to write through
 * (g2o::Sim3 is one).  KeyFrameT: mK (3x3 float), GetRotation(), GetTranslation(), GetMapPointMatches(), mvKeysUn,
 * mvInvLevelSigma2.  MapPointT: isBad(), GetWorldPos(), GetIndexInKeyFrame(KeyFrameT*). */
template <class KeyFrameT, class MapPointT, class Sim3T>
class Sim3OptBatch {
public:
    explicit Sim3OptBatch(int device = 0, int deviceFrom = (int)DRFE_SIM3OPT_DEVICE_FROM) : mDevice(device), mDeviceFrom(deviceFrom) { Clear(); }
    /* true / false: the device / the host entry whatever the number of candidates */
    void UseDevice(bool on) { mDeviceFrom = on ? 0 : 2147483647; }
    void Clear()
    {
        mMatches.clear(); mSims.clear(); mS12.clear(); mK1.clear(); mK2.clear(); mR1w.clear(); mt1w.clear(); mR2w.clear(); mt2w.clear();
        mTh2.clear(); mFix.clear(); mOff.assign(1, 0); mIdx.clear(); mP1.clear(); mP2.clear(); mObs1.clear(); mObs2.clear();
        mInv1.clear(); mInv2.clear();
    }
    size_t size() const { return mSims.size(); }
    void Add(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12, const float th2, const bool bFixScale)
    {
        using Planar_SLAM::drfe_detail::mat_f;
        mMatches.push_back(&vpMatches1);
        mSims.push_back(&g2oS12);
        const auto& r = g2oS12.rotation();
        mS12.push_back(r.x()); mS12.push_back(r.y()); mS12.push_back(r.z()); mS12.push_back(r.w());
        for (int k = 0; k < 3; k++) mS12.push_back(g2oS12.translation()[k]);
        mS12.push_back(g2oS12.scale());
        KeyFrameT* kf[2] = {pKF1, pKF2};
        std::vector<float>* K[2] = {&mK1, &mK2};
        std::vector<float>* R[2] = {&mR1w, &mR2w};
        std::vector<float>* t[2] = {&mt1w, &mt2w};
        for (int q = 0; q < 2; q++) {
            K[q]->push_back(mat_f(kf[q]->mK, 0, 0)); K[q]->push_back(mat_f(kf[q]->mK, 1, 1));
            K[q]->push_back(mat_f(kf[q]->mK, 0, 2)); K[q]->push_back(mat_f(kf[q]->mK, 1, 2));
            const auto Rm = kf[q]->GetRotation();
            const auto tm = kf[q]->GetTranslation();
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[q]->push_back(mat_f(Rm, i, j));
            for (int i = 0; i < 3; i++) t[q]->push_back(mat_f(tm, i));
        }
        mTh2.push_back(th2);
        mFix.push_back(bFixScale ? 1 : 0);
        const int N = (int)vpMatches1.size();
        const auto vpMapPoints1 = pKF1->GetMapPointMatches();
        for (int i = 0; i < N; i++) {
            if (!vpMatches1[(size_t)i]) continue;
            MapPointT* pMP1 = vpMapPoints1[(size_t)i];
            MapPointT* pMP2 = vpMatches1[(size_t)i];
            const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (!pMP1 || !pMP2 || pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
            const auto P3D1w = pMP1->GetWorldPos();
            const auto P3D2w = pMP2->GetWorldPos();
            for (int k = 0; k < 3; k++) { mP1.push_back(mat_f(P3D1w, k)); mP2.push_back(mat_f(P3D2w, k)); }
            const auto& kpUn1 = pKF1->mvKeysUn[(size_t)i];
            const auto& kpUn2 = pKF2->mvKeysUn[(size_t)i2];
            mObs1.push_back(kpUn1.pt.x); mObs1.push_back(kpUn1.pt.y);
            mObs2.push_back(kpUn2.pt.x); mObs2.push_back(kpUn2.pt.y);
            mInv1.push_back(pKF1->mvInvLevelSigma2[(size_t)kpUn1.octave]);
            mInv2.push_back(pKF2->mvInvLevelSigma2[(size_t)kpUn2.octave]);
            mIdx.push_back(i);
        }
        mOff.push_back((int32_t)mIdx.size());
    }
    /* optimises every added candidate and writes the matches and estimates back; the batch is empty afterwards but for Result(),
     * T12() and Scw() */
    void Run()
    {
        const size_t n = mSims.size();
        std::vector<double> S12(8 * n + 1);
        std::vector<int32_t> nBad(n + 1), its(2 * n + 1), trials(2 * n + 1);
        std::vector<uint8_t> outlier(mIdx.size() + 1);
        mReturns.assign(n, 0); mT12.assign(16 * n, 0.f); mScw.assign(16 * n, 0.f);
        drfe_sim3_opt_problems in = {};
        in.n = (int32_t)n;
        in.S12 = mS12.data(); in.K1 = mK1.data(); in.K2 = mK2.data(); in.R1w = mR1w.data(); in.t1w = mt1w.data();
        in.R2w = mR2w.data(); in.t2w = mt2w.data(); in.th2 = mTh2.data(); in.fix_scale = mFix.data(); in.match_offsets = mOff.data();
        in.index = mIdx.data(); in.P3D1w = mP1.data(); in.P3D2w = mP2.data(); in.obs1 = mObs1.data(); in.obs2 = mObs2.data();
        in.inv_sigma2_1 = mInv1.data(); in.inv_sigma2_2 = mInv2.data();
        drfe_sim3_opt_out out = {S12.data(), mT12.data(), mScw.data(), mReturns.data(), nBad.data(), its.data(), trials.data(), nullptr,
                                 outlier.data()};
        struct ClearOnExit {                           /* also when an entry refuses the call: the batch never keeps stale candidates */
            Sim3OptBatch* b;
            ~ClearOnExit() { b->Clear(); }
        } clearOnExit{this};
        if (n) {
            if ((int64_t)n < (int64_t)mDeviceFrom) {
                if (drfe_sim3_opt_host(&in, &out) != DRFE_OK) {
                    mReturns.clear();
                    throw std::runtime_error("drfe_sim3_opt_host: invalid argument");
                }
            } else {
                if (!mCtx) mCtx = Planar_SLAM::drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, mDevice);
                Planar_SLAM::drfe_detail::check(drfe_sim3_opt_batch(mCtx.get(), &in, &out, nullptr), mCtx.get(), "drfe_sim3_opt_batch");
            }
        }
        for (size_t f = 0; f < n; f++) {
            for (int32_t k = mOff[f]; k < mOff[f + 1]; k++)
                if (outlier[(size_t)k]) (*mMatches[f])[(size_t)mIdx[(size_t)k]] = static_cast<MapPointT*>(nullptr);
            Sim3T& S = *mSims[f];
            const double* v = &S12[8 * f];
            auto& r = S.rotation();
            r.x() = v[0]; r.y() = v[1]; r.z() = v[2]; r.w() = v[3];
            for (int k = 0; k < 3; k++) S.translation()[k] = v[4 + k];
            S.scale() = v[7];
        }
    }
    int Result(size_t i) const { return mReturns.at(i); }
    drfe_cv::Mat T12(size_t i) const { return drfe_detail_sim3::mat32(4, 4, &mT12.at(16 * i)); }
    drfe_cv::Mat Scw(size_t i) const { return drfe_detail_sim3::mat32(4, 4, &mScw.at(16 * i)); }
    drfe_ctx* ctx() const { return mCtx.get(); }

private:
    int mDevice, mDeviceFrom;
    Planar_SLAM::drfe_detail::CtxPtr mCtx;
    std::vector<std::vector<MapPointT*>*> mMatches;
    std::vector<Sim3T*> mSims;
    std::vector<double> mS12;
    std::vector<float> mK1, mK2, mR1w, mt1w, mR2w, mt2w, mTh2, mP1, mP2, mObs1, mObs2, mInv1, mInv2, mT12, mScw;
    std::vector<uint8_t> mFix;
    std::vector<int32_t> mOff, mIdx, mReturns;
};

}  // namespace drfe

namespace Planar_SLAM {

/* include/Optimizer.h: the two entries of the reference's Optimizer this library builds.  The reference reads the plane settings
 * from its Config singleton; here they are set once (SetPlaneSettings), as is the choice of the entry: a single frame is below
 * DRFE_POSEOPT_DEVICE_FROM and DRFE_TRANSOPT_DEVICE_FROM (the measured crossovers), so it takes the host entry unless
 * UseDevice(true). */
class Optimizer {
public:
    static drfe::PlaneSettings& Settings() { static drfe::PlaneSettings s; return s; }
    static void SetPlaneSettings(const drfe::PlaneSettings& s) { Settings() = s; }
    static bool& DeviceFlag() { static bool on = 1 >= DRFE_POSEOPT_DEVICE_FROM; return on; }
    static void UseDevice(bool on) { DeviceFlag() = on; TransDeviceFlag() = on; Sim3DeviceFlag() = on; }
    template <class FrameT> static int PoseOptimization(FrameT* pFrame, bool bStruct)
    {
        static thread_local drfe::PoseOptBatch<FrameT> batch;       /* keeps its context between calls */
        batch.SetSettings(Settings());
        batch.UseDevice(DeviceFlag());
        batch.Clear();
        batch.Add(pFrame, bStruct);
        batch.Run();
        return batch.Result(0);
    }
    /* TranslationWithMotionModel / TranslationEstimation: mTcw holds the Manhattan rotation, only t is optimised */
    template <class FrameT> static int TranslationOptimization(FrameT* pFrame, bool bStruct)
    {
        static thread_local drfe::TransOptBatch<FrameT> batch;      /* keeps its context between calls */
        batch.SetSettings(Settings());
        batch.UseDevice(TransDeviceFlag());
        batch.Clear();
        batch.Add(pFrame, bStruct);
        batch.Run();
        return batch.Result(0);
    }

    /* LoopClosing::ComputeSim3's call; LastScw() is mScw of the last call on this thread (src/LoopClosing.cc:379-381) */
    template <class KeyFrameT, class MapPointT, class Sim3T>
    static int OptimizeSim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12, const float th2,
                            const bool bFixScale)
    {
        static thread_local drfe::Sim3OptBatch<KeyFrameT, MapPointT, Sim3T> batch;   /* keeps its context between calls */
        batch.UseDevice(Sim3DeviceFlag());
        batch.Clear();
        batch.Add(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale);
        batch.Run();
        LastScw() = batch.Scw(0);
        return batch.Result(0);
    }
    static drfe_cv::Mat& LastScw() { static thread_local drfe_cv::Mat m; return m; }

private:
    static bool& TransDeviceFlag() { static bool on = 1 >= DRFE_TRANSOPT_DEVICE_FROM; return on; }
    static bool& Sim3DeviceFlag() { static bool on = 1 >= DRFE_SIM3OPT_DEVICE_FROM; return on; }
};

}  // namespace Planar_SLAM

namespace Planar_SLAM {

/* include/KeyFrameDatabase.h over drfe_kfdb: the reference's five signatures, so that LoopClosing.cc and
 * Tracking.cc compile unchanged against KeyFrameDatabase<KeyFrame, Frame>, and the two batch forms.  A key frame's handle is its
 * mnId, a query's id the mnId of its key frame / frame (the reference compares mnLoopQuery / mnRelocQuery with it): ids must grow
 * from query to query, as the reference's do.  A key frame's mBowVec is stored when the database first meets it (add, a query, a
 * connected or covisible key frame of a query) and is not read again.  Before every query call the GetBestCovisibilityKeyFrames(10)
 * row of every key frame the database knows and that is not bad is sent again: one pass over the key frames per call, not per
 * query, which is the price of not being told when the covisibility graph changes.  Forget(pKF) drops a culled key frame.
 * `device` < 0 (the default) is a host-only database; with a device, a call of DRFE_KFDB_DEVICE_FROM queries or more runs there.
 * KeyFrameT: mnId, mBowVec (iterable pairs of word id and value), isBad(), GetConnectedKeyFrames(), GetVectorCovisibleKeyFrames(),
 * GetBestCovisibilityKeyFrames(int).  FrameT: mnId, mBowVec. */
template <class KeyFrameT, class FrameT>
class KeyFrameDatabase {
public:
    explicit KeyFrameDatabase(int device = -1) { Open(device); }
    /* the reference's constructor: the vocabulary only sizes its inverted file */
    template <class Voc> explicit KeyFrameDatabase(const Voc&, int device = -1) { Open(device); }
    ~KeyFrameDatabase() { drfe_kfdb_destroy(mDb); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;
    /* true / false: the device / the host entries whatever the number of queries (the device needs `device` >= 0) */
    void UseDevice(bool on) { mForce = on ? 1 : -1; }

    void add(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        Know(pKF);
        Check(drfe_kfdb_add(mDb, Handle(pKF)), "drfe_kfdb_add");
        mVisible.insert(Handle(pKF));
    }
    /* as the reference's, a key frame that is not in the inverted file is left alone */
    void erase(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (!mVisible.erase(Handle(pKF))) return;
        Check(drfe_kfdb_erase(mDb, Handle(pKF)), "drfe_kfdb_erase");
    }
    void clear()
    {
        std::unique_lock<std::mutex> lock(mMutex);
        Check(drfe_kfdb_clear(mDb), "drfe_kfdb_clear");
        mVisible.clear();
    }
    /* a culled key frame: out of the inverted file and out of the database's tables */
    void Forget(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (!mKFs.erase(Handle(pKF))) return;
        mVisible.erase(Handle(pKF));
        Check(drfe_kfdb_remove(mDb, Handle(pKF)), "drfe_kfdb_remove");
    }

    std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore)
    {
        std::vector<KeyFrameT*> queue(1, pKF);
        std::vector<float> ms(1, minScore);
        return Loop(queue, &ms, false)[0];
    }
    /* LoopClosing::DetectLoop's :137-167 for a queue of key frames in one call: minScore of each from its
     * GetVectorCovisibleKeyFrames() (bad ones left out), and with addAfter the add() that follows each query, so that a later key
     * frame of the queue meets the earlier ones.  MinScores() holds the minScore each query used. */
    std::vector<std::vector<KeyFrameT*>> DetectLoopCandidates(const std::vector<KeyFrameT*>& queue, bool addAfter)
    {
        return Loop(queue, nullptr, addAfter);
    }
    std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F)
    {
        return DetectRelocalizationCandidates(std::vector<FrameT*>(1, F))[0];
    }
    /* every lost frame of a batched tracker in one call, as if asked one after another */
    std::vector<std::vector<KeyFrameT*>> DetectRelocalizationCandidates(const std::vector<FrameT*>& frames)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const size_t n = frames.size();
        std::vector<int64_t> id(n);
        std::vector<int32_t> off(1, 0), words;
        std::vector<double> values;
        for (size_t k = 0; k < n; k++) {
            id[k] = (int64_t)frames[k]->mnId;
            Flatten(frames[k]->mBowVec, words, values);
            off.push_back((int32_t)words.size());
        }
        drfe_kfdb_reloc_queries q = {};
        q.n = (int32_t)n;
        q.id = id.data(); q.word_offsets = off.data(); q.word_ids = words.data(); q.values = values.data();
        return Run(n, [&](drfe_kfdb_out* o) {
            return mForce < 0 ? drfe_kfdb_reloc_queries_host(mDb, &q, o)
                 : mForce > 0 ? drfe_kfdb_reloc_queries_device(mDb, &q, o, nullptr) : drfe_kfdb_reloc_queries_batch(mDb, &q, o, nullptr);
        }, "drfe_kfdb_reloc_queries");
    }
    /* of the last query call: the minScore of each loop query, the reads of a never-written mRelocScore of each relocalisation
     * query (where the reference itself reads an uninitialised float), and listed / scored / kept / maxCommonWords of each */
    const std::vector<float>& MinScores() const { return mMinScore; }
    const std::vector<int32_t>& UninitReads() const { return mUninit; }
    const std::vector<int32_t>& Records() const { return mRecord; }
    drfe_kfdb* db() const { return mDb; }

private:
    static int32_t Handle(const KeyFrameT* pKF) { return (int32_t)pKF->mnId; }
    void Open(int device)
    {
        if (device >= 0) mCtx = drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, device);
        if (drfe_kfdb_create(mCtx.get(), DRFE_KFDB_L1_NORM, &mDb) != DRFE_OK) throw std::runtime_error("drfe_kfdb_create failed");
    }
    void Check(int rc, const char* what) const
    {
        if (rc != DRFE_OK) throw std::runtime_error(std::string(what) + ": " + drfe_kfdb_last_error(mDb));
    }
    template <class Bow> static void Flatten(const Bow& bow, std::vector<int32_t>& words, std::vector<double>& values)
    {
        for (auto it = bow.begin(); it != bow.end(); ++it) {
            words.push_back((int32_t)it->first);
            values.push_back((double)it->second);
        }
    }
    void Know(KeyFrameT* pKF)
    {
        if (mKFs.count(Handle(pKF))) return;
        std::vector<int32_t> words;
        std::vector<double> values;
        Flatten(pKF->mBowVec, words, values);
        Check(drfe_kfdb_put(mDb, Handle(pKF), (int32_t)words.size(), words.data(), values.data()), "drfe_kfdb_put");
        mKFs[Handle(pKF)] = pKF;
    }
    /* a neighbour the database has not met is in no inverted file: it cannot pass either query's neighbour test */
    void RefreshNeighbours()
    {
        std::vector<int32_t> handles, rows;
        for (auto& kv : mKFs) {
            if (kv.second->isBad()) continue;
            handles.push_back(kv.first);
            const auto vpNeighs = kv.second->GetBestCovisibilityKeyFrames(DRFE_KFDB_NEIGHBOURS);
            size_t k = 0;
            for (; k < vpNeighs.size() && k < (size_t)DRFE_KFDB_NEIGHBOURS; k++)
                rows.push_back(mKFs.count(Handle(vpNeighs[k])) ? Handle(vpNeighs[k]) : -1);
            for (; k < (size_t)DRFE_KFDB_NEIGHBOURS; k++) rows.push_back(-1);
        }
        Check(drfe_kfdb_set_neighbours(mDb, (int32_t)handles.size(), handles.data(), rows.data()), "drfe_kfdb_set_neighbours");
    }
    template <class Fn> std::vector<std::vector<KeyFrameT*>> Run(size_t n, Fn call, const char* what)
    {
        RefreshNeighbours();
        int32_t size[2] = {0, 0};
        Check(drfe_kfdb_size(mDb, size), "drfe_kfdb_size");
        std::vector<int32_t> off(n + 1, 0), cand(n * ((size_t)size[1] + n) + 1);
        mRecord.assign(4 * n, 0);
        mMinScore.assign(n, 0.f);
        mUninit.assign(n, 0);
        drfe_kfdb_out o = {};
        o.cand_capacity = (int32_t)cand.size();
        o.cand_offsets = off.data(); o.candidates = cand.data(); o.record = mRecord.data();
        o.min_score = mMinScore.data(); o.uninit_reads = mUninit.data();
        Check(call(&o), what);
        std::vector<std::vector<KeyFrameT*>> out(n);
        for (size_t k = 0; k < n; k++)
            for (int32_t i = off[k]; i < off[k + 1]; i++) out[k].push_back(mKFs.at(cand[(size_t)i]));
        return out;
    }
    std::vector<std::vector<KeyFrameT*>> Loop(const std::vector<KeyFrameT*>& queue, const std::vector<float>* minScore, bool addAfter)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const size_t n = queue.size();
        std::vector<int32_t> handle(n), connOff(1, 0), conn, covOff(1, 0), cov;
        std::vector<int64_t> id(n);
        std::vector<uint8_t> after(n, addAfter ? 1 : 0);
        for (size_t k = 0; k < n; k++) {
            KeyFrameT* pKF = queue[k];
            Know(pKF);
            handle[k] = Handle(pKF);
            id[k] = (int64_t)pKF->mnId;
            for (KeyFrameT* c : pKF->GetConnectedKeyFrames()) {
                Know(c);
                conn.push_back(Handle(c));
            }
            connOff.push_back((int32_t)conn.size());
            if (!minScore)
                for (KeyFrameT* c : pKF->GetVectorCovisibleKeyFrames()) {
                    if (c->isBad()) continue;
                    Know(c);
                    cov.push_back(Handle(c));
                }
            covOff.push_back((int32_t)cov.size());
        }
        drfe_kfdb_loop_queries q = {};
        q.n = (int32_t)n;
        q.handle = handle.data(); q.id = id.data(); q.connected_offsets = connOff.data(); q.connected = conn.data();
        q.min_score = minScore ? minScore->data() : nullptr;
        q.covisible_offsets = covOff.data(); q.covisible = cov.data(); q.add_after = after.data();
        auto out = Run(n, [&](drfe_kfdb_out* o) {
            return mForce < 0 ? drfe_kfdb_loop_queries_host(mDb, &q, o)
                 : mForce > 0 ? drfe_kfdb_loop_queries_device(mDb, &q, o, nullptr) : drfe_kfdb_loop_queries_batch(mDb, &q, o, nullptr);
        }, "drfe_kfdb_loop_queries");
        if (addAfter)
            for (size_t k = 0; k < n; k++) mVisible.insert(handle[k]);
        return out;
    }

    drfe_detail::CtxPtr mCtx;
    drfe_kfdb* mDb = nullptr;
    int mForce = 0;
    std::mutex mMutex;
    std::map<int32_t, KeyFrameT*> mKFs;
    std::set<int32_t> mVisible;
    std::vector<float> mMinScore;
    std::vector<int32_t> mUninit, mRecord;
};

/* Tracking::UpdateLocalMap (src/Tracking.cc:3383-3541) over drfe_lmap: what UpdateLocalKeyFrames,
 * UpdateLocalPoints and UpdateLocalLines leave, for one frame or for every frame of a batched tracker in one call.  The store holds
 * a copy of the graph: Sync(pKF) / Sync(pMP) / Sync(pML) read an object's accessors again (after KeyFrame::UpdateConnections,
 * AddMapPoint, AddObservation, SetBadFlag, ...), Forget drops a culled one.  Handles are the objects' mnId (one space per class),
 * a key frame's rank is its address: the order in which the reference walks map<KeyFrame*, int> and set<KeyFrame*>.  A query on a
 * store in which some reference names an object that was never synced throws with the store's message.
 * `device` < 0 (the default) is a host-only store; with a device, a call of DRFE_LMAP_DEVICE_FROM frames or more runs there.
 * KeyFrameT: mnId, mnTrackReferenceForFrame, isBad(), GetParent(), GetChilds(), GetBestCovisibilityKeyFrames(int),
 * GetMapPointMatches(), GetMapLineMatches().  MapPointT: mnId, mnTrackReferenceForFrame, isBad(), GetObservations() (iterable
 * pairs whose first is a KeyFrameT*).  MapLineT: mnId, mnTrackReferenceForFrame, isBad().  FrameT: mnId, mvpMapPoints,
 * mvpMapLines, mpReferenceKF. */
template <class KeyFrameT, class MapPointT, class MapLineT, class FrameT>
class LocalMapTracker {
public:
    /* what UpdateLocalMap leaves for one frame.  kfs goes in as mvpLocalKeyFrames of the previous frame (kept when no point of the
     * frame votes).  mpInFrame / mlInFrame: 1 for a local point / line that the frame itself holds, which SearchLocalPoints /
     * SearchLocalLines stamp with mnLastFrameSeen instead of projecting. */
    struct Local {
        std::vector<KeyFrameT*> kfs;
        std::vector<MapPointT*> mps;
        std::vector<MapLineT*> mls;
        std::vector<uint8_t> mpInFrame, mlInFrame;
        KeyFrameT* ref = nullptr;          /* pKFmax, or nullptr: mpReferenceKF stays */
        int32_t record[4] = {0, 0, 0, 0};
    };

    explicit LocalMapTracker(int device = -1)
    {
        if (device >= 0) mCtx = drfe_detail::make_ctx(1, 1.2f, 1, 20, 7, 64, 64, 1, device);
        if (drfe_lmap_create(mCtx.get(), &mDb) != DRFE_OK) throw std::runtime_error("drfe_lmap_create failed");
    }
    ~LocalMapTracker() { drfe_lmap_destroy(mDb); }
    LocalMapTracker(const LocalMapTracker&) = delete;
    LocalMapTracker& operator=(const LocalMapTracker&) = delete;
    /* true / false: the device / the host entry whatever the number of frames (the device needs `device` >= 0) */
    void UseDevice(bool on) { mForce = on ? 1 : -1; }

    void Sync(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pKF->mnId;
        const uint64_t rank = (uint64_t)reinterpret_cast<uintptr_t>(pKF);
        const uint8_t bad = pKF->isBad() ? 1 : 0;
        KeyFrameT* pParent = pKF->GetParent();
        const int32_t parent = pParent ? (int32_t)pParent->mnId : -1;
        int32_t nbr[DRFE_LMAP_NEIGHBOURS];
        const auto vNeighs = pKF->GetBestCovisibilityKeyFrames(DRFE_LMAP_NEIGHBOURS);
        for (size_t k = 0; k < (size_t)DRFE_LMAP_NEIGHBOURS; k++) nbr[k] = k < vNeighs.size() ? (int32_t)vNeighs[k]->mnId : -1;
        std::vector<int32_t> children, points, lines;
        for (KeyFrameT* c : pKF->GetChilds()) children.push_back((int32_t)c->mnId);
        for (MapPointT* p : pKF->GetMapPointMatches()) points.push_back(p ? (int32_t)p->mnId : -1);
        for (MapLineT* l : pKF->GetMapLineMatches()) lines.push_back(l ? (int32_t)l->mnId : -1);
        const int32_t cOff[2] = {0, (int32_t)children.size()}, pOff[2] = {0, (int32_t)points.size()}, lOff[2] = {0, (int32_t)lines.size()};
        drfe_lmap_keyframes r = {};
        r.count = 1;
        r.handle = &handle; r.rank = &rank; r.bad = &bad; r.parent = &parent; r.neighbours = nbr;
        r.child_offsets = cOff; r.children = children.data(); r.point_offsets = pOff; r.points = points.data();
        r.line_offsets = lOff; r.lines = lines.data();
        Check(drfe_lmap_set_keyframes(mDb, &r), "drfe_lmap_set_keyframes");
        mKFs[handle] = pKF;
    }
    void Sync(MapPointT* pMP)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pMP->mnId;
        const uint8_t bad = pMP->isBad() ? 1 : 0;
        std::vector<int32_t> obs;
        for (const auto& o : pMP->GetObservations()) obs.push_back((int32_t)o.first->mnId);
        const int32_t off[2] = {0, (int32_t)obs.size()};
        Check(drfe_lmap_set_points(mDb, 1, &handle, &bad, off, obs.data()), "drfe_lmap_set_points");
        mMPs[handle] = pMP;
    }
    void Sync(MapLineT* pML)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pML->mnId;
        const uint8_t bad = pML->isBad() ? 1 : 0;
        Check(drfe_lmap_set_lines(mDb, 1, &handle, &bad), "drfe_lmap_set_lines");
        mMLs[handle] = pML;
    }
    /* a culled object; one the store never met is left alone */
    void Forget(KeyFrameT* pKF) { Drop(mKFs, DRFE_LMAP_KEYFRAME, (int32_t)pKF->mnId); }
    void Forget(MapPointT* pMP) { Drop(mMPs, DRFE_LMAP_POINT, (int32_t)pMP->mnId); }
    void Forget(MapLineT* pML) { Drop(mMLs, DRFE_LMAP_LINE, (int32_t)pML->mnId); }

    /* Tracking::UpdateLocalMap for mCurrentFrame: the three vectors are Tracking's mvpLocalKeyFrames, mvpLocalMapPoints and
     * mvpLocalMapLines, refKF its mpReferenceKF */
    void UpdateLocalMap(FrameT& F, std::vector<KeyFrameT*>& localKFs, std::vector<MapPointT*>& localMPs, std::vector<MapLineT*>& localMLs,
                        KeyFrameT*& refKF)
    {
        std::vector<Local> one(1);
        one[0].kfs.swap(localKFs);
        UpdateLocalMap(std::vector<FrameT*>(1, &F), one);
        localKFs.swap(one[0].kfs);
        localMPs.swap(one[0].mps);
        localMLs.swap(one[0].mls);
        if (one[0].ref) refKF = one[0].ref;
    }
    /* every frame of a batched tracker in one call (mnId ascending), each with its own tracker's lists */
    void UpdateLocalMap(const std::vector<FrameT*>& frames, std::vector<Local>& locals)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const size_t n = frames.size();
        if (locals.size() != n) throw std::runtime_error("LocalMapTracker: one Local per frame");
        std::vector<int64_t> id(n);
        std::vector<int32_t> pOff(1, 0), pts, lOff(1, 0), lns, vOff(1, 0), prev;
        for (size_t k = 0; k < n; k++) {
            id[k] = (int64_t)frames[k]->mnId;
            for (MapPointT* p : frames[k]->mvpMapPoints) pts.push_back(p ? (int32_t)p->mnId : -1);
            for (MapLineT* l : frames[k]->mvpMapLines) lns.push_back(l ? (int32_t)l->mnId : -1);
            for (KeyFrameT* kf : locals[k].kfs) prev.push_back((int32_t)kf->mnId);
            pOff.push_back((int32_t)pts.size());
            lOff.push_back((int32_t)lns.size());
            vOff.push_back((int32_t)prev.size());
        }
        int32_t size[3] = {0, 0, 0};
        Check(drfe_lmap_size(mDb, size), "drfe_lmap_size");
        std::vector<int32_t> kfOff(n + 1), mpOff(n + 1), mlOff(n + 1), nuOff(n + 1), ref(n), rec(4 * n);
        std::vector<int32_t> kfs(n * (size_t)size[0] + prev.size() + 1), mps(n * (size_t)size[1] + 1), mls(n * (size_t)size[2] + 1), nulled(pts.size() + 1);
        std::vector<uint8_t> mpIn(mps.size()), mlIn(mls.size());
        drfe_lmap_queries q = {};
        q.n = (int32_t)n;
        q.frame_id = id.data(); q.point_offsets = pOff.data(); q.points = pts.data(); q.line_offsets = lOff.data(); q.lines = lns.data();
        q.prev_kf_offsets = vOff.data(); q.prev_kfs = prev.data();
        drfe_lmap_out o = {};
        o.kf_capacity = (int32_t)kfs.size(); o.mp_capacity = (int32_t)mps.size(); o.ml_capacity = (int32_t)mls.size();
        o.nulled_capacity = (int32_t)nulled.size();
        o.kf_offsets = kfOff.data(); o.kfs = kfs.data(); o.ref_kf = ref.data(); o.mp_offsets = mpOff.data(); o.mps = mps.data();
        o.mp_in_frame = mpIn.data(); o.ml_offsets = mlOff.data(); o.mls = mls.data(); o.ml_in_frame = mlIn.data();
        o.nulled_offsets = nuOff.data(); o.nulled = nulled.data(); o.record = rec.data();
        Check(mForce < 0 ? drfe_lmap_update_host(mDb, &q, &o)
            : mForce > 0 ? drfe_lmap_update_device(mDb, &q, &o, nullptr) : drfe_lmap_update_batch(mDb, &q, &o, nullptr), "drfe_lmap_update");
        for (size_t k = 0; k < n; k++) {
            FrameT& F = *frames[k];
            Local& L = locals[k];
            const auto fid = F.mnId;
            for (int32_t i = nuOff[k]; i < nuOff[k + 1]; i++) F.mvpMapPoints[(size_t)nulled[(size_t)i]] = nullptr;
            L.kfs.clear(); L.mps.clear(); L.mls.clear();
            for (int f = 0; f < 4; f++) L.record[f] = rec[4 * k + (size_t)f];
            /* the early return stamps no key frame: the list is the previous frame's */
            const bool voted = L.record[0] > 0;
            for (int32_t i = kfOff[k]; i < kfOff[k + 1]; i++) {
                KeyFrameT* pKF = mKFs.at(kfs[(size_t)i]);
                L.kfs.push_back(pKF);
                if (voted) pKF->mnTrackReferenceForFrame = fid;
            }
            for (int32_t i = mpOff[k]; i < mpOff[k + 1]; i++) {
                MapPointT* pMP = mMPs.at(mps[(size_t)i]);
                L.mps.push_back(pMP);
                pMP->mnTrackReferenceForFrame = fid;
            }
            for (int32_t i = mlOff[k]; i < mlOff[k + 1]; i++) {
                MapLineT* pML = mMLs.at(mls[(size_t)i]);
                L.mls.push_back(pML);
                pML->mnTrackReferenceForFrame = fid;
            }
            L.mpInFrame.assign(mpIn.begin() + mpOff[k], mpIn.begin() + mpOff[k + 1]);
            L.mlInFrame.assign(mlIn.begin() + mlOff[k], mlIn.begin() + mlOff[k + 1]);
            L.ref = ref[k] >= 0 ? mKFs.at(ref[k]) : nullptr;
            if (L.ref) F.mpReferenceKF = L.ref;
        }
    }
    /* KeyFrame::UpdateConnections (src/KeyFrame.cc:366-500) of pKF on the store.  Further accessors of
     * KeyFrameT: GetConnectedKeyFrames(), GetVectorCovisibleKeyFrames(), GetWeight(KeyFrameT*), AddChild(KeyFrameT*) and one setter
     * that the integrator adds: SetConnections(const std::map<KeyFrameT*, int>& weights,
     * const std::vector<KeyFrameT*>& ordered, const std::vector<int>& orderedWeights, KeyFrameT* parent, bool firstConnection).
     * mbFirstConnection has no accessor: it is read as mnId != 0 && GetParent() == nullptr, which is what it is while the key
     * frame's parent is only ever set by UpdateConnections and ChangeParent. */
    /* the connection state of pKF into the store: its weights, its ordered list and mbFirstConnection && mnId != 0.  Call it with
     * Sync(pKF) when a key frame enters the store, and after anything but UpdateConnections below wrote its connections. */
    void SyncConnections(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pKF->mnId;
        const uint8_t first = pKF->mnId != 0 && pKF->GetParent() == nullptr ? 1 : 0;
        std::vector<int32_t> wKf, wW, oKf, oW;
        for (KeyFrameT* c : pKF->GetConnectedKeyFrames()) {
            wKf.push_back((int32_t)c->mnId);
            wW.push_back((int32_t)pKF->GetWeight(c));
        }
        for (KeyFrameT* c : pKF->GetVectorCovisibleKeyFrames()) {
            oKf.push_back((int32_t)c->mnId);
            oW.push_back((int32_t)pKF->GetWeight(c));
        }
        const int32_t wOff[2] = {0, (int32_t)wKf.size()}, oOff[2] = {0, (int32_t)oKf.size()};
        drfe_lmap_connections c = {};
        c.count = 1;
        c.handle = &handle; c.first_connection = &first; c.weight_offsets = wOff; c.weight_kfs = wKf.data(); c.weight_w = wW.data();
        c.ordered_offsets = oOff; c.ordered_kfs = oKf.data(); c.ordered_w = oW.data();
        Check(drfe_lmap_set_connections(mDb, &c), "drfe_lmap_set_connections");
    }
    void UpdateConnections(KeyFrameT* pKF) { UpdateConnections(std::vector<KeyFrameT*>(1, pKF)); }
    /* the calls of the reference one after another in this order, in one call of the store: the two loops of
     * LoopClosing::CorrectLoop.  Each key frame once.  The named key frames' rows and connection state are synced first; every key
     * frame an edge lands on must be in the store with its current state (SyncConnections; it is current when its connections
     * were last written by this function).  Returns per named key frame what GetConnectedKeyFrames() gives right after its own call. */
    std::vector<std::set<KeyFrameT*>> UpdateConnections(const std::vector<KeyFrameT*>& vpKFs)
    {
        const size_t n = vpKFs.size();
        std::vector<int32_t> handles(n);
        for (size_t k = 0; k < n; k++) {
            Sync(vpKFs[k]);
            SyncConnections(vpKFs[k]);
            handles[k] = (int32_t)vpKFs[k]->mnId;
        }
        std::unique_lock<std::mutex> lock(mMutex);
        int32_t size[3] = {0, 0, 0};
        Check(drfe_lmap_size(mDb, size), "drfe_lmap_size");
        const size_t nK = (size_t)size[0];
        std::vector<int32_t> cOff(n + 1), cKf(n * nK + 1), cVotes(n * nK + 1), rec(4 * n + 1), newParent(n + 1), touched(nK + 1), parent(nK + 1);
        std::vector<int32_t> rwOff(nK + 2), roOff(nK + 2), rwKf, rwW, roKf, roW;
        std::vector<uint8_t> rFirst(nK + 1), flags(nK + 1);
        int32_t nTouched = 0;
        /* a touched row has at most nK - 1 entries, but nK rows of them are rarely needed: grow until the call fits (a call that
         * does not fit changes nothing) */
        for (size_t cap = 64 * (n + 16) + 1024;; cap *= 4) {
            rwKf.resize(cap); rwW.resize(cap); roKf.resize(cap); roW.resize(cap);
            drfe_lmap_connect_out o = {};
            o.counter_capacity = (int32_t)(n * nK); o.touched_capacity = (int32_t)nK;
            o.counter_offsets = cOff.data(); o.counter_kfs = cKf.data(); o.counter_votes = cVotes.data(); o.record = rec.data();
            o.new_parent = newParent.data(); o.n_touched = &nTouched; o.touched = touched.data(); o.flags = flags.data();
            o.rows.weights_capacity = o.rows.ordered_capacity = (int32_t)cap;
            o.rows.weight_offsets = rwOff.data(); o.rows.weight_kfs = rwKf.data(); o.rows.weight_w = rwW.data();
            o.rows.ordered_offsets = roOff.data(); o.rows.ordered_kfs = roKf.data(); o.rows.ordered_w = roW.data();
            o.rows.parent = parent.data(); o.rows.first_connection = rFirst.data();
            const int rc = mForce < 0 ? drfe_lmap_connect_host(mDb, (int32_t)n, handles.data(), &o)
                         : mForce > 0 ? drfe_lmap_connect_device(mDb, (int32_t)n, handles.data(), &o, nullptr)
                                      : drfe_lmap_connect_batch(mDb, (int32_t)n, handles.data(), &o, nullptr);
            if (rc == DRFE_ERR_CAPACITY && cap < nK * nK) continue;      /* nK x nK always suffices: what remains is the scratch budget */
            Check(rc, "drfe_lmap_connect");
            break;
        }
        for (int32_t t = 0; t < nTouched; t++) {
            KeyFrameT* pKF = mKFs.at(touched[(size_t)t]);
            std::map<KeyFrameT*, int> weights;
            std::vector<KeyFrameT*> ordered;
            std::vector<int> orderedWeights;
            for (int32_t i = rwOff[(size_t)t]; i < rwOff[(size_t)t + 1]; i++) weights[mKFs.at(rwKf[(size_t)i])] = rwW[(size_t)i];
            for (int32_t i = roOff[(size_t)t]; i < roOff[(size_t)t + 1]; i++) {
                ordered.push_back(mKFs.at(roKf[(size_t)i]));
                orderedWeights.push_back(roW[(size_t)i]);
            }
            pKF->SetConnections(weights, ordered, orderedWeights, parent[(size_t)t] >= 0 ? mKFs.at(parent[(size_t)t]) : nullptr, rFirst[(size_t)t] != 0);
        }
        std::vector<std::set<KeyFrameT*>> connected(n);
        for (size_t k = 0; k < n; k++) {
            if (newParent[k] >= 0) mKFs.at(newParent[k])->AddChild(vpKFs[k]);
            for (int32_t i = cOff[k]; i < cOff[k + 1]; i++) connected[k].insert(mKFs.at(cKf[(size_t)i]));
        }
        return connected;
    }

    /* The Sim3 propagation of LoopClosing::CorrectLoop (src/LoopClosing.cc:480-562) on the store.  Further
     * accessors of KeyFrameT: GetPose() (4x4 float), SetPose(Mat), mvKeysUn (.octave), mvScaleFactors, mnScaleLevels; of MapPointT:
     * GetWorldPos() (3x1 float), SetWorldPos(Mat), GetReferenceKeyFrame(), the public mnCorrectedByKF / mnCorrectedReference, and
     * one setter that the integrator adds because mNormalVector, mfMaxDistance and mfMinDistance are protected (INTEGRATION.md
     * section 4p): SetNormalAndDepth(const float normal[3], float maxDistance, float minDistance).  Sim3T as for Sim3OptBatch:
     * default-constructible, rotation() with x() y() z() w(), translation() with operator[], scale(), each writable. */
    /* the pose SetPose last received, and the store's mvScaleFactors from this key frame */
    void SyncGeometry(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pKF->mnId;
        float T[16];
        const auto Tcw = pKF->GetPose();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) T[r * 4 + c] = Tcw.template ptr<float>(r)[c];
        Check(drfe_lmap_set_poses(mDb, 1, &handle, T), "drfe_lmap_set_poses");
        const std::vector<float> sf(pKF->mvScaleFactors.begin(), pKF->mvScaleFactors.begin() + pKF->mnScaleLevels);
        Check(drfe_lmap_set_scales(mDb, (int32_t)sf.size(), sf.data()), "drfe_lmap_set_scales");
    }
    /* position, reference key frame with the octave of its key point (key point 0 when it does not observe the point) and stamps */
    void SyncGeometry(MapPointT* pMP)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pMP->mnId;
        float X[3];
        const auto P = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) X[k] = P.template ptr<float>(k)[0];
        KeyFrameT* pRef = pMP->GetReferenceKeyFrame();
        const auto observations = pMP->GetObservations();
        const auto f = observations.find(pRef);
        const int32_t ref = (int32_t)pRef->mnId;
        const int32_t level = pRef->mvKeysUn.empty() ? 0 : (int32_t)pRef->mvKeysUn[f == observations.end() ? (size_t)0 : (size_t)f->second].octave;
        const int32_t by = (int32_t)pMP->mnCorrectedByKF, byRef = (int32_t)pMP->mnCorrectedReference;
        drfe_lmap_point_geometry g = {};
        g.count = 1;
        g.handle = &handle; g.world = X; g.ref_kf = &ref; g.ref_level = &level; g.corrected_by = &by; g.corrected_ref = &byRef;
        Check(drfe_lmap_set_point_geometry(mDb, &g), "drfe_lmap_set_point_geometry");
    }
    /* Lines :480-562 for mpCurrentKF = pCurKF, mg2oScw = g2oScw and mvpCurrentConnectedKFs = vpConnected (pCurKF among them),
     * without the UpdateConnections calls of its loop: call UpdateConnections(inRankOrder) afterwards, where inRankOrder is the
     * returned maps' iteration order.  The store must hold the current rows and geometry of the connected key frames, of the
     * points in their match rows and of those points' observers (Sync, SyncGeometry).  Writes poses, positions, stamps, normals
     * and distances into the caller's objects and returns CorrectedSim3 and NonCorrectedSim3. */
    template <class Sim3T>
    std::pair<std::map<KeyFrameT*, Sim3T>, std::map<KeyFrameT*, Sim3T>> CorrectLoop(KeyFrameT* pCurKF, const Sim3T& g2oScw,
                                                                                     const std::vector<KeyFrameT*>& vpConnected)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const size_t n = vpConnected.size();
        std::vector<int32_t> handles(n);
        size_t cap = 1;
        for (size_t k = 0; k < n; k++) {
            handles[k] = (int32_t)vpConnected[k]->mnId;
            cap += vpConnected[k]->GetMapPointMatches().size();
        }
        const auto& q = g2oScw.rotation();
        const double Scw[8] = {q.x(), q.y(), q.z(), q.w(), g2oScw.translation()[0], g2oScw.translation()[1], g2oScw.translation()[2],
                               g2oScw.scale()};
        std::vector<int32_t> walk(n + 1), points(cap), by(cap);
        std::vector<double> corrected(8 * n + 8), nonCorrected(8 * n + 8);
        std::vector<float> Tiw(16 * n + 16), world(3 * cap), normal(3 * cap), maxD(cap), minD(cap);
        std::vector<uint8_t> status(cap);
        int32_t nPoints = 0;
        drfe_lmap_correct_out o = {};
        o.points_capacity = (int32_t)cap;
        o.walk_pos = walk.data(); o.corrected = corrected.data(); o.non_corrected = nonCorrected.data(); o.Tiw = Tiw.data();
        o.n_points = &nPoints; o.points = points.data(); o.claimed_by = by.data(); o.world = world.data(); o.normal = normal.data();
        o.max_distance = maxD.data(); o.min_distance = minD.data(); o.status = status.data();
        const int32_t cur = (int32_t)pCurKF->mnId;
        Check(mForce < 0 ? drfe_lmap_correct_host(mDb, cur, Scw, (int32_t)n, handles.data(), &o)
            : mForce > 0 ? drfe_lmap_correct_device(mDb, cur, Scw, (int32_t)n, handles.data(), &o, nullptr)
                         : drfe_lmap_correct_batch(mDb, cur, Scw, (int32_t)n, handles.data(), &o, nullptr), "drfe_lmap_correct");
        using ::drfe::drfe_detail_sim3::mat32;
        for (int32_t t = 0; t < nPoints; t++) {
            MapPointT* pMP = mMPs.at(points[(size_t)t]);
            pMP->SetWorldPos(mat32(3, 1, &world[3 * (size_t)t]));
            pMP->mnCorrectedByKF = pCurKF->mnId;
            pMP->mnCorrectedReference = mKFs.at(by[(size_t)t])->mnId;
            if (status[(size_t)t] & DRFE_UPKEEP_NORMAL) pMP->SetNormalAndDepth(&normal[3 * (size_t)t], maxD[(size_t)t], minD[(size_t)t]);
        }
        std::pair<std::map<KeyFrameT*, Sim3T>, std::map<KeyFrameT*, Sim3T>> sims;
        auto fill = [](Sim3T& S, const double* v) {
            auto& r = S.rotation();
            r.x() = v[0]; r.y() = v[1]; r.z() = v[2]; r.w() = v[3];
            for (int k = 0; k < 3; k++) S.translation()[k] = v[4 + k];
            S.scale() = v[7];
        };
        for (size_t k = 0; k < n; k++) {
            fill(sims.first[vpConnected[k]], &corrected[8 * k]);
            fill(sims.second[vpConnected[k]], &nonCorrected[8 * k]);
            vpConnected[k]->SetPose(mat32(4, 4, &Tiw[16 * k]));
        }
        return sims;
    }

    /* The map update that ends LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:722-783) on the store (DESIGN.md section
     * 29).  Further accessors: the public mTcwGBA, mTcwBefGBA and mnBAGlobalForKF of KeyFrameT, mPosGBA and mnBAGlobalForKF of
     * MapPointT.  Call SyncGlobalBA for what Optimizer::BundleAdjustment's write-back touched (an empty mTcwGBA / mPosGBA is not
     * sent: the item then has no state, as a key frame or point made while the adjustment ran). */
    void SyncGlobalBA(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (pKF->mTcwGBA.empty()) return;
        const int32_t handle = (int32_t)pKF->mnId, stamp = (int32_t)pKF->mnBAGlobalForKF;
        float T[16];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) T[r * 4 + c] = pKF->mTcwGBA.template ptr<float>(r)[c];
        Check(drfe_lmap_set_gba_keyframes(mDb, 1, &handle, T, &stamp), "drfe_lmap_set_gba_keyframes");
    }
    void SyncGlobalBA(MapPointT* pMP)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (pMP->mPosGBA.empty()) return;
        const int32_t handle = (int32_t)pMP->mnId, stamp = (int32_t)pMP->mnBAGlobalForKF;
        float X[3];
        for (int k = 0; k < 3; k++) X[k] = pMP->mPosGBA.template ptr<float>(k)[0];
        Check(drfe_lmap_set_gba_points(mDb, 1, &handle, X, &stamp), "drfe_lmap_set_gba_points");
    }
    /* Lines :722-783 for nLoopKF and mpMap->mvpKeyFrameOrigins = vpOrigins.  The store must hold the current rows and geometry of
     * every key frame and map point of the map (Sync, SyncGeometry) and the adjustment's results (SyncGlobalBA).  Writes mTcwGBA,
     * mTcwBefGBA, mnBAGlobalForKF and SetPose into the visited key frames in the order of the reference's FIFO and SetWorldPos
     * into the moved points; returns the visited key frames in that order. */
    std::vector<KeyFrameT*> PropagateGlobalBA(unsigned long nLoopKF, const std::vector<KeyFrameT*>& vpOrigins)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<int32_t> origins;
        for (KeyFrameT* pKF : vpOrigins) origins.push_back((int32_t)pKF->mnId);
        int32_t size[3] = {0, 0, 0};
        Check(drfe_lmap_size(mDb, size), "drfe_lmap_size");
        const size_t capK = (size_t)size[0] + 1, capP = (size_t)size[1] + 1;
        std::vector<int32_t> kfs(capK), points(capP);
        std::vector<float> Tcw(16 * capK), bef(16 * capK), world(3 * capP);
        std::vector<uint8_t> composed(capK), kind(capP);
        int32_t nKfs = 0, nPoints = 0;
        drfe_lmap_gba_out o = {};
        o.keyframes_capacity = (int32_t)capK; o.points_capacity = (int32_t)capP;
        o.n_keyframes = &nKfs; o.keyframes = kfs.data(); o.Tcw = Tcw.data(); o.TcwBef = bef.data(); o.composed = composed.data();
        o.n_points = &nPoints; o.points = points.data(); o.world = world.data(); o.kind = kind.data();
        const int32_t loop = (int32_t)nLoopKF;
        Check(mForce < 0 ? drfe_lmap_gba_host(mDb, loop, (int32_t)origins.size(), origins.data(), &o)
            : mForce > 0 ? drfe_lmap_gba_device(mDb, loop, (int32_t)origins.size(), origins.data(), &o, nullptr)
                         : drfe_lmap_gba_batch(mDb, loop, (int32_t)origins.size(), origins.data(), &o, nullptr), "drfe_lmap_gba");
        using ::drfe::drfe_detail_sim3::mat32;
        std::vector<KeyFrameT*> visited;
        for (int32_t v = 0; v < nKfs; v++) {
            KeyFrameT* pKF = mKFs.at(kfs[(size_t)v]);
            if (composed[(size_t)v]) {
                pKF->mTcwGBA = mat32(4, 4, &Tcw[16 * (size_t)v]);
                pKF->mnBAGlobalForKF = nLoopKF;
            }
            pKF->mTcwBefGBA = mat32(4, 4, &bef[16 * (size_t)v]);
            pKF->SetPose(mat32(4, 4, &Tcw[16 * (size_t)v]));
            visited.push_back(pKF);
        }
        for (int32_t t = 0; t < nPoints; t++) mMPs.at(points[(size_t)t])->SetWorldPos(mat32(3, 1, &world[3 * (size_t)t]));
        return visited;
    }

    /* What surrounds the solver of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2910-3131) on the store (DESIGN.md section
     * 35).  Further accessor of KeyFrameT: GetLoopEdges().  Sim3T as for CorrectLoop. */
    /* mspLoopEdges of pKF into the store: call it after AddLoopEdge */
    void SyncLoopEdges(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pKF->mnId;
        std::vector<int32_t> edges;
        for (KeyFrameT* l : pKF->GetLoopEdges()) edges.push_back((int32_t)l->mnId);
        const int32_t off[2] = {0, (int32_t)edges.size()};
        Check(drfe_lmap_set_loop_edges(mDb, 1, &handle, off, edges.data()), "drfe_lmap_set_loop_edges");
    }
    /* the vertices in rank order and the edges in the order of the reference's addEdge: what the caller's solver is given */
    template <class Sim3T>
    struct EssentialGraph {
        struct Vertex { KeyFrameT* pKF; Sim3T Scw; bool fixed; };
        struct Edge { KeyFrameT* from; KeyFrameT* to; Sim3T Sji; int kind; };
        std::vector<Vertex> vertices;
        std::vector<Edge> edges;
    };
    /* Lines :2910-3080.  The store must hold the current rows, connections, loop edges and poses of every key frame of the map
     * (Sync, SyncConnections, SyncLoopEdges, SyncGeometry; they are current after CorrectLoop and UpdateConnections above). */
    template <class Sim3T>
    EssentialGraph<Sim3T> EssentialEdges(KeyFrameT* pLoopKF, KeyFrameT* pCurKF, const std::map<KeyFrameT*, Sim3T>& NonCorrectedSim3,
                                         const std::map<KeyFrameT*, Sim3T>& CorrectedSim3,
                                         const std::map<KeyFrameT*, std::set<KeyFrameT*>>& LoopConnections)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        auto put = [](const Sim3T& S, double* v) {
            const auto& q = S.rotation();
            v[0] = q.x(); v[1] = q.y(); v[2] = q.z(); v[3] = q.w();
            for (int k = 0; k < 3; k++) v[4 + k] = S.translation()[k];
            v[7] = S.scale();
        };
        auto fill = [](Sim3T& S, const double* v) {
            auto& r = S.rotation();
            r.x() = v[0]; r.y() = v[1]; r.z() = v[2]; r.w() = v[3];
            for (int k = 0; k < 3; k++) S.translation()[k] = v[4 + k];
            S.scale() = v[7];
        };
        std::vector<int32_t> tab, lcH, lcOff(1, 0), lcKf;
        std::vector<double> co, nc;
        for (const auto& e : CorrectedSim3) {
            const auto n = NonCorrectedSim3.find(e.first);
            tab.push_back((int32_t)e.first->mnId);
            co.resize(co.size() + 8);
            nc.resize(nc.size() + 8);
            put(e.second, &co[co.size() - 8]);
            put(n == NonCorrectedSim3.end() ? e.second : n->second, &nc[nc.size() - 8]);
        }
        for (const auto& e : LoopConnections) {
            lcH.push_back((int32_t)e.first->mnId);
            for (KeyFrameT* m : e.second) lcKf.push_back((int32_t)m->mnId);
            lcOff.push_back((int32_t)lcKf.size());
        }
        int64_t need[6] = {0, 0, 0, 0, 0, 0};
        int32_t size[3] = {0, 0, 0};
        Check(drfe_lmap_size(mDb, size), "drfe_lmap_size");
        Check(drfe_lmap_essential_scratch(mDb, (int32_t)lcKf.size(), need), "drfe_lmap_essential_scratch");
        const size_t capV = (size_t)size[0] + 1, capE = (size_t)need[5] + 1;
        std::vector<int32_t> vert(capV), from(capE), to(capE);
        std::vector<double> scw(8 * capV), meas(8 * capE);
        std::vector<uint8_t> fixed(capV), kind(capE);
        int32_t nV = 0, nE = 0;
        drfe_lmap_essential_edges_call c = {};
        c.loop_kf = (int32_t)pLoopKF->mnId; c.cur_kf = (int32_t)pCurKF->mnId;
        c.n_sim3 = (int32_t)tab.size(); c.n_lc = (int32_t)lcH.size();
        c.sim3_handles = tab.data(); c.corrected = co.data(); c.non_corrected = nc.data();
        c.lc_handles = lcH.data(); c.lc_offsets = lcOff.data(); c.lc_kfs = lcKf.data();
        c.vertices_capacity = (int32_t)capV; c.edges_capacity = (int32_t)capE;
        c.n_vertices = &nV; c.vertices = vert.data(); c.Scw = scw.data(); c.fixed = fixed.data();
        c.n_edges = &nE; c.from = from.data(); c.to = to.data(); c.measurement = meas.data(); c.kind = kind.data();
        Check(mForce < 0 ? drfe_lmap_essential_edges_host(mDb, &c)
            : mForce > 0 ? drfe_lmap_essential_edges_device(mDb, &c, nullptr) : drfe_lmap_essential_edges_batch(mDb, &c, nullptr),
              "drfe_lmap_essential_edges");
        EssentialGraph<Sim3T> G;
        G.vertices.resize((size_t)nV);
        G.edges.resize((size_t)nE);
        for (int32_t v = 0; v < nV; v++) {
            G.vertices[(size_t)v].pKF = mKFs.at(vert[(size_t)v]);
            fill(G.vertices[(size_t)v].Scw, &scw[8 * (size_t)v]);
            G.vertices[(size_t)v].fixed = fixed[(size_t)v] != 0;
        }
        for (int32_t e = 0; e < nE; e++) {
            G.edges[(size_t)e].from = mKFs.at(from[(size_t)e]);
            G.edges[(size_t)e].to = mKFs.at(to[(size_t)e]);
            fill(G.edges[(size_t)e].Sji, &meas[8 * (size_t)e]);
            G.edges[(size_t)e].kind = kind[(size_t)e];
        }
        return G;
    }
    /* Lines :3088-3131 for the graph EssentialEdges returned and the solver's estimates, one per vertex in the graph's order.
     * The store must hold the current geometry of every map point (SyncGeometry).  Writes SetPose into every key frame in the
     * graph's order, then SetWorldPos and the normal and distances into every moved point in ascending mnId (the reference walks
     * set<MapPoint*>; no point reads another).  Map lines and planes stay with the caller: the returned vCorrectedSwc, with the
     * graph's Scw, is what :3134-3204 read. */
    template <class Sim3T>
    std::map<KeyFrameT*, Sim3T> EssentialCommit(KeyFrameT* pCurKF, const EssentialGraph<Sim3T>& G, const std::vector<Sim3T>& optimised)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const size_t n = G.vertices.size();
        if (optimised.size() != n) throw std::runtime_error("EssentialCommit: one estimate per vertex");
        std::vector<int32_t> handles(n);
        std::vector<double> scw(8 * n + 8), opt(8 * n + 8), swc(8 * n + 8);
        auto put = [](const Sim3T& S, double* v) {
            const auto& q = S.rotation();
            v[0] = q.x(); v[1] = q.y(); v[2] = q.z(); v[3] = q.w();
            for (int k = 0; k < 3; k++) v[4 + k] = S.translation()[k];
            v[7] = S.scale();
        };
        for (size_t v = 0; v < n; v++) {
            handles[v] = (int32_t)G.vertices[v].pKF->mnId;
            put(G.vertices[v].Scw, &scw[8 * v]);
            put(optimised[v], &opt[8 * v]);
        }
        int32_t size[3] = {0, 0, 0};
        Check(drfe_lmap_size(mDb, size), "drfe_lmap_size");
        const size_t cap = (size_t)size[1] + 1;
        std::vector<int32_t> points(cap), ref(cap);
        std::vector<float> Tiw(16 * n + 16), world(3 * cap), normal(3 * cap), maxD(cap), minD(cap);
        std::vector<uint8_t> status(cap);
        int32_t nPoints = 0;
        drfe_lmap_essential_commit_call c = {};
        c.cur_kf = (int32_t)pCurKF->mnId; c.n = (int32_t)n;
        c.handles = handles.data(); c.Scw = scw.data(); c.optimised = opt.data();
        c.points_capacity = (int32_t)cap;
        c.Tiw = Tiw.data(); c.Swc = swc.data(); c.n_points = &nPoints; c.points = points.data(); c.ref = ref.data();
        c.world = world.data(); c.normal = normal.data(); c.max_distance = maxD.data(); c.min_distance = minD.data(); c.status = status.data();
        Check(mForce < 0 ? drfe_lmap_essential_commit_host(mDb, &c)
            : mForce > 0 ? drfe_lmap_essential_commit_device(mDb, &c, nullptr) : drfe_lmap_essential_commit_batch(mDb, &c, nullptr),
              "drfe_lmap_essential_commit");
        using ::drfe::drfe_detail_sim3::mat32;
        std::map<KeyFrameT*, Sim3T> vCorrectedSwc;
        for (size_t v = 0; v < n; v++) {
            KeyFrameT* pKF = G.vertices[v].pKF;
            Sim3T& S = vCorrectedSwc[pKF];
            auto& r = S.rotation();
            const double* w = &swc[8 * v];
            r.x() = w[0]; r.y() = w[1]; r.z() = w[2]; r.w() = w[3];
            for (int k = 0; k < 3; k++) S.translation()[k] = w[4 + k];
            S.scale() = w[7];
            pKF->SetPose(mat32(4, 4, &Tiw[16 * v]));
        }
        for (int32_t t = 0; t < nPoints; t++) {
            MapPointT* pMP = mMPs.at(points[(size_t)t]);
            pMP->SetWorldPos(mat32(3, 1, &world[3 * (size_t)t]));
            if (status[(size_t)t] & DRFE_UPKEEP_NORMAL) pMP->SetNormalAndDepth(&normal[3 * (size_t)t], maxD[(size_t)t], minD[(size_t)t]);
        }
        return vCorrectedSwc;
    }

    /* LocalMapping::KeyFrameCulling (src/LocalMapping.cc:1226-1285) with KeyFrame::SetBadFlag on the store.
     * Further accessors of KeyFrameT: the public mThDepth, mvKeysUn (.octave), mvDepth, mvuRight and mbNewPlane, SetBadFlag(), and
     * two getters that the integrator adds because mbNotErase and mbToBeErased are protected:
     * GetNotErase() and GetToBeErased(); of MapPointT: Observations() and GetObservations(). */
    /* what the walk reads of pKF: mThDepth, the flags, and octave, depth and stereo of every entry of its match row.  Call it
     * with Sync(pKF): the arrays have to fit the row the store holds. */
    void SyncCulling(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pKF->mnId;
        const float th = (float)pKF->mThDepth;
        const uint8_t flags = (uint8_t)((pKF->GetNotErase() ? 1 : 0) | (pKF->mnId == 0 ? 2 : 0) | (pKF->GetToBeErased() ? 4 : 0));
        const size_t n = pKF->GetMapPointMatches().size();
        std::vector<int32_t> octave(n);
        std::vector<float> depth(n);
        std::vector<uint8_t> stereo(n);
        for (size_t i = 0; i < n; i++) {
            octave[i] = (int32_t)pKF->mvKeysUn[i].octave;
            depth[i] = (float)pKF->mvDepth[i];
            stereo[i] = pKF->mvuRight[i] >= 0 ? 1 : 0;
        }
        const int32_t off[2] = {0, (int32_t)n};
        drfe_lmap_cull_attributes a = {};
        a.n_kfs = 1;
        a.kf_handle = &handle; a.th_depth = &th; a.kf_flags = &flags; a.row_offsets = off;
        a.octave = octave.data(); a.depth = depth.data(); a.stereo = stereo.data();
        Check(drfe_lmap_set_cull_attributes(mDb, &a), "drfe_lmap_set_cull_attributes");
    }
    /* nObs and mit->second of every observation of pMP, in the order Sync(pMP) sends the observations */
    void SyncCulling(MapPointT* pMP)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pMP->mnId;
        const int32_t nObs = (int32_t)pMP->Observations();
        std::vector<int32_t> idx;
        for (const auto& o : pMP->GetObservations()) idx.push_back((int32_t)o.second);
        const int32_t off[2] = {0, (int32_t)idx.size()};
        drfe_lmap_cull_attributes a = {};
        a.n_points = 1;
        a.point_handle = &handle; a.n_obs = &nObs; a.obs_offsets = off; a.obs_index = idx.data();
        Check(drfe_lmap_set_cull_attributes(mDb, &a), "drfe_lmap_set_cull_attributes");
    }
    /* KeyFrameCulling() for mpCurrentKeyFrame = pCurrentKF and mbMonocular = bMonocular.  The store must hold the current rows,
     * connections and culling attributes of the covisible key frames, of the points in their match rows and of those points'
     * observers (Sync, SyncConnections, SyncCulling).  The store decides and takes the culled key frames out of its own graph;
     * then every key frame with a verdict gets its own SetBadFlag() in that order, which does the same to the objects and sees to
     * map lines, planes, the map and the key-frame database (and only sets mbToBeErased where mbNotErase holds).  Returns the
     * culled key frames in order. */
    std::vector<KeyFrameT*> KeyFrameCulling(KeyFrameT* pCurrentKF, bool bMonocular)
    {
        std::vector<KeyFrameT*> culled;
        if (pCurrentKF->mbNewPlane) return culled;
        const std::vector<KeyFrameT*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
        const size_t n = vpLocalKeyFrames.size();
        if (n == 0) return culled;
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<int32_t> handles(n);
        size_t rows = 1;
        for (size_t k = 0; k < n; k++) {
            handles[k] = (int32_t)vpLocalKeyFrames[k]->mnId;
            rows += vpLocalKeyFrames[k]->GetMapPointMatches().size();
        }
        int32_t size[3] = {0, 0, 0};
        Check(drfe_lmap_size(mDb, size), "drfe_lmap_size");
        const size_t nK = (size_t)size[0] + 1;
        std::vector<int32_t> rec(4 * n), culledH(n), touched(nK), parent(nK), rwOff(nK + 1), roOff(nK + 1), chOff(nK + 1), nuOff(nK + 1);
        std::vector<int32_t> rwKf, rwW, roKf, roW, ch, nulled, points, pNObs, pRef, obsOff, obs, obsIdx;
        std::vector<float> Tcp(16 * n);
        std::vector<uint8_t> hasTcp(n), flags(nK), rFirst(nK), pBad;
        int32_t nCulled = 0, nTouched = 0, nPoints = 0;
        /* a call touches at most the points of the called rows; the rows of connections and children grow until the call fits (a
         * call that does not fit changes nothing) */
        for (size_t cap = 64 * (n + 16) + 1024;; cap *= 4) {
            rwKf.resize(cap); rwW.resize(cap); roKf.resize(cap); roW.resize(cap); ch.resize(cap); nulled.resize(cap * 4);
            points.resize(rows); pNObs.resize(rows); pRef.resize(rows); pBad.resize(rows); obsOff.resize(rows + 1);
            obs.resize(cap * 16); obsIdx.resize(cap * 16);
            drfe_lmap_cull_out o = {};
            o.touched_capacity = (int32_t)nK; o.children_capacity = (int32_t)cap; o.nulled_capacity = (int32_t)(cap * 4);
            o.points_capacity = (int32_t)rows; o.obs_capacity = (int32_t)(cap * 16);
            o.record = rec.data(); o.Tcp = Tcp.data(); o.has_Tcp = hasTcp.data(); o.n_culled = &nCulled; o.culled = culledH.data();
            o.n_touched = &nTouched; o.touched = touched.data(); o.flags = flags.data();
            o.rows.weights_capacity = o.rows.ordered_capacity = (int32_t)cap;
            o.rows.weight_offsets = rwOff.data(); o.rows.weight_kfs = rwKf.data(); o.rows.weight_w = rwW.data();
            o.rows.ordered_offsets = roOff.data(); o.rows.ordered_kfs = roKf.data(); o.rows.ordered_w = roW.data();
            o.rows.parent = parent.data(); o.rows.first_connection = rFirst.data();
            o.children_offsets = chOff.data(); o.children = ch.data(); o.nulled_offsets = nuOff.data(); o.nulled = nulled.data();
            o.n_points = &nPoints; o.points = points.data(); o.point_n_obs = pNObs.data(); o.point_ref = pRef.data();
            o.point_bad = pBad.data(); o.obs_offsets = obsOff.data(); o.obs = obs.data(); o.obs_index = obsIdx.data();
            const int32_t mono = bMonocular ? 1 : 0;
            const int rc = mForce < 0 ? drfe_lmap_cull_host(mDb, (int32_t)n, handles.data(), mono, &o)
                         : mForce > 0 ? drfe_lmap_cull_device(mDb, (int32_t)n, handles.data(), mono, &o, nullptr)
                                      : drfe_lmap_cull_batch(mDb, (int32_t)n, handles.data(), mono, &o, nullptr);
            if (rc == DRFE_ERR_CAPACITY && cap < ((size_t)1 << 26) &&
                std::string(drfe_lmap_last_error(mDb)).find("the call returns more than") != std::string::npos)
                continue;
            Check(rc, "drfe_lmap_cull");
            break;
        }
        lock.unlock();
        for (size_t k = 0; k < n; k++)
            if (rec[4 * k + 2]) vpLocalKeyFrames[k]->SetBadFlag();       /* culled, or deferred by mbNotErase */
        for (int32_t i = 0; i < nCulled; i++) culled.push_back(mKFs.at(culledH[(size_t)i]));
        return culled;
    }
    /* LocalMapping::MapPointCulling and MapLineCulling (src/LocalMapping.cc:175-231) with MapPoint::SetBadFlag and
     * MapLine::SetBadFlag on the store.  Further accessors of MapPointT and MapLineT: GetFound(), the public
     * mnFirstKFid, Observations(), GetObservations() (pairs of KeyFrameT* and index), SetBadFlag(), and one getter that the
     * integrator adds because mnVisible is protected: GetVisible(). */
    /* mnFound, mnVisible and mnFirstKFid of pMP.  Call it with Sync(pMP) and SyncCulling(pMP), which hold its observations. */
    void SyncRecent(MapPointT* pMP)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pMP->mnId, found = (int32_t)pMP->GetFound(), visible = (int32_t)pMP->GetVisible();
        const int64_t first = (int64_t)pMP->mnFirstKFid;
        drfe_lmap_recent_attributes a = {};
        a.n_points = 1;
        a.point_handle = &handle; a.point_found = &found; a.point_visible = &visible; a.point_first_kf = &first;
        Check(drfe_lmap_set_recent_attributes(mDb, &a), "drfe_lmap_set_recent_attributes");
    }
    /* the same of pML, with nObs and its observations in the order of GetObservations().  Call it with Sync(pML). */
    void SyncRecent(MapLineT* pML)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pML->mnId, found = (int32_t)pML->GetFound(), visible = (int32_t)pML->GetVisible();
        const int32_t nObs = (int32_t)pML->Observations();
        const int64_t first = (int64_t)pML->mnFirstKFid;
        std::vector<int32_t> obs, idx;
        for (const auto& o : pML->GetObservations()) {
            obs.push_back((int32_t)o.first->mnId);
            idx.push_back((int32_t)o.second);
        }
        const int32_t off[2] = {0, (int32_t)obs.size()};
        drfe_lmap_recent_attributes a = {};
        a.n_lines = 1;
        a.line_handle = &handle; a.line_found = &found; a.line_visible = &visible; a.line_first_kf = &first; a.line_n_obs = &nObs;
        a.line_obs_offsets = off; a.line_obs = obs.data(); a.line_obs_index = idx.data();
        Check(drfe_lmap_set_recent_attributes(mDb, &a), "drfe_lmap_set_recent_attributes");
    }
    /* after pMP->IncreaseFound(dFound) / IncreaseVisible(dVisible), or pML's: the counters alone travel */
    void Increased(MapPointT* pMP, int dFound, int dVisible) { Increase(DRFE_LMAP_POINT, (int32_t)pMP->mnId, dFound, dVisible); }
    void Increased(MapLineT* pML, int dFound, int dVisible) { Increase(DRFE_LMAP_LINE, (int32_t)pML->mnId, dFound, dVisible); }
    /* MapPointCulling() over mlpRecentAddedMapPoints = recent for mpCurrentKeyFrame = pCurrentKF.  The store must hold the current
     * rows of the listed points that are not bad and of their observers (Sync, SyncCulling, SyncRecent).  The store decides and
     * nulls its own rows; then the list is walked as the reference walks it: an entry with a verdict gets the object's own
     * SetBadFlag(), which does the same to the objects and sees to the map, and every entry but a kept one is erased. */
    void MapPointCulling(std::list<MapPointT*>& recent, KeyFrameT* pCurrentKF, bool bMonocular)
    {
        RecentCulling(recent, (int64_t)pCurrentKF->mnId, bMonocular, DRFE_LMAP_POINT);
    }
    /* MapLineCulling() over mlpRecentAddedMapLines, likewise (Sync, SyncRecent) */
    void MapLineCulling(std::list<MapLineT*>& recent, KeyFrameT* pCurrentKF, bool bMonocular)
    {
        RecentCulling(recent, (int64_t)pCurrentKF->mnId, bMonocular, DRFE_LMAP_LINE);
    }
    /* The fuse commit on the store: the loop that applies a fusion search, with MapPoint::Replace /
     * MapLine::Replace and AddObservation.  bestIdx[i] is the search's answer for candidate i with the bestDist <= TH_LOW gate
     * applied, -1 = none.  Each method runs the store call, then the reference's loop on the caller's objects with the objects'
     * own Replace / AddObservation / AddMapPoint: the objects stay authoritative, and decide the same.  The store must hold the
     * current rows of pKF (Sync, SyncCulling), of the candidates, of the entries of pKF's row they are sent to and of those items'
     * observers (Sync, SyncCulling, SyncRecent).  Further accessors: MapPointT / MapLineT IsInKeyFrame(), Replace(),
     * AddObservation(); KeyFrameT GetMapPoint(), AddMapPoint(), GetMapLine(), AddMapLine(), GetMapPoints().  Returns nFused. */
    /* ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:845-976) */
    int Fuse(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const std::vector<int32_t>& bestIdx)
    {
        FuseStore(pKF, vpMapPoints, bestIdx.data(), DRFE_LMAP_POINT, DRFE_LMAP_FUSE_NEIGHBOURS, nullptr);
        int nFused = 0;
        for (size_t i = 0; i < vpMapPoints.size(); i++) {
            MapPointT* pMP = vpMapPoints[i];
            if (!pMP) continue;
            if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
            if (bestIdx[i] < 0) continue;
            MapPointT* pMPinKF = pKF->GetMapPoint((size_t)bestIdx[i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                    else pMPinKF->Replace(pMP);
                }
            } else {
                pMP->AddObservation(pKF, (size_t)bestIdx[i]);
                pKF->AddMapPoint(pMP, (size_t)bestIdx[i]);
            }
            nFused++;
        }
        return nFused;
    }
    /* LSDmatcher::Fuse(pKF, vpMapLines, th) (src/LSDmatcher.cpp:897-1012) */
    int Fuse(KeyFrameT* pKF, const std::vector<MapLineT*>& vpMapLines, const std::vector<int32_t>& bestIdx)
    {
        FuseStore(pKF, vpMapLines, bestIdx.data(), DRFE_LMAP_LINE, DRFE_LMAP_FUSE_NEIGHBOURS, nullptr);
        int nFused = 0;
        for (size_t i = 0; i < vpMapLines.size(); i++) {
            MapLineT* pML = vpMapLines[i];
            if (!pML || pML->isBad()) continue;        /* the reference does not ask IsInKeyFrame of a line (:1043 is commented out) */
            if (bestIdx[i] < 0) continue;
            MapLineT* pMLinKF = pKF->GetMapLine((size_t)bestIdx[i]);
            if (pMLinKF) {
                if (!pMLinKF->isBad()) {
                    if (pMLinKF->Observations() > pML->Observations()) pML->Replace(pMLinKF);
                    else pMLinKF->Replace(pML);
                }
            } else {
                pML->AddObservation(pKF, (size_t)bestIdx[i]);
                pKF->AddMapLine(pML, (size_t)bestIdx[i]);
            }
            nFused++;
        }
        return nFused;
    }
    /* ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1001-1101) followed by SearchAndFuse's loop
     * (src/LoopClosing.cc:650-657): vpReplacePoint is filled, then every recorded point is replaced by its candidate */
    int FuseLoop(KeyFrameT* pKF, const std::vector<MapPointT*>& vpPoints, const std::vector<int32_t>& bestIdx, std::vector<MapPointT*>& vpReplacePoint)
    {
        std::vector<int32_t> recorded(vpPoints.size(), -1);
        FuseStore(pKF, vpPoints, bestIdx.data(), DRFE_LMAP_POINT, DRFE_LMAP_FUSE_LOOP, recorded.data());
        const std::set<MapPointT*> spAlreadyFound = pKF->GetMapPoints();
        std::vector<uint8_t> skip(vpPoints.size());
        for (size_t i = 0; i < vpPoints.size(); i++) skip[i] = vpPoints[i]->isBad() || spAlreadyFound.count(vpPoints[i]);
        vpReplacePoint.assign(vpPoints.size(), static_cast<MapPointT*>(nullptr));
        int nFused = 0;
        for (size_t i = 0; i < vpPoints.size(); i++) {
            if (skip[i] || bestIdx[i] < 0) continue;
            MapPointT* pMP = vpPoints[i];
            MapPointT* pMPinKF = pKF->GetMapPoint((size_t)bestIdx[i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) vpReplacePoint[i] = pMPinKF;
            } else {
                pMP->AddObservation(pKF, (size_t)bestIdx[i]);
                pKF->AddMapPoint(pMP, (size_t)bestIdx[i]);
            }
            nFused++;
        }
        for (size_t i = 0; i < vpPoints.size(); i++) {
            /* the store recorded the same occupants */
            if ((vpReplacePoint[i] ? (int32_t)vpReplacePoint[i]->mnId : -1) != recorded[i])
                throw std::runtime_error("LocalMapTracker::FuseLoop: the store and the objects disagree: the store was not in sync");
            if (vpReplacePoint[i]) vpReplacePoint[i]->Replace(vpPoints[i]);
        }
        return nFused;
    }
    /* the loop over mvpCurrentMatchedPoints of CorrectLoop (src/LoopClosing.cc:566-581): vpMatched is parallel to pKF's row */
    int FuseMatched(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMatched)
    {
        FuseStore(pKF, vpMatched, nullptr, DRFE_LMAP_POINT, DRFE_LMAP_FUSE_MATCHED, nullptr);
        int nFused = 0;
        for (size_t i = 0; i < vpMatched.size(); i++) {
            if (!vpMatched[i]) continue;
            MapPointT* pLoopMP = vpMatched[i];
            MapPointT* pCurMP = pKF->GetMapPoint(i);
            if (pCurMP) pCurMP->Replace(pLoopMP);
            else {
                pKF->AddMapPoint(pLoopMP, i);
                pLoopMP->AddObservation(pKF, i);
            }
            nFused++;
        }
        return nFused;
    }
    /* The store's half alone, for Planar_SLAM::ORBmatcher::Fuse / LSDmatcher::Fuse, which run the loop on the objects themselves
     * and inform a tracker they are given: one step on the store, nothing on the objects.  recorded: LOOP's replace[] as
     * handles, or nullptr. */
    template <class ItemT>
    void FuseStore(KeyFrameT* pKF, const std::vector<ItemT*>& items, const int32_t* bestIdx, int kind, int form, int32_t* recorded)
    {
        const size_t n = items.size();
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<int32_t> handles(n), rep(n + 1, -1);
        size_t live = 0;
        for (size_t i = 0; i < n; i++) {
            handles[i] = items[i] ? (int32_t)items[i]->mnId : -1;
            live += items[i] != nullptr;
        }
        std::vector<uint8_t> action(n + 1), moved;
        std::vector<int32_t> rkind(live + 1), loser(live + 1), winner(live + 1), off(live + 2), tp(live + 1), tl(live + 1), rkf, ridx;
        int32_t nFused = 0, nReplaced = 0, nTouched[2] = {0, 0};
        /* the records grow until the call fits (a call that does not fit changes nothing) */
        for (size_t cap = 16 * live + 1024;; cap *= 8) {
            rkf.resize(cap);
            ridx.resize(cap);
            moved.resize(cap);
            drfe_lmap_fuse_step s = {};
            s.keyframe = (int32_t)pKF->mnId; s.kind = kind; s.form = form; s.n = (int32_t)n;
            s.candidates = handles.data(); s.best_idx = bestIdx; s.action = action.data(); s.n_fused = &nFused; s.replace = rep.data();
            drfe_lmap_fuse_call c = {};
            c.n_steps = 1; c.steps = &s;
            c.replaced_capacity = (int32_t)live; c.record_capacity = (int32_t)cap; c.touched_capacity = (int32_t)live;
            c.n_replaced = &nReplaced; c.replaced_kind = rkind.data(); c.loser = loser.data(); c.winner = winner.data();
            c.record_offsets = off.data(); c.record_kf = rkf.data(); c.record_index = ridx.data(); c.record_moved = moved.data();
            c.n_touched = nTouched; c.touched_points = tp.data(); c.touched_lines = tl.data();
            const int rc = mForce < 0 ? drfe_lmap_fuse_host(mDb, &c) : mForce > 0 ? drfe_lmap_fuse_device(mDb, &c, nullptr)
                                                                                   : drfe_lmap_fuse_batch(mDb, &c, nullptr);
            if (rc == DRFE_ERR_CAPACITY && cap < ((size_t)1 << 28) && std::string(drfe_lmap_last_error(mDb)).find("record_capacity") != std::string::npos)
                continue;
            Check(rc, "drfe_lmap_fuse");
            break;
        }
        if (recorded) std::copy(rep.begin(), rep.begin() + (ptrdiff_t)n, recorded);
    }
    /* The item loops of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:124-157) on the store for
     * mpCurrentKeyFrame = pKF, or for a queue of new key frames in order.  The store must hold the current rows of the key frames
     * (Sync, SyncCulling), of the items in them (Sync, SyncCulling, SyncRecent) and - with normals - the geometry of those points,
     * of their observers and reference key frames (SyncGeometry).  The store decides and commits; then the rows are walked as the
     * reference walks them: an ADDED entry gets the object's own AddObservation(pKF, i), a RECENT one is pushed onto recentPoints /
     * recentLines.  Returns one record per ADDED point entry in walk order, as MapUpkeep::Points returns them (status
     * DRFE_UPKEEP_NORMAL with the normal and the two distances of its UpdateNormalAndDepth; best_obs and descriptor unset:
     * ComputeDistinctiveDescriptors stays with the upkeep batch); `added`, when given, receives the points of those entries.
     * normals = false skips that part: no geometry is read and every status is 0.  Several key frames in one call: see drfe.h on
     * UpdateConnections between them.  Further accessors: MapPointT / MapLineT IsInKeyFrame(), AddObservation(). */
    std::vector<drfe::MapPointUpkeep> ProcessNewKeyFrame(KeyFrameT* pKF, std::list<MapPointT*>& recentPoints, std::list<MapLineT*>& recentLines,
                                                   bool normals = true, std::vector<MapPointT*>* added = nullptr)
    {
        return ProcessNewKeyFrame(std::vector<KeyFrameT*>(1, pKF), recentPoints, recentLines, normals, added);
    }
    std::vector<drfe::MapPointUpkeep> ProcessNewKeyFrame(const std::vector<KeyFrameT*>& vpKFs, std::list<MapPointT*>& recentPoints,
                                                   std::list<MapLineT*>& recentLines, bool normals = true, std::vector<MapPointT*>* added = nullptr)
    {
        const size_t n = vpKFs.size();
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<int32_t> handles(n);
        size_t rows[2] = {0, 0};
        for (size_t j = 0; j < n; j++) {
            handles[j] = (int32_t)vpKFs[j]->mnId;
            rows[0] += vpKFs[j]->GetMapPointMatches().size();
            rows[1] += vpKFs[j]->GetMapLineMatches().size();
        }
        std::vector<int32_t> pOff(n + 1), lOff(n + 1), ap(rows[0] + 1), apKf(rows[0] + 1), apIdx(rows[0] + 1), al(rows[1] + 1), alKf(rows[1] + 1),
            alIdx(rows[1] + 1), rp(rows[0] + 1), rl(rows[1] + 1);
        std::vector<uint8_t> pAct(rows[0] + 1), lAct(rows[1] + 1), status(rows[0] + 1);
        std::vector<float> nrm(3 * (rows[0] + 1)), maxD(rows[0] + 1), minD(rows[0] + 1);
        int32_t nAdded[2] = {0, 0}, nRecent[2] = {0, 0};
        drfe_lmap_insert_call c = {};
        c.n = (int32_t)n; c.handles = handles.data();
        for (int k = 0; k < 2; k++) c.action_capacity[k] = c.added_capacity[k] = c.recent_capacity[k] = (int32_t)rows[k];
        c.point_offsets = pOff.data(); c.point_action = pAct.data(); c.line_offsets = lOff.data(); c.line_action = lAct.data();
        c.n_added = nAdded; c.added_points = ap.data(); c.added_point_kf = apKf.data(); c.added_point_index = apIdx.data();
        c.normal = normals ? nrm.data() : nullptr; c.max_distance = maxD.data(); c.min_distance = minD.data(); c.status = status.data();
        c.added_lines = al.data(); c.added_line_kf = alKf.data(); c.added_line_index = alIdx.data();
        c.n_recent = nRecent; c.recent_points = rp.data(); c.recent_lines = rl.data();
        Check(mForce < 0 ? drfe_lmap_insert_host(mDb, &c) : mForce > 0 ? drfe_lmap_insert_device(mDb, &c, nullptr) : drfe_lmap_insert_batch(mDb, &c, nullptr),
              "drfe_lmap_insert");
        lock.unlock();
        std::vector<drfe::MapPointUpkeep> records((size_t)nAdded[0]);
        for (size_t t = 0; t < records.size(); t++) {
            drfe::MapPointUpkeep& u = records[t];
            if (!normals) continue;
            u.status = status[t];
            for (int k = 0; k < 3; k++) u.normal[k] = nrm[3 * t + (size_t)k];
            u.max_distance = maxD[t];
            u.min_distance = minD[t];
        }
        if (added) added->clear();
        /* the reference's loops on the objects, which decide the same */
        auto disagree = []() { return std::runtime_error("LocalMapTracker::ProcessNewKeyFrame: the store and the objects disagree: the store was not in sync"); };
        for (size_t j = 0; j < n; j++) {
            KeyFrameT* pKF = vpKFs[j];
            const std::vector<MapPointT*> vpMapPointMatches = pKF->GetMapPointMatches();
            for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
                MapPointT* pMP = vpMapPointMatches[i];
                const uint8_t a = pAct[(size_t)pOff[j] + i];
                const bool live = pMP && !pMP->isBad();
                if (live != (a == DRFE_LMAP_INSERT_ADDED || a == DRFE_LMAP_INSERT_RECENT)) throw disagree();
                if (!live) continue;
                if (!pMP->IsInKeyFrame(pKF)) {
                    if (a != DRFE_LMAP_INSERT_ADDED) throw disagree();
                    pMP->AddObservation(pKF, i);
                    if (added) added->push_back(pMP);
                } else {
                    if (a != DRFE_LMAP_INSERT_RECENT) throw disagree();
                    recentPoints.push_back(pMP);
                }
            }
            const std::vector<MapLineT*> vpMapLineMatches = pKF->GetMapLineMatches();
            for (size_t i = 0; i < vpMapLineMatches.size(); i++) {
                MapLineT* pML = vpMapLineMatches[i];
                const uint8_t a = lAct[(size_t)lOff[j] + i];
                const bool live = pML && !pML->isBad();
                if (live != (a == DRFE_LMAP_INSERT_ADDED || a == DRFE_LMAP_INSERT_RECENT)) throw disagree();
                if (!live) continue;
                if (!pML->IsInKeyFrame(pKF)) {
                    if (a != DRFE_LMAP_INSERT_ADDED) throw disagree();
                    pML->AddObservation(pKF, i);
                } else {
                    if (a != DRFE_LMAP_INSERT_RECENT) throw disagree();
                    recentLines.push_back(pML);
                }
            }
        }
        return records;
    }
    /* The tail of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:522-535) on the store for the
     * already constructed points vpMPs[t] = new MapPoint(x3D, pRefKF, mpMap): point t is observed by kf1[t] at idx1[t] and by
     * kf2[t] at idx2[t], in that order, as the reference calls AddObservation; pRefKF is the key frame it was constructed with
     * (mpCurrentKeyFrame; the first key frame in CreateInitialMapMonocular, where it stands second).  world[t] is x3D as 3 floats.
     * The store must hold the current rows and culling attributes of the named key frames (Sync, SyncCulling) and - with normals
     * - their poses and the scales (SyncGeometry).  The store creates and commits; then every object gets what the reference
     * gives it: AddObservation, AddMapPoint on both key frames, and the tracker learns the object (as Sync does).  Returns one
     * record per point in order, as ProcessNewKeyFrame returns them (status DRFE_UPKEEP_NORMAL with the normal and the two
     * distances of its UpdateNormalAndDepth: assign them the way the upkeep batch's are assigned; best_obs and descriptor unset:
     * ComputeDistinctiveDescriptors stays with the upkeep batch).  Map::AddMapPoint and the push onto mlpRecentAddedMapPoints
     * stay with the caller.  Further accessors: MapPointT mnFirstKFid; KeyFrameT AddMapPoint(MapPointT*, size_t). */
    std::vector<drfe::MapPointUpkeep> CreateMapPoints(const std::vector<MapPointT*>& vpMPs, const std::vector<KeyFrameT*>& kf1,
                                                      const std::vector<size_t>& idx1, const std::vector<KeyFrameT*>& kf2,
                                                      const std::vector<size_t>& idx2, KeyFrameT* pRefKF, const float* world, bool normals = true)
    {
        return CreatePoints(vpMPs, kf1, idx1, &kf2, &idx2, pRefKF, world, normals);
    }
    /* the single-observer form: CreateNewKeyFrame's two loops and StereoInitialization (src/Tracking.cc:3097-3103, :3145-3150,
     * :1579-1589), every point observed by pKF alone, at idx[t] */
    std::vector<drfe::MapPointUpkeep> CreateMapPoints(const std::vector<MapPointT*>& vpMPs, KeyFrameT* pKF, const std::vector<size_t>& idx,
                                                      const float* world, bool normals = true)
    {
        return CreatePoints(vpMPs, std::vector<KeyFrameT*>(vpMPs.size(), pKF), idx, nullptr, nullptr, pKF, world, normals);
    }
    /* The tail of LocalMapping::CreateNewMapLines2 (src/LocalMapping.cc:1019-1031) for the already constructed lines: as
     * CreateMapPoints, with AddMapLine; the store holds no line geometry, so UpdateAverageDir stays with the upkeep batch. */
    void CreateMapLines(const std::vector<MapLineT*>& vpMLs, const std::vector<KeyFrameT*>& kf1, const std::vector<size_t>& idx1,
                        const std::vector<KeyFrameT*>& kf2, const std::vector<size_t>& idx2, KeyFrameT* pRefKF)
    {
        CreateLines(vpMLs, kf1, idx1, &kf2, &idx2, pRefKF);
    }
    void CreateMapLines(const std::vector<MapLineT*>& vpMLs, KeyFrameT* pKF, const std::vector<size_t>& idx)
    {
        CreateLines(vpMLs, std::vector<KeyFrameT*>(vpMLs.size(), pKF), idx, nullptr, nullptr, pKF);
    }
    /* mpReplaced of pMP as the store holds it: the handle, or -1 */
    int32_t Replaced(MapPointT* pMP)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t handle = (int32_t)pMP->mnId;
        int32_t out = -1;
        Check(drfe_lmap_get_replaced(mDb, DRFE_LMAP_POINT, 1, &handle, &out), "drfe_lmap_get_replaced");
        return out;
    }
    drfe_lmap* db() const { return mDb; }

private:
    void Check(int rc, const char* what) const
    {
        if (rc != DRFE_OK) throw std::runtime_error(std::string(what) + ": " + drfe_lmap_last_error(mDb));
    }
    /* the arrays of one kind of a drfe_lmap_create_call */
    struct CreateArrays {
        std::vector<int32_t> handle, nObs, kf, idx, ref, displaced;
        std::vector<int64_t> first;
    };
    template <class ItemT>
    static CreateArrays CreateFill(const std::vector<ItemT*>& items, const std::vector<KeyFrameT*>& kf1, const std::vector<size_t>& idx1,
                                   const std::vector<KeyFrameT*>* kf2, const std::vector<size_t>* idx2, KeyFrameT* pRefKF)
    {
        const size_t n = items.size();
        CreateArrays A;
        A.handle.resize(n); A.nObs.resize(n); A.kf.assign(2 * n, 0); A.idx.assign(2 * n, 0); A.ref.resize(n); A.first.resize(n);
        A.displaced.assign(2 * n + 1, -1);
        for (size_t t = 0; t < n; t++) {
            A.handle[t] = (int32_t)items[t]->mnId;
            A.nObs[t] = kf2 ? 2 : 1;
            A.kf[2 * t] = (int32_t)kf1[t]->mnId; A.idx[2 * t] = (int32_t)idx1[t];
            if (kf2) { A.kf[2 * t + 1] = (int32_t)(*kf2)[t]->mnId; A.idx[2 * t + 1] = (int32_t)(*idx2)[t]; }
            A.ref[t] = (int32_t)pRefKF->mnId;
            A.first[t] = (int64_t)items[t]->mnFirstKFid;
        }
        return A;
    }
    int CreateCall(drfe_lmap_create_call* c)
    {
        return mForce < 0 ? drfe_lmap_create_host(mDb, c) : mForce > 0 ? drfe_lmap_create_device(mDb, c, nullptr) : drfe_lmap_create_batch(mDb, c, nullptr);
    }
    std::vector<drfe::MapPointUpkeep> CreatePoints(const std::vector<MapPointT*>& vpMPs, const std::vector<KeyFrameT*>& kf1,
                                                   const std::vector<size_t>& idx1, const std::vector<KeyFrameT*>* kf2,
                                                   const std::vector<size_t>* idx2, KeyFrameT* pRefKF, const float* world, bool normals)
    {
        const size_t n = vpMPs.size();
        std::vector<drfe::MapPointUpkeep> records(n);
        if (!n) return records;
        CreateArrays A = CreateFill(vpMPs, kf1, idx1, kf2, idx2, pRefKF);
        std::vector<float> nrm(3 * n), maxD(n), minD(n);
        std::vector<uint8_t> status(n);
        drfe_lmap_create_call c = {};
        c.n_points = (int32_t)n;
        c.point_handle = A.handle.data(); c.point_n_obs = A.nObs.data(); c.point_obs_kf = A.kf.data(); c.point_obs_index = A.idx.data();
        c.point_ref_kf = A.ref.data(); c.point_first_kf = A.first.data(); c.point_world = world;
        c.displaced_capacity[0] = (int32_t)(2 * n); c.record_capacity = (int32_t)n; c.point_displaced = A.displaced.data();
        c.normal = normals ? nrm.data() : nullptr; c.max_distance = maxD.data(); c.min_distance = minD.data(); c.status = status.data();
        {
            std::unique_lock<std::mutex> lock(mMutex);
            Check(CreateCall(&c), "drfe_lmap_create");
            for (size_t t = 0; t < n; t++) mMPs[A.handle[t]] = vpMPs[t];
        }
        for (size_t t = 0; t < n; t++) {
            /* the reference's tail on the objects */
            vpMPs[t]->AddObservation(kf1[t], idx1[t]);
            if (kf2) vpMPs[t]->AddObservation((*kf2)[t], (*idx2)[t]);
            kf1[t]->AddMapPoint(vpMPs[t], idx1[t]);
            if (kf2) (*kf2)[t]->AddMapPoint(vpMPs[t], (*idx2)[t]);
            if (!normals) continue;
            drfe::MapPointUpkeep& u = records[t];
            u.status = status[t];
            for (int k = 0; k < 3; k++) u.normal[k] = nrm[3 * t + (size_t)k];
            u.max_distance = maxD[t];
            u.min_distance = minD[t];
        }
        return records;
    }
    void CreateLines(const std::vector<MapLineT*>& vpMLs, const std::vector<KeyFrameT*>& kf1, const std::vector<size_t>& idx1,
                     const std::vector<KeyFrameT*>* kf2, const std::vector<size_t>* idx2, KeyFrameT* pRefKF)
    {
        const size_t n = vpMLs.size();
        if (!n) return;
        CreateArrays A = CreateFill(vpMLs, kf1, idx1, kf2, idx2, pRefKF);
        drfe_lmap_create_call c = {};
        c.n_lines = (int32_t)n;
        c.line_handle = A.handle.data(); c.line_n_obs = A.nObs.data(); c.line_obs_kf = A.kf.data(); c.line_obs_index = A.idx.data();
        c.line_ref_kf = A.ref.data(); c.line_first_kf = A.first.data();
        c.displaced_capacity[1] = (int32_t)(2 * n); c.line_displaced = A.displaced.data();
        {
            std::unique_lock<std::mutex> lock(mMutex);
            Check(CreateCall(&c), "drfe_lmap_create");
            for (size_t t = 0; t < n; t++) mMLs[A.handle[t]] = vpMLs[t];
        }
        for (size_t t = 0; t < n; t++) {
            vpMLs[t]->AddObservation(kf1[t], idx1[t]);
            if (kf2) vpMLs[t]->AddObservation((*kf2)[t], (*idx2)[t]);
            kf1[t]->AddMapLine(vpMLs[t], idx1[t]);
            if (kf2) (*kf2)[t]->AddMapLine(vpMLs[t], (*idx2)[t]);
        }
    }
    void Increase(int kind, int32_t handle, int dFound, int dVisible)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int32_t df = (int32_t)dFound, dv = (int32_t)dVisible;
        Check(drfe_lmap_recent_increase(mDb, kind, 1, &handle, &df, &dv), "drfe_lmap_recent_increase");
    }
    template <class ItemT> void RecentCulling(std::list<ItemT*>& recent, int64_t current, bool bMonocular, int kind)
    {
        const size_t n = recent.size();
        if (n == 0) return;
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<int32_t> handles;
        for (ItemT* p : recent) handles.push_back((int32_t)p->mnId);
        std::vector<uint8_t> action(n);
        std::vector<int32_t> kept(n), culled(n), erOff(n + 1), erKf, erIdx;
        int32_t nKept = 0, nCulled = 0, none = 0, noneOff = 0;
        /* the erased observations grow until the call fits (a call that does not fit changes nothing) */
        for (size_t cap = 8 * n + 1024;; cap *= 8) {
            erKf.resize(cap);
            erIdx.resize(cap);
            drfe_lmap_recent_list mine = {}, other = {};
            mine.n = (int32_t)n; mine.handles = handles.data(); mine.erased_capacity = (int32_t)cap;
            mine.action = action.data(); mine.n_kept = &nKept; mine.kept = kept.data(); mine.n_culled = &nCulled; mine.culled = culled.data();
            mine.erased_offsets = erOff.data(); mine.erased_kf = erKf.data(); mine.erased_index = erIdx.data();
            other.n_kept = other.n_culled = &none; other.erased_offsets = &noneOff;
            drfe_lmap_recent_list* points = kind == DRFE_LMAP_POINT ? &mine : &other;
            drfe_lmap_recent_list* lines = kind == DRFE_LMAP_POINT ? &other : &mine;
            const int32_t mono = bMonocular ? 1 : 0;
            const int rc = mForce < 0 ? drfe_lmap_recent_cull_host(mDb, current, mono, points, lines)
                         : mForce > 0 ? drfe_lmap_recent_cull_device(mDb, current, mono, points, lines, nullptr)
                                      : drfe_lmap_recent_cull_batch(mDb, current, mono, points, lines, nullptr);
            if (rc == DRFE_ERR_CAPACITY && cap < ((size_t)1 << 28) &&
                std::string(drfe_lmap_last_error(mDb)).find("than erased_capacity") != std::string::npos)
                continue;
            Check(rc, "drfe_lmap_recent_cull");
            break;
        }
        lock.unlock();
        size_t i = 0;
        for (auto lit = recent.begin(); lit != recent.end(); i++) {
            if (action[i] == DRFE_LMAP_RECENT_RATIO || action[i] == DRFE_LMAP_RECENT_OBSERVATIONS) (*lit)->SetBadFlag();
            if (action[i] == DRFE_LMAP_RECENT_KEPT) ++lit;
            else lit = recent.erase(lit);
        }
    }
    template <class M> void Drop(M& known, int kind, int32_t handle)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (!known.erase(handle)) return;
        Check(drfe_lmap_remove(mDb, kind, handle), "drfe_lmap_remove");
    }

    drfe_detail::CtxPtr mCtx;
    drfe_lmap* mDb = nullptr;
    int mForce = 0;
    std::mutex mMutex;
    std::map<int32_t, KeyFrameT*> mKFs;
    std::map<int32_t, MapPointT*> mMPs;
    std::map<int32_t, MapLineT*> mMLs;
};

}  // namespace Planar_SLAM

#endif /* DRFE_ADAPTOR_HPP */
