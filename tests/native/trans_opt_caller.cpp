/* trans_opt_caller.cpp — Planar_SLAM::Optimizer::TranslationOptimization(Frame*, bool) with the reference's signature and
 * drfe::TransOptBatch over the adaptor, on stand-in Frame / MapPoint / MapLine / MapPlane types that hold what the reference's
 * function reads (src/Optimizer.cc:3211-3980): first every frame on its own through the Optimizer, then all of them through one
 * batch.
 *
 *   trans_opt_caller <in.bin> <out.bin> [host | auto]
 * Without a third argument both go to the device; `auto` leaves them their default threshold (DRFE_TRANSOPT_DEVICE_FROM frames);
 * `host` forces the host entry.
 * in:  int32 n; float invSigma2[8]; per frame: float Tcw[16], K[4], bf; int32 bStruct, N, NL, M; per key uint8 has, float pt[2], ur,
 *      int32 octave, float Xw[3]; per line uint8 has, double fn[3], ends[6]; per plane uint8 mask, float meas[4], world[12]
 * out: two passes (Optimizer, batch) of one record per frame { int32 ret; float Tcw[16]; uint8 mvbOutlier[N], mvbLineOutlier[NL],
 *      mvbPlaneOutlier[M], mvbParPlaneOutlier[M], mvbVerPlaneOutlier[M] }.  stdout also says how many device calls and frames the
 *      batch's own context counted (drfe_trans_opt_stats), which shows on which side of DRFE_TRANSOPT_DEVICE_FROM `auto` fell.  Compared by tests/test_gpu_trans_opt.py and
 *      tests/test_trans_opt_cpu.py with the ctypes path. */
#include "drfe_adaptor.hpp"

#include <cstdio>
#include <memory>
#include <string>
#include <vector>

namespace {

struct MapPoint {
    float w[3];
    drfe_cv::Mat GetWorldPos() const { return drfe::drfe_detail_sim3::mat32(3, 1, w); }
};
struct Vec6 {
    double v[6];
    double operator()(int i) const { return v[i]; }
};
struct Vec3 {
    double v[3];
    double operator()(int i) const { return v[i]; }
};
struct MapLine { Vec6 mWorldPos; };
struct MapPlane {
    float w[4];
    drfe_cv::Mat GetWorldPos() const { return drfe::drfe_detail_sim3::mat32(4, 1, w); }
};
struct Frame {
    drfe_cv::Mat mTcw;
    float fx, fy, cx, cy, mbf;
    int N = 0, NL = 0, mnPlaneNum = 0;
    std::vector<drfe_cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier, mvbLineOutlier, mvbPlaneOutlier, mvbParPlaneOutlier, mvbVerPlaneOutlier;
    std::vector<Vec3> mvKeyLineFunctions;
    std::vector<MapLine*> mvpMapLines;
    std::vector<drfe_cv::Mat> mvPlaneCoefficients;
    std::vector<MapPlane*> mvpMapPlanes, mvpParallelPlanes, mvpVerticalPlanes;
    void SetPose(const drfe_cv::Mat& T) { mTcw = T; }
};

template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> void wr(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

void write_frame(FILE* o, int ret, const Frame& F)
{
    const int32_t r = ret;
    wr(o, &r, 1);
    for (int row = 0; row < 4; row++) wr(o, F.mTcw.ptr<float>(row), 4);
    for (const std::vector<bool>* v : {&F.mvbOutlier, &F.mvbLineOutlier, &F.mvbPlaneOutlier, &F.mvbParPlaneOutlier, &F.mvbVerPlaneOutlier})
        for (bool b : *v) { const uint8_t u = b ? 1 : 0; wr(o, &u, 1); }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string mode = argc > 3 ? argv[3] : "device";
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t n = 0;
    float inv[8];
    if (!rd(f, &n, 1) || n < 0 || !rd(f, inv, 8)) return 4;
    std::vector<std::unique_ptr<MapPoint>> points;
    std::vector<std::unique_ptr<MapLine>> lines;
    std::vector<std::unique_ptr<MapPlane>> planes;
    std::vector<Frame> frames((size_t)n);
    std::vector<int> bStruct((size_t)n);
    for (int k = 0; k < n; k++) {
        Frame& F = frames[(size_t)k];
        float T[16], K[4], bf;
        int32_t h[4];
        if (!rd(f, T, 16) || !rd(f, K, 4) || !rd(f, &bf, 1) || !rd(f, h, 4)) return 4;
        F.mTcw = drfe::drfe_detail_sim3::mat32(4, 4, T);
        F.fx = K[0]; F.fy = K[1]; F.cx = K[2]; F.cy = K[3]; F.mbf = bf;
        bStruct[(size_t)k] = h[0]; F.N = h[1]; F.NL = h[2]; F.mnPlaneNum = h[3];
        F.mvInvLevelSigma2.assign(inv, inv + 8);
        for (int i = 0; i < F.N; i++) {
            uint8_t has; float pt[2], ur, X[3]; int32_t oct;
            if (!rd(f, &has, 1) || !rd(f, pt, 2) || !rd(f, &ur, 1) || !rd(f, &oct, 1) || !rd(f, X, 3)) return 4;
            drfe_cv::KeyPoint kp{};
            kp.pt.x = pt[0]; kp.pt.y = pt[1]; kp.octave = oct;
            F.mvKeysUn.push_back(kp);
            F.mvuRight.push_back(ur);
            MapPoint* p = nullptr;
            if (has) { points.emplace_back(new MapPoint{{X[0], X[1], X[2]}}); p = points.back().get(); }
            F.mvpMapPoints.push_back(p);
        }
        F.mvbOutlier.assign((size_t)F.N, false);
        for (int i = 0; i < F.NL; i++) {
            uint8_t has; Vec3 fn; Vec6 e;
            if (!rd(f, &has, 1) || !rd(f, fn.v, 3) || !rd(f, e.v, 6)) return 4;
            F.mvKeyLineFunctions.push_back(fn);
            MapLine* p = nullptr;
            if (has) { lines.emplace_back(new MapLine{e}); p = lines.back().get(); }
            F.mvpMapLines.push_back(p);
        }
        F.mvbLineOutlier.assign((size_t)F.NL, false);
        for (int i = 0; i < F.mnPlaneNum; i++) {
            uint8_t mask; float meas[4], w[12];
            if (!rd(f, &mask, 1) || !rd(f, meas, 4) || !rd(f, w, 12)) return 4;
            F.mvPlaneCoefficients.push_back(drfe::drfe_detail_sim3::mat32(4, 1, meas));
            MapPlane* p[3] = {nullptr, nullptr, nullptr};
            for (int q = 0; q < 3; q++)
                if (mask & (1 << q)) { planes.emplace_back(new MapPlane{{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]}}); p[q] = planes.back().get(); }
            F.mvpMapPlanes.push_back(p[0]); F.mvpParallelPlanes.push_back(p[1]); F.mvpVerticalPlanes.push_back(p[2]);
        }
        F.mvbPlaneOutlier.assign((size_t)F.mnPlaneNum, false);
        F.mvbParPlaneOutlier.assign((size_t)F.mnPlaneNum, false);
        F.mvbVerPlaneOutlier.assign((size_t)F.mnPlaneNum, false);
    }
    fclose(f);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    long long batchStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    try {
        /* TranslationWithMotionModel / TranslationEstimation: one frame a call */
        if (mode != "auto") Planar_SLAM::Optimizer::UseDevice(mode == "device");
        std::vector<Frame> single = frames;
        for (int k = 0; k < n; k++) write_frame(o, Planar_SLAM::Optimizer::TranslationOptimization(&single[(size_t)k], bStruct[(size_t)k] != 0), single[(size_t)k]);
        /* the frames of a batched tracker: one call */
        drfe::TransOptBatch<Frame> batch;
        if (mode != "auto") batch.UseDevice(mode == "device");
        std::vector<Frame> many = frames;
        for (int k = 0; k < n; k++) batch.Add(&many[(size_t)k], bStruct[(size_t)k] != 0);
        batch.Run();
        for (int k = 0; k < n; k++) write_frame(o, batch.Result((size_t)k), many[(size_t)k]);
        /* what the batch sent to the device entry: nothing when it never made a context */
        if (batch.ctx()) {
            int64_t st[8];
            if (drfe_trans_opt_stats(batch.ctx(), st) == DRFE_OK)
                for (int k = 0; k < 8; k++) batchStats[k] = (long long)st[k];
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "trans_opt_caller: %s\n", e.what());
        return 6;
    }
    fclose(o);
    printf("trans_opt_caller ok (%d frames, %s)\n", n, mode.c_str());
    printf("batch device calls %lld, frames %lld, handed back %lld\n", batchStats[0], batchStats[1], batchStats[6]);
    return 0;
}
