/* sim3_opt_caller.cpp — the part of LoopClosing::ComputeSim3's candidate loop (reference src/LoopClosing.cc:333-388) that follows
 * SearchBySim3, with the real optimisation where sim3_caller.cpp has a stub, on stand-in KeyFrame / MapPoint / Sim3 types that hold
 * what Optimizer::OptimizeSim3 reads (src/Optimizer.cc:3982-4177).  What Sim3Solver::iterate and SearchBySim3 hand to it (gScm and
 * vpMapPointMatches) comes from the input file; tests/native/sim3_caller.cpp and the matcher callers cover those steps.
 * First the loop as the reference runs it, candidate after candidate through Planar_SLAM::Optimizer::OptimizeSim3 until one has
 * 20 inliers; then the live candidates of the round through one drfe::Sim3OptBatch.
 *
 *   sim3_opt_caller <in.bin> <out.bin> [host | auto]
 * Without a third argument both go to the device; `auto` leaves them their default threshold (DRFE_SIM3OPT_DEVICE_FROM
 * candidates); `host` forces the host entry.
 * in:  int32 nCand, fixScale; float th2, invSigma2[8]; the current keyframe; per candidate its keyframe, double gScm[8] (rotation
 *      x y z w, translation, scale) and vpMapPointMatches (int32 per current keypoint: the candidate's keypoint whose map point it
 *      is, or -1).
 *      keyframe = float K[4], R[9], t[3]; int32 nKeys; per key float pt[2]; int32 octave; float world[3]; uint8 state (0 a map
 *      point, 1 a bad one, 2 none, 3 one that does not list this keyframe)
 * out: the loop's records, int32 -1, the batch's records, int32 -1, int32 matched candidate of the loop and of the batch (-1 none).
 *      record = { int32 cand, nInliers; double gScm[8]; float mScw[16]; uint8 isNull[N1] }.  stdout also says how many device calls
 *      and problems the batch's own context counted (drfe_sim3_opt_stats).  Compared by tests/test_sim3_opt_cpu.py and
 *      tests/test_gpu_sim3_opt.py with the ctypes path. */
#include "drfe_adaptor.hpp"

#include <cstdio>
#include <memory>
#include <string>
#include <vector>

namespace {

struct KeyFrame;
struct MapPoint {
    float w[3];
    bool bad = false;
    const KeyFrame* kf = nullptr;
    int idx = -1;
    drfe_cv::Mat GetWorldPos() const { return drfe::drfe_detail_sim3::mat32(3, 1, w); }
    bool isBad() const { return bad; }
    int GetIndexInKeyFrame(const KeyFrame* k) const { return k == kf ? idx : -1; }
};
struct KeyFrame {
    drfe_cv::Mat mK;
    float R[9], t[3];
    std::vector<drfe_cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    std::vector<MapPoint*> mps;
    std::vector<std::unique_ptr<MapPoint>> own;
    drfe_cv::Mat GetRotation() const { return drfe::drfe_detail_sim3::mat32(3, 3, R); }
    drfe_cv::Mat GetTranslation() const { return drfe::drfe_detail_sim3::mat32(3, 1, t); }
    std::vector<MapPoint*> GetMapPointMatches() const { return mps; }
};
/* what the adaptor needs of g2o::Sim3 */
struct Quat {
    double c[4];
    double& x() { return c[0]; } double& y() { return c[1]; } double& z() { return c[2]; } double& w() { return c[3]; }
    double x() const { return c[0]; } double y() const { return c[1]; } double z() const { return c[2]; } double w() const { return c[3]; }
};
struct Vec3 {
    double v[3];
    double& operator[](int i) { return v[i]; }
    double operator[](int i) const { return v[i]; }
};
struct Sim3 {
    Quat r; Vec3 tr; double s;
    Quat& rotation() { return r; } const Quat& rotation() const { return r; }
    Vec3& translation() { return tr; } const Vec3& translation() const { return tr; }
    double& scale() { return s; } const double& scale() const { return s; }
};

template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> void wr(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

bool read_kf(FILE* f, KeyFrame& k, const float* inv)
{
    float K[4];
    int32_t n = 0;
    if (!rd(f, K, 4) || !rd(f, k.R, 9) || !rd(f, k.t, 3) || !rd(f, &n, 1) || n < 0) return false;
    const float Km[9] = {K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1};
    k.mK = drfe::drfe_detail_sim3::mat32(3, 3, Km);
    k.mvInvLevelSigma2.assign(inv, inv + 8);
    for (int i = 0; i < n; i++) {
        float pt[2], w[3]; int32_t oct; uint8_t st;
        if (!rd(f, pt, 2) || !rd(f, &oct, 1) || !rd(f, w, 3) || !rd(f, &st, 1)) return false;
        drfe_cv::KeyPoint kp{};
        kp.pt.x = pt[0]; kp.pt.y = pt[1]; kp.octave = oct;
        k.mvKeysUn.push_back(kp);
        MapPoint* mp = nullptr;
        if (st != 2) {
            k.own.emplace_back(new MapPoint());
            mp = k.own.back().get();
            for (int q = 0; q < 3; q++) mp->w[q] = w[q];
            mp->bad = st == 1;
            mp->kf = st == 3 ? nullptr : &k;
            mp->idx = i;
        }
        k.mps.push_back(mp);
    }
    return true;
}

void write_record(FILE* o, int cand, int nInliers, const Sim3& S, const drfe_cv::Mat& Scw, const std::vector<MapPoint*>& m)
{
    const int32_t h[2] = {cand, nInliers};
    wr(o, h, 2);
    wr(o, S.r.c, 4); wr(o, S.tr.v, 3); wr(o, &S.s, 1);
    for (int r = 0; r < 4; r++) wr(o, Scw.ptr<float>(r), 4);
    for (MapPoint* p : m) { const uint8_t u = p ? 0 : 1; wr(o, &u, 1); }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string mode = argc > 3 ? argv[3] : "device";
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[2];
    float th2, inv[8];
    if (!rd(f, head, 2) || !rd(f, &th2, 1) || !rd(f, inv, 8)) return 4;
    const int nInitialCandidates = head[0];
    const bool mbFixScale = head[1] != 0;
    KeyFrame cur;
    if (!read_kf(f, cur, inv)) return 4;
    KeyFrame* mpCurrentKF = &cur;
    std::vector<std::unique_ptr<KeyFrame>> cands;
    std::vector<Sim3> gScms((size_t)nInitialCandidates);
    std::vector<std::vector<MapPoint*>> vvpMapPointMatches((size_t)nInitialCandidates);
    for (int i = 0; i < nInitialCandidates; i++) {
        cands.emplace_back(new KeyFrame());
        if (!read_kf(f, *cands.back(), inv)) return 4;
        double S[8];
        std::vector<int32_t> m(cur.mps.size());
        if (!rd(f, S, 8) || !rd(f, m.data(), m.size())) return 4;
        for (int k = 0; k < 4; k++) gScms[(size_t)i].r.c[k] = S[k];
        for (int k = 0; k < 3; k++) gScms[(size_t)i].tr.v[k] = S[4 + k];
        gScms[(size_t)i].s = S[7];
        for (int32_t j : m) vvpMapPointMatches[(size_t)i].push_back(j < 0 ? nullptr : cands.back()->mps[(size_t)j]);
    }
    fclose(f);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    const int32_t end = -1;
    int32_t matched[2] = {-1, -1};
    long long batchStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    try {
        /* the loop as the reference runs it: one candidate a call, until one is accepted */
        if (mode != "auto") Planar_SLAM::Optimizer::UseDevice(mode == "device");
        for (int i = 0; i < nInitialCandidates; i++) {
            KeyFrame* pKF = cands[(size_t)i].get();
            std::vector<MapPoint*> vpMapPointMatches = vvpMapPointMatches[(size_t)i];
            Sim3 gScm = gScms[(size_t)i];
            const int nInliers = Planar_SLAM::Optimizer::OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, th2, mbFixScale);
            write_record(o, i, nInliers, gScm, Planar_SLAM::Optimizer::LastScw(), vpMapPointMatches);
            if (nInliers >= 20) { matched[0] = i; break; }
        }
        wr(o, &end, 1);
        /* the live candidates of a round in one call; the first accepted one is the match */
        drfe::Sim3OptBatch<KeyFrame, MapPoint, Sim3> batch;
        if (mode != "auto") batch.UseDevice(mode == "device");
        std::vector<std::vector<MapPoint*>> matches = vvpMapPointMatches;
        std::vector<Sim3> sims = gScms;
        for (int i = 0; i < nInitialCandidates; i++) batch.Add(mpCurrentKF, cands[(size_t)i].get(), matches[(size_t)i], sims[(size_t)i], th2, mbFixScale);
        batch.Run();
        for (int i = 0; i < nInitialCandidates; i++) {
            write_record(o, i, batch.Result((size_t)i), sims[(size_t)i], batch.Scw((size_t)i), matches[(size_t)i]);
            if (matched[1] < 0 && batch.Result((size_t)i) >= 20) matched[1] = i;
        }
        wr(o, &end, 1);
        wr(o, matched, 2);
        if (batch.ctx()) {
            int64_t st[8];
            if (drfe_sim3_opt_stats(batch.ctx(), st) == DRFE_OK)
                for (int k = 0; k < 8; k++) batchStats[k] = (long long)st[k];
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "sim3_opt_caller: %s\n", e.what());
        return 6;
    }
    fclose(o);
    printf("sim3_opt_caller ok (%d candidates, %s, match %d / %d)\n", nInitialCandidates, mode.c_str(), matched[0], matched[1]);
    printf("batch device calls %lld, problems %lld, handed back %lld\n", batchStats[0], batchStats[1], batchStats[6]);
    return 0;
}
