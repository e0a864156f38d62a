/* sim3_caller.cpp — the candidate loop of LoopClosing::ComputeSim3 (reference src/LoopClosing.cc:320-388) over
 * Planar_SLAM::Sim3Solver with the reference's signatures, on stand-in KeyFrame / MapPoint types: the solvers are built from
 * (pKF1, pKF2, vpMatched12, bFixScale), drfe::Sim3Batch fills all their tables with one device call, and the loop gives every
 * candidate five iterations in turn until a transform passes the (stubbed) optimisation.  g2o's OptimizeSim3 is not part of this
 * project: the stub accepts the third transform handed back, so that the loop also goes on after a failed one.
 *
 *   sim3_caller <in.bin> <out.bin> [host]
 * in:  int32 nCand, fixScale; the current keyframe; per candidate its keyframe and vpMatched12 (int32 per current keypoint: the
 *      candidate's keypoint whose map point it is, or -1).
 *      keyframe = float Tcw[16], K[4], sigma2[8]; int32 nKeys; int32 octave[nKeys]; float world[nKeys][3]; uint8 state[nKeys]
 *      (0 a map point, 1 a bad one, 2 none, 3 one that does not list this keyframe)
 * out: per iterate() call a record { int32 cand, noMore, hasT, nInliers; float T[16], R[9], t[3], s; uint8 vbInliers[N1] }
 *      (T, R, t, s zero when no transform came back), compared by tests/test_gpu_sim3.py with the ctypes path. */
#include "drfe_adaptor.hpp"

#include <cstdio>
#include <memory>
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
    float Tcw[16];
    float fx, fy, cx, cy;
    std::vector<drfe_cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint*> mps;
    std::vector<std::unique_ptr<MapPoint>> own;
    drfe_cv::Mat GetPose() const { return drfe::drfe_detail_sim3::mat32(4, 4, Tcw); }
    std::vector<MapPoint*> GetMapPointMatches() const { return mps; }
};

template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

bool read_kf(FILE* f, KeyFrame& k)
{
    float K[4], sig[8];
    int32_t n = 0;
    if (!rd(f, k.Tcw, 16) || !rd(f, K, 4) || !rd(f, sig, 8) || !rd(f, &n, 1) || n < 0) return false;
    k.fx = K[0]; k.fy = K[1]; k.cx = K[2]; k.cy = K[3];
    k.mvLevelSigma2.assign(sig, sig + 8);
    std::vector<int32_t> oct((size_t)n);
    std::vector<float> w(3 * (size_t)n);
    std::vector<uint8_t> st((size_t)n);
    if (!rd(f, oct.data(), oct.size()) || !rd(f, w.data(), w.size()) || !rd(f, st.data(), st.size())) return false;
    for (int i = 0; i < n; i++) {
        drfe_cv::KeyPoint kp{};
        kp.octave = oct[(size_t)i];
        k.mvKeysUn.push_back(kp);
        MapPoint* mp = nullptr;
        if (st[(size_t)i] != 2) {
            k.own.emplace_back(new MapPoint());
            mp = k.own.back().get();
            for (int q = 0; q < 3; q++) mp->w[q] = w[3 * (size_t)i + q];
            mp->bad = st[(size_t)i] == 1;
            mp->kf = st[(size_t)i] == 3 ? nullptr : &k;
            mp->idx = i;
        }
        k.mps.push_back(mp);
    }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const bool host = argc > 3;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[2];
    if (!rd(f, head, 2)) return 4;
    const int nInitialCandidates = head[0];
    const bool mbFixScale = head[1] != 0;
    KeyFrame cur;
    if (!read_kf(f, cur)) return 4;
    KeyFrame* mpCurrentKF = &cur;
    std::vector<std::unique_ptr<KeyFrame>> cands;
    std::vector<std::vector<MapPoint*>> vvpMapPointMatches((size_t)nInitialCandidates);
    for (int i = 0; i < nInitialCandidates; i++) {
        cands.emplace_back(new KeyFrame());
        if (!read_kf(f, *cands.back())) return 4;
        std::vector<int32_t> m(cur.mps.size());
        if (!rd(f, m.data(), m.size())) return 4;
        for (int32_t j : m) vvpMapPointMatches[(size_t)i].push_back(j < 0 ? nullptr : cands.back()->mps[(size_t)j]);
    }
    fclose(f);

    using Solver = Planar_SLAM::Sim3Solver<KeyFrame, MapPoint>;
    std::vector<Solver*> vpSim3Solvers((size_t)nInitialCandidates);
    std::vector<std::unique_ptr<Solver>> owned;
    std::vector<bool> vbDiscarded((size_t)nInitialCandidates, false);
    int nCandidates = 0;
    for (int i = 0; i < nInitialCandidates; i++) {
        KeyFrame* pKF = cands[(size_t)i].get();
        Solver* pSolver = new Solver(mpCurrentKF, pKF, vvpMapPointMatches[(size_t)i], mbFixScale);
        owned.emplace_back(pSolver);
        pSolver->SetRansacParameters(0.99, 20, 300);
        pSolver->SetSeed((uint32_t)(i + 1));
        vpSim3Solvers[(size_t)i] = pSolver;
        nCandidates++;
    }
    /* every hypothesis of every candidate in one launch; without this the first iterate() of each solver fills it on the host */
    std::unique_ptr<drfe::Sim3Batch> batch;
    if (!host) {
        batch.reset(new drfe::Sim3Batch());
        batch->Fill(vpSim3Solvers);
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    bool bMatch = false;
    int handedBack = 0, calls = 0;
    while (nCandidates > 0 && !bMatch) {
        for (int i = 0; i < nInitialCandidates; i++) {
            if (vbDiscarded[(size_t)i]) continue;
            std::vector<bool> vbInliers;
            int nInliers;
            bool bNoMore;
            Solver* pSolver = vpSim3Solvers[(size_t)i];
            drfe_cv::Mat Scm = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
            calls++;
            if (bNoMore) {
                vbDiscarded[(size_t)i] = true;
                nCandidates--;
            }
            const int32_t rec[4] = {i, bNoMore ? 1 : 0, Scm.empty() ? 0 : 1, nInliers};
            float v[29] = {0};
            if (!Scm.empty()) {
                const drfe_cv::Mat R = pSolver->GetEstimatedRotation();
                const drfe_cv::Mat t = pSolver->GetEstimatedTranslation();
                const float s = pSolver->GetEstimatedScale();
                for (int r = 0; r < 4; r++)
                    for (int c = 0; c < 4; c++) v[r * 4 + c] = Scm.ptr<float>(r)[c];
                for (int r = 0; r < 3; r++)
                    for (int c = 0; c < 3; c++) v[16 + r * 3 + c] = R.ptr<float>(r)[c];
                for (int r = 0; r < 3; r++) v[25 + r] = t.ptr<float>(r)[0];
                v[28] = s;
            }
            fwrite(rec, sizeof(rec), 1, o);
            fwrite(v, sizeof(v), 1, o);
            for (bool b : vbInliers) fputc(b ? 1 : 0, o);
            if (!Scm.empty()) {
                /* SearchBySim3 and OptimizeSim3 would run here; the stub's verdict */
                if (++handedBack >= 3) {
                    bMatch = true;
                    break;
                }
            }
        }
    }
    fclose(o);
    printf("sim3_caller ok: %d iterate calls, %d transforms, match %d\n", calls, handedBack, bMatch ? 1 : 0);
    return 0;
}
