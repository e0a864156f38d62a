/* pnp_caller.cpp — the candidate loop of Tracking::Relocalization (reference src/Tracking.cc:3600-3700) over
 * Planar_SLAM::PnPsolver with the reference's signatures, on stand-in Frame / MapPoint types: a solver per candidate keyframe from
 * (mCurrentFrame, vvpMapPointMatches[i]), SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), drfe::PnPBatch fills all their tables
 * with one call, and the loop gives every candidate iterate(5, ..) in turn, discarding it on bNoMore.  g2o's PoseOptimization is not
 * part of this project: a caller-supplied list says which of the poses handed back it accepts, so that rejected ones send the
 * loop on and exercise the cursor.
 *
 *   pnp_caller <in.bin> <out.bin> [host | auto]
 * Without a third argument drfe::PnPBatch sends every call to the device; `auto` leaves it its default threshold
 * (DRFE_PNP_DEVICE_FROM solvers, so these three candidates go to the host entry through the batch); `host` uses no batch: every
 * solver fills its own table on first use.
 * in:  int32 nCand, nVerdicts; uint8 verdict[nVerdicts] (the k-th pose handed back is accepted when verdict[k] != 0; past the list:
 *      rejected); the frame: float K[4], sigma2[8]; int32 nKeys; float pt[nKeys][2]; int32 octave[nKeys]; per candidate
 *      uint8 state[nKeys] (0 a map point, 1 a bad one, 2 none) and float world[nKeys][3]
 * out: per iterate() call a record { int32 cand, noMore, hasT, nInliers, nFlags; float T[16]; uint8 vbInliers[nFlags] }
 *      (T zero when no pose came back); after the loop one more record with cand = -1: find() of a fresh solver over the last
 *      candidate.  Compared by tests/test_gpu_pnp.py and tests/test_pnp_cpu.py with the ctypes path. */
#include "drfe_adaptor.hpp"

#include <cstdio>
#include <memory>
#include <string>
#include <vector>

namespace {

struct MapPoint {
    float w[3];
    bool bad = false;
    drfe_cv::Mat GetWorldPos() const { return drfe::drfe_detail_sim3::mat32(3, 1, w); }
    bool isBad() const { return bad; }
};
struct Frame {
    float fx, fy, cx, cy;
    std::vector<drfe_cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
};

template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string mode = argc > 3 ? argv[3] : "device";
    const bool host = mode == "host";
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[2];
    if (!rd(f, head, 2) || head[0] < 0 || head[1] < 0) return 4;
    const int nKFs = head[0];
    std::vector<uint8_t> verdict((size_t)head[1]);
    float K[4], sig[8];
    int32_t nKeys = 0;
    if (!rd(f, verdict.data(), verdict.size()) || !rd(f, K, 4) || !rd(f, sig, 8) || !rd(f, &nKeys, 1) || nKeys < 0) return 4;
    Frame mCurrentFrame;
    mCurrentFrame.fx = K[0]; mCurrentFrame.fy = K[1]; mCurrentFrame.cx = K[2]; mCurrentFrame.cy = K[3];
    mCurrentFrame.mvLevelSigma2.assign(sig, sig + 8);
    std::vector<float> pt(2 * (size_t)nKeys);
    std::vector<int32_t> oct((size_t)nKeys);
    if (!rd(f, pt.data(), pt.size()) || !rd(f, oct.data(), oct.size())) return 4;
    for (int i = 0; i < nKeys; i++) {
        drfe_cv::KeyPoint kp{};
        kp.pt.x = pt[2 * (size_t)i];
        kp.pt.y = pt[2 * (size_t)i + 1];
        kp.octave = oct[(size_t)i];
        mCurrentFrame.mvKeysUn.push_back(kp);
    }
    std::vector<std::unique_ptr<MapPoint>> own;
    std::vector<std::vector<MapPoint*>> vvpMapPointMatches((size_t)nKFs);
    for (int i = 0; i < nKFs; i++) {
        std::vector<uint8_t> st((size_t)nKeys);
        std::vector<float> w(3 * (size_t)nKeys);
        if (!rd(f, st.data(), st.size()) || !rd(f, w.data(), w.size())) return 4;
        for (int j = 0; j < nKeys; j++) {
            MapPoint* mp = nullptr;
            if (st[(size_t)j] != 2) {
                own.emplace_back(new MapPoint());
                mp = own.back().get();
                for (int q = 0; q < 3; q++) mp->w[q] = w[3 * (size_t)j + q];
                mp->bad = st[(size_t)j] == 1;
            }
            vvpMapPointMatches[(size_t)i].push_back(mp);
        }
    }
    fclose(f);

    using Solver = Planar_SLAM::PnPsolver<Frame, MapPoint>;
    std::vector<Solver*> vpPnPsolvers((size_t)nKFs);
    std::vector<std::unique_ptr<Solver>> owned;
    std::vector<bool> vbDiscarded((size_t)nKFs, false);
    int nCandidates = 0;
    for (int i = 0; i < nKFs; i++) {
        Solver* pSolver = new Solver(mCurrentFrame, vvpMapPointMatches[(size_t)i]);
        owned.emplace_back(pSolver);
        pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        pSolver->SetSeed((uint32_t)(i + 1));
        vpPnPsolvers[(size_t)i] = pSolver;
        nCandidates++;
    }
    /* every row of every candidate in one call; without this the first iterate() of each solver fills it on the host */
    std::unique_ptr<drfe::PnPBatch> batch;
    if (!host) {
        batch.reset(mode == "auto" ? new drfe::PnPBatch() : new drfe::PnPBatch(0, 1));
        batch->Fill(vpPnPsolvers);
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    bool bMatch = false;
    int handedBack = 0, calls = 0, refills = 0;
    while (nCandidates > 0 && !bMatch) {
        for (int i = 0; i < nKFs; i++) {
            if (vbDiscarded[(size_t)i]) continue;
            std::vector<bool> vbInliers;
            int nInliers;
            bool bNoMore;
            Solver* pSolver = vpPnPsolvers[(size_t)i];
            drfe_cv::Mat Tcw = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
            calls++;
            if (bNoMore) {
                vbDiscarded[(size_t)i] = true;
                nCandidates--;
            }
            const int32_t rec[5] = {i, bNoMore ? 1 : 0, Tcw.empty() ? 0 : 1, nInliers, (int32_t)vbInliers.size()};
            float v[16] = {0};
            if (!Tcw.empty())
                for (int r = 0; r < 4; r++)
                    for (int c = 0; c < 4; c++) v[r * 4 + c] = Tcw.ptr<float>(r)[c];
            fwrite(rec, sizeof(rec), 1, o);
            fwrite(v, sizeof(v), 1, o);
            for (bool b : vbInliers) fputc(b ? 1 : 0, o);
            if (!Tcw.empty()) {
                /* PoseOptimization and SearchByProjection would run here; the caller's verdict */
                const bool good = (size_t)handedBack < verdict.size() && verdict[(size_t)handedBack] != 0;
                handedBack++;
                if (good) {
                    bMatch = true;
                    break;
                }
            }
        }
    }
    if (nKFs > 0) {
        /* find(): iterate(mRansacMaxIts, ..) of a solver that has not iterated yet */
        Solver fresh(mCurrentFrame, vvpMapPointMatches[(size_t)nKFs - 1]);
        fresh.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        fresh.SetSeed((uint32_t)nKFs);
        if (batch) batch->Fill(std::vector<Solver*>{&fresh});
        std::vector<bool> vbInliers;
        int nInliers;
        drfe_cv::Mat Tcw = fresh.find(vbInliers, nInliers);
        const int32_t rec[5] = {-1, 0, Tcw.empty() ? 0 : 1, nInliers, (int32_t)vbInliers.size()};
        float v[16] = {0};
        if (!Tcw.empty())
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) v[r * 4 + c] = Tcw.ptr<float>(r)[c];
        fwrite(rec, sizeof(rec), 1, o);
        fwrite(v, sizeof(v), 1, o);
        for (bool b : vbInliers) fputc(b ? 1 : 0, o);
    }
    fclose(o);
    for (Solver* s : vpPnPsolvers) refills += s->Refills();
    printf("pnp_caller ok: %d iterate calls, %d poses, %d refills, match %d\n", calls, handedBack, refills, bMatch ? 1 : 0);
    return 0;
}
