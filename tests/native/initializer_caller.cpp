/* initializer_caller.cpp — the Initialize call of Tracking::MonocularInitialization (reference src/Tracking.cc:1705-1721) over
 * Planar_SLAM::Initializer with the reference's signatures, on a stand-in Frame type: mpInitializer = new Initializer(
 * mInitialFrame, 1.0, iterations), then Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated) and the
 * caller's loop that drops the matches that were not triangulated.
 *
 *   initializer_caller <in.bin> <out.bin> [device | host | auto]
 * device / host force the entry (Initializer::UseDevice); auto leaves the adaptor's constant DRFE_INIT_DEVICE_FROM to decide.
 * in:  float K[9], sigma; int32 iterations; uint32 seed; int32 n1, n2; float keys1[n1][2], keys2[n2][2]; int32 matches[n1]
 * out: int32 ok, branch, flags, nmatches (after the caller's loop); float R[9], t[3] (zero when the Mat is empty);
 *      int32 n; float P3D[n][3]; uint8 vbTriangulated[n]; int32 matches[n1] (after the loop)
 * Compared by tests/test_gpu_initializer.py with the ctypes path. */
#include "drfe_adaptor.hpp"

#include <cstdio>
#include <string>
#include <vector>

namespace {

struct Point3f { float x = 0, y = 0, z = 0; };
struct Frame {
    drfe_cv::Mat mK;
    std::vector<drfe_cv::KeyPoint> mvKeysUn;
};

template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

void keys_of(Frame& fr, const std::vector<float>& pt)
{
    for (size_t i = 0; i < pt.size() / 2; i++) {
        drfe_cv::KeyPoint kp{};
        kp.pt.x = pt[2 * i];
        kp.pt.y = pt[2 * i + 1];
        fr.mvKeysUn.push_back(kp);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string mode = argc > 3 ? argv[3] : "auto";
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    float K[9], sigma;
    int32_t iterations, n[2];
    uint32_t seed;
    if (!rd(f, K, 9) || !rd(f, &sigma, 1) || !rd(f, &iterations, 1) || !rd(f, &seed, 1) || !rd(f, n, 2) || n[0] < 0 || n[1] < 0) return 4;
    std::vector<float> k1(2 * (size_t)n[0]), k2(2 * (size_t)n[1]);
    std::vector<int32_t> m((size_t)n[0]);
    if (!rd(f, k1.data(), k1.size()) || !rd(f, k2.data(), k2.size()) || !rd(f, m.data(), m.size())) return 4;
    fclose(f);
    Frame mInitialFrame, mCurrentFrame;
    mInitialFrame.mK = drfe::drfe_detail_sim3::mat32(3, 3, K);
    mCurrentFrame.mK = mInitialFrame.mK;
    keys_of(mInitialFrame, k1);
    keys_of(mCurrentFrame, k2);
    std::vector<int> mvIniMatches(m.begin(), m.end());
    int nmatches = 0;
    for (int v : mvIniMatches) nmatches += v >= 0;

    Planar_SLAM::Initializer<Frame> initializer(mInitialFrame, sigma, iterations);
    Planar_SLAM::Initializer<Frame>* mpInitializer = &initializer;
    mpInitializer->SetSeed(seed);
    if (mode == "device") mpInitializer->UseDevice(true);
    if (mode == "host") mpInitializer->UseDevice(false);
    drfe_cv::Mat Rcw, tcw;
    std::vector<bool> vbTriangulated;
    std::vector<Point3f> mvIniP3D;
    const bool ok = mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated);
    if (ok)
        for (size_t i = 0, iend = mvIniMatches.size(); i < iend; i++)
            if (mvIniMatches[i] >= 0 && !vbTriangulated[i]) {
                mvIniMatches[i] = -1;
                nmatches--;
            }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    const int32_t head[4] = {ok ? 1 : 0, mpInitializer->Branch(), mpInitializer->Flags(), nmatches};
    float Rt[12] = {0};
    if (!Rcw.empty())
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Rt[r * 3 + c] = Rcw.ptr<float>(r)[c];
    if (!tcw.empty())
        for (int r = 0; r < 3; r++) Rt[9 + r] = tcw.ptr<float>(r)[0];
    fwrite(head, sizeof(head), 1, o);
    fwrite(Rt, sizeof(Rt), 1, o);
    const int32_t np = (int32_t)mvIniP3D.size();
    fwrite(&np, sizeof(np), 1, o);
    for (const Point3f& p : mvIniP3D) fwrite(&p, sizeof(float), 3, o);
    for (bool b : vbTriangulated) fputc(b ? 1 : 0, o);
    for (int v : mvIniMatches) {
        const int32_t w = v;
        fwrite(&w, sizeof(w), 1, o);
    }
    fclose(o);
    printf("initializer_caller ok: mode %s, ok %d, branch %d, %d matches kept\n", mode.c_str(), ok ? 1 : 0, head[1], nmatches);
    return 0;
}
