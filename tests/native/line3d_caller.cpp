/* line3d_caller.cpp - drfe::Line3DBatch (include/drfe_adaptor.hpp) as a tracking front end would call it after extracting the
 * lines of a batch of frames: Frame-like objects with mvKeylinesUn, mK and the intrinsics, one CV_32F depth image each.  The same
 * frames are filled twice - through the device entry (deviceFrom = 1) and through the host entry (deviceFrom above the batch) -
 * and must agree byte for byte, in the intended mode and as shipped; prints "line3d_caller ok". */
#include "drfe_adaptor.hpp"

#include <cstdio>
#include <cstring>

struct Vector6d {
    double v[6] = {0, 0, 0, 0, 0, 0};
    double& operator()(int i) { return v[i]; }
};

struct Frame {
    std::vector<drfe_cv::KeyLine> mvKeylinesUn;
    drfe_cv::Mat mK;
    float cx, cy, invfx, invfy;
    std::vector<float> mvDepthLine;
    std::vector<Vector6d> mvLines3D;
};

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main()
{
    const int W = 160, H = 120, B = 9;
    const float fx = 200.f, K[9] = {fx, 0, 80, 0, fx, 60, 0, 0, 1};
    std::vector<Frame> frames(B);
    std::vector<drfe_cv::Mat> depth;
    std::vector<uint32_t> seeds;
    uint32_t s = 7;
    for (int f = 0; f < B; f++) {
        drfe_cv::Mat d(H, W, 4);                       /* a wall with a step, noise, a tenth of the pixels pushed back, a hole */
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                float z = x < 100 ? 2.f + 0.002f * x : 4.f;
                z += ((int)(lcg(s) % 401) - 200) * 1e-4f;
                if (lcg(s) % 10 == 0) z += 0.2f + (lcg(s) % 800) * 1e-3f;
                if (y >= 95 && y < 111 && x >= 30 && x < 36) z = 0.f;
                d.ptr<float>(y)[x] = z;
            }
        depth.push_back(d);
        Frame& F = frames[f];
        F.mK = drfe_cv::Mat(3, 3, 4);
        std::memcpy(F.mK.data, K, sizeof K);
        F.cx = 80; F.cy = 60; F.invfx = 1.f / fx; F.invfy = 1.f / fx;
        const int n = f == 4 ? 0 : 3 + 4 * f;           /* an empty frame among full ones */
        for (int i = 0; i < n; i++) {
            drfe_cv::KeyLine k = {};
            k.startPointX = (float)(lcg(s) % 1500) * 0.1f; k.startPointY = (float)(lcg(s) % 1100) * 0.1f;
            k.endPointX = k.startPointX + (float)(lcg(s) % 900) * 0.1f - 20.f; k.endPointY = k.startPointY + (float)(lcg(s) % 300) * 0.1f - 15.f;
            k.class_id = i;
            F.mvKeylinesUn.push_back(k);
        }
        seeds.push_back(1 + f);
    }
    int total[2] = {0, 0};
    for (int kAsF64 = 1; kAsF64 >= 0; kAsF64--) {
        std::vector<Frame> dev = frames, host = frames;
        std::vector<Frame*> pd, ph;
        for (int f = 0; f < B; f++) { pd.push_back(&dev[f]); ph.push_back(&host[f]); }
        drfe::Line3DBatch onDevice(0, 1, kAsF64), onHost(0, B + 1, kAsF64);
        const int gd = onDevice.Fill(pd, depth, &seeds), gh = onHost.Fill(ph, depth, &seeds);
        if (gd != gh) { std::printf("accepted lines differ: %d / %d\n", gd, gh); return 1; }
        for (int f = 0; f < B; f++) {
            const size_t n = frames[f].mvKeylinesUn.size();
            if (dev[f].mvDepthLine.size() != n || host[f].mvLines3D.size() != n || dev[f].mvLines3D.size() != n ||
                (n && (std::memcmp(dev[f].mvDepthLine.data(), host[f].mvDepthLine.data(), n * sizeof(float)) ||
                       std::memcmp(dev[f].mvLines3D.data(), host[f].mvLines3D.data(), n * sizeof(Vector6d))))) {
                std::printf("frame %d differs (k_as_f64 = %d)\n", f, kAsF64);
                return 1;
            }
        }
        total[kAsF64] = gd;
    }
    if (total[1] < 10 || total[0] != 0) { std::printf("accepted %d lines as intended, %d as shipped\n", total[1], total[0]); return 1; }
    std::printf("line3d_caller ok: %d lines accepted in %d frames\n", total[1], B);
    return 0;
}
