/* lines_3d.cpp — Frame::isLineGood (reference src/Frame.cc:481-558) and the 3-D line lifting helpers it calls
 * (src/LineExtractor.cpp: depthStdDev :1180, compPt3dCov :1196, extract3dline_mahdist :1266, verify3dLine :1362,
 * mah_dist3d_pt_line :1419, computeLine3d_svd :1157, projectPt3d2Ln3d :278).  SURVEY.md row a-8: <= 40 lines x
 * <= 51 samples of double arithmetic with a rand()-driven RANSAC — the single-frame host entry.
 *
 * What the reference really computes.  isLineGood receives mK, a CV_32F matrix, and compPt3dCov reads it with
 * K.at<double>(0,0): the eight bytes of (fx, 0.0f) reinterpreted as a double are a subnormal ~5.6e-315, so
 * J0(0,0) = z / f overflows to +inf for every valid depth, J0 * diag(1,1,sigma^2) * J0^T contains inf * 0 = NaN in
 * every row and column, cv::SVD of it has NaN singular values, every Mahalanobis distance is NaN, `dist < 1.5` is
 * never true, no sample is an inlier and the line is rejected: the shipped function leaves mvDepthLine = -1 and
 * mvLines3D = 0 for every line.  k_as_f64 = 0 reproduces exactly that by doing the same arithmetic on the same
 * bytes (nothing is hard-coded); k_as_f64 = 1 runs the algorithm as it was evidently meant, with f = fx.  In that
 * mode the two cv::SVD calls are replaced by a symmetric 3x3 eigen-solve (the Mahalanobis distance is invariant
 * to the sign and order of the singular vectors), so results agree with an OpenCV build to rounding, not to the
 * bit, and the endpoint order (A, B) may be swapped; rand() is glibc's TYPE_3 generator restated, seeded per call
 * because the reference shares the process-wide state between its extraction threads.
 * The arithmetic is line3d_core.h's, shared with the batch entry's kernels (lines_3d_batch.cpp). */
#include "line3d_core.h"
#include "glibc_rand.h"

#include <vector>

namespace {

/* verify3dLine, :1362-1417: the inliers must populate more than 7 of the 10 cells between their extremities */
bool verify_3d_line(const std::vector<L3Point>& pts, const L3P& A, const L3P& B)
{
    L3Extremes e;
    for (int i = 0; i < (int)pts.size(); i++) l3_extremes_step(e, i, l3_dot(pts[i].pos - A, B - A));
    L3Cells g;
    if (!l3_cells_begin(pts[e.lo].pos, pts[e.hi].pos, A, B, &g)) return false;
    int cells[10] = {0};
    for (const L3Point& p : pts) cells[l3_cell_of(g, p.pos)] += 1;
    int populated = 0;
    for (int c : cells)
        if (c > 0) populated++;
    return l3_cells_pass(populated);
}

/* computeLine3d_svd, :1157-1178: mean and principal direction of the selected points */
void compute_line3d(const std::vector<L3Point>& pts, const std::vector<int>& idx, L3P& mean, L3P& drct)
{
    mean = {0, 0, 0};
    for (int i : idx) mean = mean + pts[i].pos;
    mean = l3_mean(mean, (int)idx.size());
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int i : idx) l3_scatter_add(s, pts[i].pos - mean);
    drct = l3_direction(s);
}

struct Line3d { L3P A{0, 0, 0}, B{0, 0, 0}; int nInliers = 0; };

/* extract3dline_mahdist, :1266-1360 */
Line3d extract_3d_line(const std::vector<L3Point>& pts, GlibcRand& rng)
{
    const int n = (int)pts.size();
    const int maxIterNo = l3_max_iterations(n);
    std::vector<int> indexes(n);
    for (int i = 0; i < n; i++) indexes[i] = i;
    std::vector<int> maxInlierSet;
    L3P bestA{0, 0, 0}, bestB{0, 0, 0};
    for (int iter = 0; iter < maxIterNo; iter++) {
        /* random_unique(begin, end, 2), include/LSDextractor.h:241-251: two Fisher-Yates steps */
        for (int k = 0; k < 2; k++) std::swap(indexes[k], indexes[l3_swap_with(k, rng.next(), n)]);
        const L3Point& A = pts[indexes[0]];
        const L3Point& B = pts[indexes[1]];
        if (l3_norm(B.pos - A.pos) < L3_EPS) continue;
        std::vector<int> inlierSet;
        for (int i = 0; i < n; i++)
            if (l3_is_inlier(pts[i], A.pos, B.pos)) inlierSet.push_back(i);
        if (inlierSet.size() > maxInlierSet.size()) {
            std::vector<L3Point> inlierPts(inlierSet.size());
            for (size_t ii = 0; ii < inlierSet.size(); ii++) inlierPts[ii] = pts[inlierSet[ii]];
            if (verify_3d_line(inlierPts, A.pos, B.pos)) {
                maxInlierSet = inlierSet;
                bestA = A.pos; bestB = B.pos;
            }
        }
        if (l3_enough((int)maxInlierSet.size(), n)) break;
    }
    Line3d rl;
    if (maxInlierSet.size() >= 2) {
        L3P m = (bestA + bestB) * 0.5, d = bestB - bestA;
        while (true) {   /* refit on the inliers and reselect while the set grows */
            std::vector<int> tmp;
            L3P tm, td;
            compute_line3d(pts, maxInlierSet, tm, td);
            for (int i = 0; i < n; i++)
                if (l3_is_inlier(pts[i], tm, tm + td)) tmp.push_back(i);
            if (tmp.size() > maxInlierSet.size()) { maxInlierSet = tmp; m = tm; d = td; }
            else break;
        }
        L3Extremes e;
        for (size_t i = 0; i < maxInlierSet.size(); i++) l3_extremes_step(e, (int)i, l3_dot(pts[maxInlierSet[i]].pos - m, d));
        rl.A = pts[maxInlierSet[e.lo]].pos;
        rl.B = pts[maxInlierSet[e.hi]].pos;
    }
    rl.nInliers = (int)maxInlierSet.size();
    return rl;
}

} // namespace

extern "C" int drfe_lines_is_good(const drfe_keyline* lines, int n, const float* depth, int w, int h, size_t stride,
                                  const float* K, int k_as_f64, float cx, float cy, float invfx, float invfy,
                                  uint32_t seed, float* depth_line, double* lines3d, int32_t* n_inliers, int* n_good)
{
    if (n < 0 || (n && (!lines || !depth_line || !lines3d)) || !depth || !K || w < 1 || h < 1 || stride < (size_t)w)
        return DRFE_ERR_INVALID;
    const double f = l3_focal(K, k_as_f64);
    GlibcRand rng(seed);
    int good = 0;
    for (int i = 0; i < n; i++) {
        depth_line[i] = -1.0f;
        for (int k = 0; k < 6; k++) lines3d[6 * i + k] = 0.0;
        if (n_inliers) n_inliers[i] = 0;
        const drfe_keyline& kl = lines[i];
        double len;
        const int numSmp = l3_num_samples(kl, &len);
        if (!numSmp) continue;                         /* a sub-pixel line: the reference divides 0 by 0 here */
        std::vector<L3P> pts3d;
        for (int j = 0; j <= numSmp; ++j) {
            L3P p;
            if (l3_sample(kl, j, numSmp, depth, w, h, stride, cx, cy, invfx, invfy, &p)) pts3d.push_back(p);
        }
        if (pts3d.size() < L3_MIN_POINTS) continue;
        std::vector<L3Point> rnd;
        rnd.reserve(pts3d.size());
        for (const L3P& p : pts3d) rnd.push_back(l3_comp_pt3d_cov(p, f));
        const Line3d ln = extract_3d_line(rnd, rng);
        if (n_inliers) n_inliers[i] = ln.nInliers;
        if (l3_accept(ln.nInliers, len, ln.A, ln.B)) {
            depth_line[i] = l3_end_point_depth(kl, depth, w, h, stride);
            lines3d[6 * i + 0] = ln.A.x; lines3d[6 * i + 1] = ln.A.y; lines3d[6 * i + 2] = ln.A.z;
            lines3d[6 * i + 3] = ln.B.x; lines3d[6 * i + 4] = ln.B.y; lines3d[6 * i + 5] = ln.B.z;
            good++;
        }
    }
    if (n_good) *n_good = good;
    return DRFE_OK;
}
