/* map_upkeep_core.h — the arithmetic of MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (reference
 * src/MapPoint.cc:288-350, 376-411) and MapLine::ComputeDistinctiveDescriptors / UpdateAverageDir (src/MapLine.cpp:241-318,
 * 320-362).  Shared by the host entries (map_upkeep.cpp) and the device kernels (map_upkeep_kernels.hip) so that both produce
 * the same bits; plain IEEE add / mul / div / sqrt, compiled with -ffp-contract=off on both sides.  DESIGN.md section 14. */
#ifndef DRFE_MAP_UPKEEP_CORE_H
#define DRFE_MAP_UPKEEP_CORE_H

#include "../../include/drfe.h"
#include "../../include/drfe_math.h"

#include <stdint.h>

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1712) over the eight 32-bit words of two rows; cv::norm(a, b, NORM_HAMMING)
 * of two 32-byte LBD rows is the same count. */
DRFE_HD int mu_hamming(const uint32_t* a, const uint32_t* b)
{
    int d = 0;
    for (int k = 0; k < 8; k++) d += __builtin_popcount(a[k] ^ b[k]);
    return d;
}

/* The median index of a sorted row of N: vDists[0.5 * (N - 1)], the double truncated by size_t, i.e. floor((N - 1) / 2). */
DRFE_HD int mu_median_rank(int N) { return (N - 1) / 2; }

/* The argmin key of row i: the strictly smaller median wins, and at ties the first row (median <= 256, i < 2^16). */
DRFE_HD uint32_t mu_key(int median, int i) { return ((uint32_t)median << 16) | (uint32_t)i; }

/* One observation of UpdateNormalAndDepth's loop: normali = mWorldPos - Owi (float), then normal = normal + normali / cv::norm(normali)
 * read as MatExpr's scaleAdd: cv::norm is the double sum of squares in order, then sqrt; the scale (float)(1.0 / s); per element
 * normali[k] * scale + normal[k] in float.  A centre equal to the point gives s = 0, scale = inf and 0 * inf = NaN, as OpenCV. */
DRFE_HD void mu_point_obs(float nrm[3], const float X[3], const float Ow[3])
{
    const float v0 = X[0] - Ow[0], v1 = X[1] - Ow[1], v2 = X[2] - Ow[2];
    double s = 0.0;
    s += (double)v0 * (double)v0;
    s += (double)v1 * (double)v1;
    s += (double)v2 * (double)v2;
    const float a = (float)(1.0 / sqrt(s));
    nrm[0] = v0 * a + nrm[0];
    nrm[1] = v1 * a + nrm[1];
    nrm[2] = v2 * a + nrm[2];
}

/* (float)cv::norm(P - Ow) of two float 3-vectors */
DRFE_HD float mu_dist(const float P[3], const float Ow[3])
{
    const float c0 = P[0] - Ow[0], c1 = P[1] - Ow[1], c2 = P[2] - Ow[2];
    double s = 0.0;
    s += (double)c0 * (double)c0;
    s += (double)c1 * (double)c1;
    s += (double)c2 * (double)c2;
    return (float)sqrt(s);
}

/* The tail of UpdateNormalAndDepth: dist = cv::norm(Pos - Ow_ref), mfMaxDistance = dist * scale[level], mfMinDistance = max /
 * scale[nLevels - 1], mNormalVector = normal / n read as convertTo with the float scale (float)(1.0 / n). */
DRFE_HD void mu_point_finish(float nrm[3], int n, const float X[3], const float OwRef[3], float levelScale, float lastScale,
                             float* maxD, float* minD)
{
    const float dist = mu_dist(X, OwRef);
    *maxD = dist * levelScale;
    *minD = *maxD / lastScale;
    const float a = (float)(1.0 / (double)n);
    for (int k = 0; k < 3; k++) nrm[k] = nrm[k] * a;
}

/* One observation of UpdateAverageDir's loop, in double (Eigen): middlePos = 0.5 * (head + tail), normali = middlePos - OWi
 * (the float centre widened), normal = normal + normali / normali.norm() with squaredNorm read ((x x + y y) + z z). */
DRFE_HD void mu_line_obs(double nrm[3], const double P[6], const float Ow[3])
{
    const double m0 = 0.5 * (P[0] + P[3]), m1 = 0.5 * (P[1] + P[4]), m2 = 0.5 * (P[2] + P[5]);
    const double v0 = m0 - (double)Ow[0], v1 = m1 - (double)Ow[1], v2 = m2 - (double)Ow[2];
    const double s = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    nrm[0] = nrm[0] + v0 / s;
    nrm[1] = nrm[1] + v1 / s;
    nrm[2] = nrm[2] + v2 / s;
}

/* The tail of UpdateAverageDir: SP, EP = the endpoints cast to float, MP = 0.5 * (SP + EP) (float (a + b) * 0.5; addWeighted in
 * double rounds the same exact sum once), dist = (float)cv::norm(MP - Ow_ref), max / min as for points,
 * mNormalVector = normal / n in double. */
DRFE_HD void mu_line_finish(double nrm[3], int n, const double P[6], const float OwRef[3], float levelScale, float lastScale,
                            float* maxD, float* minD)
{
    float MP[3];
    for (int k = 0; k < 3; k++) MP[k] = ((float)P[k] + (float)P[k + 3]) * 0.5f;
    const float dist = mu_dist(MP, OwRef);
    *maxD = dist * levelScale;
    *minD = *maxD / lastScale;
    for (int k = 0; k < 3; k++) nrm[k] = nrm[k] / (double)n;
}

#endif
