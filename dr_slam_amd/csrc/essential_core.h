/* essential_core.h — what surrounds the solver of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2910-3131), once,
 * for lmap_essential.cpp and essential_kernels.hip.  DESIGN.md section 35.  g2o::Sim3 is sim3_opt_core.h's restatement, the pose
 * pieces are correct_core.h's and UpdateNormalAndDepth is map_upkeep_core.h's: plain IEEE add / mul / div / sqrt, compiled with
 * -ffp-contract=off on both sides.
 *
 * Key frames are slots in rank order (the iteration order of set<KeyFrame*>); every `mnId <` of the reference is a comparison of
 * handles.  A unit of the edge builder is one row of LoopConnections (the leading segment) or one key frame of the map. */
#ifndef DRFE_ESSENTIAL_CORE_H
#define DRFE_ESSENTIAL_CORE_H

#include "correct_core.h"

/* const int minFeat = 100 */
#define ESS_MIN_FEAT 100
/* drfe_lmap_essential_edges_call.kind */
enum { ESS_KIND_LOOP_CONNECTION = 0, ESS_KIND_SPANNING_TREE = 1, ESS_KIND_LOOP_EDGE = 2, ESS_KIND_COVISIBILITY = 3 };

/* the stored loop edges by slot, next to LmapImage: the known members of mspLoopEdges in ascending slot (rank order) */
struct EssImage {
    const int32_t* leOff;          /* nK + 1 */
    const int32_t* le;
};

/* the four Sim3s a vertex lends to its edges: vScw and its inverse (loop connections), and the non-corrected one where the table
 * has it, else vScw again, with its inverse (the normal edges) */
struct EssKf {
    SoSim3 scw, scwInv, snw, snwInv;
};

/* both Sim3s a key frame lends to the points of the commit: vScw and vCorrectedSwc; a default-constructed pair where the
 * reference's vectors were never written */
struct EssMove {
    SoSim3 scw, swc;
};

DRFE_HD void ess_identity(SoSim3& S)
{
    S.q[0] = 0.0; S.q[1] = 0.0; S.q[2] = 0.0; S.q[3] = 1.0;
    S.t[0] = 0.0; S.t[1] = 0.0; S.t[2] = 0.0;
    S.s = 1.0;
}

/* position of v in the ascending row [a, a + n), or -1 */
DRFE_HD int32_t ess_find(const int32_t* a, int32_t n, int32_t v)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && a[lo] == v ? lo : -1;
}

/* first position of the ascending 64-bit row that is not below v */
DRFE_HD int32_t ess_lower64(const uint64_t* a, int32_t n, uint64_t v)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* pKF->GetWeight(other) from the weights row of slot i (ascending slot): 0 when absent */
DRFE_HD int32_t ess_weight(const int32_t* wOff, const int32_t* wKf, const int32_t* wW, int32_t i, int32_t other)
{
    const int32_t o = wOff[i], k = ess_find(wKf + o, wOff[i + 1] - o, other);
    return k < 0 ? 0 : wW[o + k];
}

/* :2971 turned round: the member j of key i gets its edge */
DRFE_HD bool ess_lc_kept(const int32_t* wOff, const int32_t* wKf, const int32_t* wW, int32_t i, int32_t j, int32_t cur, int32_t loop)
{
    return (i == cur && j == loop) || ess_weight(wOff, wKf, wW, i, j) >= ESS_MIN_FEAT;
}

/* an unordered pair of slots as one key; (min, max) of the handles names the same pair */
DRFE_HD uint64_t ess_pair(int32_t a, int32_t b)
{
    const uint32_t lo = (uint32_t)(a < b ? a : b), hi = (uint32_t)(a < b ? b : a);
    return ((uint64_t)lo << 32) | hi;
}

/* sInsertedEdges.count(pair): pairKey is every entry of LoopConnections as a pair key, ascending, pairI / pairJ its key and member;
 * the pair is in the set exactly when one of its entries was kept */
DRFE_HD bool ess_inserted(const uint64_t* pairKey, const int32_t* pairI, const int32_t* pairJ, int32_t nPairs, const int32_t* wOff,
                          const int32_t* wKf, const int32_t* wW, int32_t a, int32_t b, int32_t cur, int32_t loop)
{
    const uint64_t key = ess_pair(a, b);
    for (int32_t e = ess_lower64(pairKey, nPairs, key); e < nPairs && pairKey[e] == key; e++)
        if (ess_lc_kept(wOff, wKf, wW, pairI[e], pairJ[e], cur, loop)) return true;
    return false;
}

/* GetCovisiblesByWeight(100)'s length from the first ordered entry below 100 (`first`, the row length when there is none): the
 * whole row comes back empty, upper_bound having returned end() (src/KeyFrame.cc:268-270) */
DRFE_HD int32_t ess_prefix(int32_t first, int32_t len) { return first == len ? 0 : first; }

/* :3055-3058 of the prefix entry `other` of key frame i */
DRFE_HD bool ess_covis_kept(const int32_t* child, int32_t nChild, const int32_t* le, int32_t nLe, const uint8_t* kfBad,
                            const int32_t* kfHandle, int32_t parent, int32_t i, int32_t other)
{
    return other != parent && ess_find(child, nChild, other) < 0 && ess_find(le, nLe, other) < 0 && !kfBad[other] &&
           kfHandle[other] < kfHandle[i];
}

/* the Sim3s of one vertex: corrected / nonCorrected are its rows of the tables or NULL, Tcw its stored pose */
DRFE_HD void ess_vertex(const double* corrected, const double* nonCorrected, const float* Tcw, EssKf& K)
{
    if (corrected) corr_sim3_from8(corrected, K.scw);
    else corr_sim3_of_pose(Tcw, K.scw);
    so_inverse(K.scw, K.scwInv);
    if (nonCorrected) corr_sim3_from8(nonCorrected, K.snw);
    else K.snw = K.scw;
    so_inverse(K.snw, K.snwInv);
}

/* Sji = Sjw * Swi of an edge from i to j */
DRFE_HD void ess_measure(const EssKf& Ki, const EssKf& Kj, int kind, double m[8])
{
    SoSim3 S;
    if (kind == ESS_KIND_LOOP_CONNECTION) so_mul(Kj.scw, Ki.scwInv, S);
    else so_mul(Kj.snw, Ki.snwInv, S);
    corr_sim3_to8(S, m);
}

/* :3093-3103 of one key frame: vCorrectedSwc, the pose toCvSE3(r.toRotationMatrix(), t * (1. / s)) and SetPose's centre */
DRFE_HD void ess_pose(const double optimised[8], SoSim3& swc, float Tiw[16], float Ow[3])
{
    SoSim3 S;
    corr_sim3_from8(optimised, S);
    so_inverse(S, swc);
    double R[3][3];
    mp_quat_to_matrix(S.q, R);
    const double inv = 1.0 / S.s;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Tiw[r * 4 + c] = (float)R[r][c];
        Tiw[r * 4 + 3] = (float)(S.t[r] * inv);
    }
    Tiw[12] = 0.0f; Tiw[13] = 0.0f; Tiw[14] = 0.0f; Tiw[15] = 1.0f;
    camera_centre_kf(Tiw, Ow);
}

/* nIDr of a point (:3111-3117) as a handle */
DRFE_HD int32_t ess_ref_handle(int32_t by, int32_t byRef, int32_t refHandle, int32_t cur) { return by == cur ? byRef : refHandle; }

/* UpdateNormalAndDepth of point p at Xn, every SetPose of the call done: kfOw holds each key frame's centre as it is now.  Returns
 * DRFE_UPKEEP_NORMAL, or 0 when the point has no observations and nothing is computed. */
DRFE_HD uint8_t ess_normal(const CorrImage& G, const float* kfOw, const int32_t* obsOff, const int32_t* obs, int32_t p, const float Xn[3],
                           float nrm[3], float* maxD, float* minD)
{
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
    *maxD = *minD = 0.0f;
    const int32_t o0 = obsOff[p], o1 = obsOff[p + 1];
    if (o1 == o0) return 0;
    for (int32_t o = o0; o < o1; o++) mu_point_obs(nrm, Xn, kfOw + 3 * (size_t)obs[o]);
    mu_point_finish(nrm, o1 - o0, Xn, kfOw + 3 * (size_t)G.mpRef[p], G.scale[G.mpLevel[p]], G.scale[G.nLevels - 1], maxD, minD);
    return DRFE_UPKEEP_NORMAL;
}

#endif
