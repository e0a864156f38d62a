/* ransac_table.h — what the RANSAC solvers (sim3.cpp, pnp.cpp) share on the host: a call is a table of rows, one per hypothesis,
 * a solver's rows contiguous; the caller's table has a solver's cap of rows, the compact one of a call only those that run.  Here:
 * the iteration count, the sampling, the plan of where a solver's rows lie in both tables and the head of a solver's device record;
 * the buffers and the ends of a batch entry are batch_entry.h's.  A solver keeps its argument checks, its records and its rows.
 * Host only; DESIGN.md section 16. */
#ifndef DRFE_RANSAC_TABLE_H
#define DRFE_RANSAC_TABLE_H

#include "batch_entry.h"
#include "glibc_rand.h"

#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

/* the end of SetRansacParameters (Sim3Solver.cc:118-142, PnPsolver.cc:139-152): the count in double through the host's libm,
 * int conversion as cvttsd2si (NaN and out-of-range give INT_MIN), clamped to [1, maxIterations] */
inline int ransac_iteration_count(bool single, float epsilon, double probability, int maxIterations)
{
    int nIterations = 1;
    if (!single) {
        const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
        nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
    }
    const int m = nIterations < maxIterations ? nIterations : maxIterations;
    return m > 1 ? m : 1;
}

/* one iteration's sample (Sim3Solver.cc:167-181, PnPsolver.cc:188-201): K RandomInt draws from a list that shrinks by
 * swap-with-back */
template <int K>
void ransac_draw_sample(GlibcRand& rng, std::vector<int32_t>& avail, int N, int32_t out[K])
{
    /* vAvailableIndices = mvAllIndices: only the entries a previous iteration touched differ from the identity */
    int size = N;
    int touched[K];
    for (int q = 0; q < K; q++) {
        const int randi = rng.random_int(0, size - 1);
        out[q] = avail[(size_t)randi];
        avail[(size_t)randi] = avail[(size_t)size - 1];
        touched[q] = randi;
        size--;
    }
    for (int q = 0; q < K; q++) avail[(size_t)touched[q]] = touched[q];
}

/* solver s of a call's offsets table: it starts at 0, does not decrease and gives no solver more than maxCorr (named capName in
 * the message) correspondences.  A table that does not start at 0 leaves err as the caller set it. */
inline bool ransac_offsets_ok(const int32_t* offsets, int s, int maxCorr, const char* name, const char* capName, std::string& err)
{
    if (s == 0 && offsets[0] != 0) return false;
    const int64_t N = (int64_t)offsets[s + 1] - offsets[s];
    if (N < 0) { err = std::string(name) + ": decreasing offsets"; return false; }
    if (N > maxCorr) { err = std::string(name) + ": more than " + capName + " correspondences in a solver"; return false; }
    return true;
}

/* what every solver's device record says about its place in the compact table */
struct RansacSolverHead {
    int32_t minInliers;            /* as the walk over the counts compares it */
    int32_t n, corr0;              /* correspondences: count, first */
    int32_t hyp, hyp0;             /* rows: count, first (compact over the call) */
    int32_t words;                 /* mask words per row */
    int64_t mask0;                 /* first mask word (compact over the call) */
};
static_assert(sizeof(RansacSolverHead) == 32 && alignof(RansacSolverHead) == 8, "six int32 and an aligned int64, no padding");

/* where a solver's rows lie in the caller's table and in the compact one of a call; K correspondences a sample */
template <int K, int MaxCorr>
struct RansacPlan {
    std::vector<int32_t> iterations, hyp, hyp0, words, row0;
    std::vector<int64_t> mask0Out, mask0;  /* the caller's (cap rows), the compact one (hyp rows) */
    std::vector<int32_t> sample;           /* K per row, compact */
    std::vector<int32_t> avail;            /* ransac_draw_sample's list, the identity between draws */
    int nHyp = 0, maxHyp = 0, rows = 0;
    int64_t maskWords = 0, maskWordsOut = 0;

    RansacPlan() : avail((size_t)MaxCorr)
    {
        for (int i = 0; i < MaxCorr; i++) avail[(size_t)i] = i;
    }

    /* the next solver: N correspondences, h rows that run of the cap the caller's table holds, their samples drawn from seed */
    void add_solver(int N, int it, int h, int cap, uint32_t seed)
    {
        const int w = (N + 63) / 64;
        const size_t first = (size_t)nHyp;
        iterations.push_back(it); hyp.push_back(h); hyp0.push_back(nHyp); words.push_back(w); row0.push_back(rows);
        mask0.push_back(maskWords); mask0Out.push_back(maskWordsOut);
        nHyp += h;
        rows += cap;
        maskWords += (int64_t)h * w;
        maskWordsOut += (int64_t)cap * w;
        if (h > maxHyp) maxHyp = h;
        if (h > 0) {
            GlibcRand rng(seed);
            sample.resize(K * (size_t)nHyp);
            for (int q = 0; q < h; q++) ransac_draw_sample<K>(rng, avail, N, &sample[K * (first + q)]);
        }
    }

    const int32_t* sample_of(int s, int h) const { return &sample[K * ((size_t)hyp0[(size_t)s] + h)]; }

    /* solver s's hyp * per elements from the compact array of a call (at hyp0) to the caller's (at row0); its mask rows */
    template <class T>
    void scatter(int s, T* dst, const T* src, size_t per = 1) const
    {
        const size_t i = (size_t)s;
        if (hyp[i]) std::memcpy(dst + per * (size_t)row0[i], src + per * (size_t)hyp0[i], per * (size_t)hyp[i] * sizeof(T));
    }
    void scatter_mask(int s, uint64_t* dst, const uint64_t* src) const
    {
        const size_t i = (size_t)s;
        if (hyp[i]) std::memcpy(dst + mask0Out[i], src + mask0[i], (size_t)hyp[i] * (size_t)words[i] * sizeof(uint64_t));
    }

    RansacSolverHead head(int s, const int32_t* offsets, int minInliers) const
    {
        const size_t i = (size_t)s;
        return RansacSolverHead{minInliers, offsets[s + 1] - offsets[s], offsets[s], hyp[i], hyp0[i], words[i], mask0[i]};
    }
    void fill_hyp_solver(int32_t* hypSolver) const
    {
        for (size_t s = 0; s < hyp.size(); s++)
            for (int q = 0; q < hyp[s]; q++) hypSolver[hyp0[s] + q] = (int32_t)s;
    }

    /* the counters every solver keeps: [0] calls, [1] solvers, [2] rows, [3] correspondences, [7] solvers without a row */
    void count_call(int64_t stats[8], const int32_t* offsets) const
    {
        stats[0]++;
        if (hyp.empty()) return;
        stats[1] += (int64_t)hyp.size();
        stats[2] += nHyp;
        stats[3] += offsets[hyp.size()];
        for (const int32_t h : hyp)
            if (!h) stats[7]++;
    }
};

#endif
