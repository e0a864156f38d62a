/* kfdb_core.h — the arithmetic of KeyFrameDatabase's two queries (reference src/KeyFrameDatabase.cc:76-309) and of DBoW2's
 * L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), once, for kfdb.cpp and kfdb_kernels.hip.  DESIGN.md
 * section 23.  No product feeds a sum: nothing for a compiler to contract. */
#ifndef DRFE_KFDB_CORE_H
#define DRFE_KFDB_CORE_H

#include "../../include/drfe_math.h"
#include <math.h>
#include <stdint.h>

#define KFDB_NEIGHBOURS 10

/* One sorted-merge walk over a query vector and a stored one: the number of common words (mnLoopWords / mnRelocWords once the
 * inverted file has been walked), the smallest of them (-1 when there is none: the word at which the key frame is first met) and
 * L1Scoring::score's double sum in ascending word id, query value first.  lower_bound of the reference lands where single steps do. */
DRFE_HD void kfdb_walk(const int32_t* qi, const double* qv, int nq, const int32_t* ki, const double* kv, int nk, int32_t* count,
                       int32_t* first, double* sum)
{
    int a = 0, b = 0;
    int32_t c = 0, f = -1;
    double s = 0.0;
    while (a < nq && b < nk) {
        const int32_t wa = qi[a], wb = ki[b];
        if (wa == wb) {
            const double vi = qv[a], wi = kv[b];
            s += fabs(vi - wi) - fabs(vi) - fabs(wi);
            if (c == 0) f = wa;
            c++;
            a++;
            b++;
        } else if (wa < wb) {
            a++;
        } else {
            b++;
        }
    }
    *count = c;
    *first = f;
    *sum = s;
}

/* score = -score / 2.0, narrowed where TemplatedVocabulary::score's double lands in a float */
DRFE_HD float kfdb_score(double sum) { return (float)(-sum / 2.0); }

/* int minCommonWords = maxCommonWords * 0.8f */
DRFE_HD int32_t kfdb_min_common(int32_t maxCommonWords) { return (int32_t)((float)maxCommonWords * 0.8f); }

/* the order in which the inverted file is walked meets key frames: (smallest shared word, sequence number of the latest add) */
DRFE_HD int kfdb_before(int32_t firstA, int64_t seqA, int32_t firstB, int64_t seqB)
{
    return firstA < firstB || (firstA == firstB && seqA < seqB);
}

/* The covisibility accumulation of one kept key frame (:148-170, :262-284): look(slot, &score) says whether neighbour `slot` passes
 * the query's neighbour test and with which mLoopScore / mRelocScore.  float sums in neighbour order, the best changes on strict >. */
template <class Look>
DRFE_HD void kfdb_accumulate(float si, int32_t self, const int32_t* nbr, Look& look, float* acc, int32_t* best)
{
    float bestScore = si, a = si;
    int32_t b = self;
    for (int k = 0; k < KFDB_NEIGHBOURS; k++) {
        const int32_t nb = nbr[k];
        if (nb < 0) continue;
        float s;
        if (!look(nb, &s)) continue;
        a += s;
        if (s > bestScore) {
            b = nb;
            bestScore = s;
        }
    }
    *acc = a;
    *best = b;
}

/* float minScoreToRetain = 0.75f * bestAccScore */
DRFE_HD float kfdb_retain(float bestAcc) { return 0.75f * bestAcc; }

#endif
