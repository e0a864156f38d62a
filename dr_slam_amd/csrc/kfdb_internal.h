/* kfdb_internal.h — what kfdb.cpp hands to kfdb_kernels.hip. */
#ifndef DRFE_KFDB_INTERNAL_H
#define DRFE_KFDB_INTERNAL_H

#include "drfe_internal.h"
#include "kfdb_core.h"

/* threads of a query's workgroup: key frames (stage 1) and kept entries (stages 4-6) go across them */
#define KFDB_THREADS 256

/* bits of KfdbLaunch::flag */
enum { KFDB_F_CONNECTED = 1, KFDB_F_LISTED = 2, KFDB_F_SCORED = 4 };

/* per-query record of the device path, written by k_kfdb_count and finished by k_kfdb_select */
struct KfdbQueryRec {
    int32_t listed, scored, kept, maxCommon;
    int32_t minCommon, nCand, uninit, pad;
    float minScore, pad2;
};

/* One call.  Key frames are slots 0 .. nSlots of the resident tables; everything per (query, slot) is [query * nSlots + slot]. */
struct KfdbLaunch {
    int nQueries, nSlots, reloc;
    /* resident */
    const int32_t* wordOff;        /* nSlots + 1: slot s holds words [wordOff[s], wordOff[s + 1]) (none for a free slot) */
    const int32_t* wordIds;
    const double* wordVals;
    const int32_t* nbr;            /* nSlots x 10 slots, -1 = none */
    float* relocScore;             /* nSlots: mRelocScore */
    uint8_t* relocWritten;         /* nSlots: a query has written it */
    /* per call */
    const int64_t* seq;            /* nSlots: sequence number of the latest add, -1 = not in the inverted file during this call */
    const int32_t* from;           /* nSlots: first query of the call that sees the slot (add_after of query from - 1) */
    const int32_t* qOff;           /* nQueries + 1: the queries' vectors */
    const int32_t* qIds;
    const double* qVals;
    const int32_t* connOff;        /* loop: nQueries + 1, connected slots */
    const int32_t* conn;
    const int32_t* covOff;         /* loop: nQueries + 1, covisible slots (an empty range where min_score was given) */
    const int32_t* cov;
    const float* minScoreIn;       /* loop: nQueries */
    const uint8_t* useCov;         /* loop: nQueries, minScore is computed from cov */
    /* scratch, per (query, slot) */
    int32_t* cnt;
    int32_t* first;
    float* score;
    uint8_t* flag;                 /* zero before the launch */
    int32_t* minEntry;             /* 0x7f7f7f7f before the launch */
    int32_t* keptTmp;
    int32_t* keptOrd;
    float* acc;
    int32_t* best;
    int32_t* cand;
    /* out */
    KfdbQueryRec* rec;             /* nQueries */
    int32_t* candOff;              /* nQueries + 1 */
    int32_t* candPacked;           /* nQueries * nSlots */
};
hipError_t drfe_launch_kfdb(const KfdbLaunch& L, hipStream_t s);

#endif
