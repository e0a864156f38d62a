/* lmap_internal.h — what lmap.cpp hands to lmap_kernels.hip. */
#ifndef DRFE_LMAP_INTERNAL_H
#define DRFE_LMAP_INTERNAL_H

#include "drfe_internal.h"
#include "lmap_core.h"

/* threads of a workgroup: frame points and key-frame slots go across them in the vote, the entries of a match row in the gather */
#define LMAP_THREADS 256
/* stored key frames up to which a query's vote histogram is in LDS (32 KiB of the CU's 160 KiB) */
#define LMAP_LDS_KFS 8192
/* entries of one key frame's match row that a gather workgroup takes per pass */
#define LMAP_GATHER_ENTRIES LMAP_THREADS
/* gather workgroups per query: workgroup b takes the local key frames b, b + LMAP_GATHER_ROWS, ... */
#define LMAP_GATHER_ROWS 64

/* per query, written by k_lmap_vote, finished by k_lmap_scan */
struct LmapQueryRec {
    int32_t nKf, refKf;
    int32_t rec[4];
    int32_t nItems[2];             /* local points, local lines */
    int32_t nNulled, pad[3];
};

/* One chunk of a call: queries 0 .. nQ of the staged block.  Everything per (query, x) is [query * stride + x]. */
struct LmapLaunch {
    LmapImage I;                   /* resident */
    int32_t nQ;
    int32_t rowK;                  /* entries of a query's row of list / cnt: stored key frames or the longest prev_kfs list */
    int32_t rowStride[2];          /* lmap_walk_rank's stride for points, lines: above every match-row length */
    int32_t markWords;             /* (nK + 31) / 32 */
    /* per call, staged */
    const int32_t* ptOff;          /* nQ + 1, from 0 */
    const int32_t* pts;            /* point slots, -1 = null */
    const int32_t* lnOff;          /* nQ + 1 */
    const int32_t* lns;
    const int32_t* prevOff;        /* nQ + 1 */
    const int32_t* prev;           /* key-frame slots */
    /* scratch */
    int32_t* hist;                 /* nQ x nK, zero before the launch; unused while nK <= LMAP_LDS_KFS */
    uint32_t* mark;                /* nQ x markWords */
    int32_t* list;                 /* nQ x rowK: the local key frames */
    int32_t* cnt[2];               /* nQ x rowK: kept entries of each local key frame, then their exclusive prefix */
    int32_t* claim[2];             /* nQ x nP, nQ x nL: LMAP_NO_CLAIM bytes before the launch */
    uint8_t* inFrame[2];           /* nQ x nP, nQ x nL: zero before the launch */
    int32_t* nulledTmp;            /* ptOff[nQ] */
    /* out */
    LmapQueryRec* rec;             /* nQ */
    int32_t* off[4];               /* nQ + 1 each: local key frames, points, lines, nulled */
    int32_t* packedKf;             /* nQ x rowK */
    int32_t* packedItem[2];        /* nQ x nP, nQ x nL */
    uint8_t* packedIn[2];
    int32_t* packedNulled;         /* ptOff[nQ] */
};
hipError_t drfe_launch_lmap(const LmapLaunch& L, hipStream_t s);

#endif
