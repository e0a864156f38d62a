/* map_upkeep_internal.h — the records map_upkeep.cpp stages for map_upkeep_kernels.hip. */
#ifndef DRFE_MAP_UPKEEP_INTERNAL_H
#define DRFE_MAP_UPKEEP_INTERNAL_H

#include "drfe_internal.h"

/* descriptor buckets by row count: four lanes per item, sixteen lanes, one wavefront, one workgroup (rows in LDS) */
enum { MU_B4 = 0, MU_B16, MU_B64, MU_BWG, MU_BUCKETS };
enum { MU_ACTIVE = 1,          /* not bad, observations present: the normal half runs (with DRFE_UPKEEP_NORMAL) */
       MU_HAS_ROWS = 2,        /* the descriptor half runs (DRFE_UPKEEP_DESCRIPTOR, rows of non-bad keyframes present) */
       MU_DEVICE_DESC = 4 };   /* ... on the device (else best / desc are written by the host after the copy back) */

/* one item: observations [obs0, obs0 + nobs) of the call, descriptor rows [row0, row0 + nrows) of the staged rows */
struct MuItem { int32_t obs0, nobs, row0, nrows, refKf, level, flags, pad; };

struct MuLaunch {
    const MuItem* items;
    int n, what, line, nLevels;
    const float *kfCenter, *scale;
    const void* world;                 /* float[3] / double[6] per item */
    const int32_t* obsKf;
    const uint4* rows;                 /* 32 bytes per staged row */
    const int32_t* rowObs;             /* the row's index in its item's observation list */
    const int32_t* list[MU_BUCKETS];   /* items of each bucket */
    int count[MU_BUCKETS];
    int maxRowsWg;                     /* largest row count of the workgroup bucket (its LDS) */
    int32_t* best;
    uint4* desc;                       /* 32 bytes per item */
    uint8_t* status;
    void* normal;                      /* float[3] / double[3] per item */
    float *maxD, *minD;
    void* frustum;                     /* drfe_frustum_point / drfe_frustum_line per item, or NULL */
};
hipError_t drfe_launch_map_upkeep(const MuLaunch& L, hipStream_t s);
void drfe_map_upkeep_free(drfe_ctx* c);

#endif
