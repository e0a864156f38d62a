/* sim3_internal.h — the records sim3.cpp stages for sim3_kernels.hip. */
#ifndef DRFE_SIM3_INTERNAL_H
#define DRFE_SIM3_INTERNAL_H

#include "drfe_internal.h"
#include "ransac_table.h"
#include "sim3_core.h"

/* the counting kernel's LDS bound and rows per workgroup (ransac_device.h); a Sim3Corr is 48 bytes */
#define DRFE_SIM3_LDS_CORR 1024
#define DRFE_SIM3_CHUNK 32

/* one solver on the device */
struct Sim3Solver {
    float Tcw1[12], Tcw2[12], K1[4], K2[4];
    int32_t fixScale, pad;
    RansacSolverHead head;         /* minInliers as the caller gave it */
};

struct Sim3Launch {
    const Sim3Solver* solver;
    int nSolvers, nCorr, nHyp, maxHyp; /* maxHyp: the largest hyp of a solver */
    /* in */
    const int32_t* corrSolver;     /* per correspondence */
    const float *Xw1, *Xw2, *sig1, *sig2;
    const int32_t* hypSolver;      /* per hypothesis */
    const int32_t* sample;         /* 3 per hypothesis */
    /* scratch */
    Sim3Corr* corr;
    float* T21;                    /* 12 per hypothesis */
    /* out, compact over the hypotheses of the call */
    float *R12, *t12, *s12, *T12;
    int32_t *inliers, *best;
    uint8_t *returns, *uncertified;
    uint64_t* mask;
};
hipError_t drfe_launch_sim3(const Sim3Launch& L, hipStream_t s);
void drfe_sim3_free(drfe_ctx* c);

#endif
