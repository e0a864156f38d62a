/* pnp_internal.h — the records pnp.cpp stages for pnp_kernels.hip. */
#ifndef DRFE_PNP_INTERNAL_H
#define DRFE_PNP_INTERNAL_H

#include "drfe_internal.h"
#include "ransac_table.h"
#include "pnp_core.h"

/* the counting kernel's LDS bound and rows per workgroup (ransac_device.h); a PnpCorr is 24 bytes */
#define DRFE_PNP_LDS_CORR 2048
#define DRFE_PNP_CHUNK 32

/* one solver on the device */
struct PnpSolverRec {
    double K[4];                   /* fu, fv, uc, vc */
    RansacSolverHead head;         /* minInliers after SetRansacParameters */
};

struct PnpLaunch {
    const PnpSolverRec* solver;
    int nSolvers, nCorr, nHyp, maxHyp; /* maxHyp: the largest hyp of a solver */
    /* in */
    const PnpCorr* corr;
    const int32_t* hypSolver;      /* per row */
    const int32_t* sample;         /* 4 per row */
    /* scratch */
    int32_t* jobs;                 /* per solver, at hyp0: the rows Refine runs over */
    int32_t *jobSolver, *jobRow;   /* the call's compact job list (k_pnp_jobs): solver, row within it */
    int32_t* totalJobs;
    /* out, compact over the rows of the call; zero before the launches */
    double *R, *t, *refR, *refT;   /* 9 and 3 per row */
    int32_t *inliers, *best, *refInliers, *nJobs;
    uint8_t* returns;
    uint64_t *mask, *refMask;
};
hipError_t drfe_launch_pnp(const PnpLaunch& L, hipStream_t s);
hipError_t drfe_launch_pnp_sweep_one(const PnpCorr* corr, int n, const double* Rt, const double* K, uint64_t* mask, int32_t* count,
                                     hipStream_t s);
void drfe_pnp_free(drfe_ctx* c);

#endif
