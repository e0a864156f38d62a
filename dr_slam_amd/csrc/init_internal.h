/* init_internal.h — the records init.cpp stages for init_kernels.hip. */
#ifndef DRFE_INIT_INTERNAL_H
#define DRFE_INIT_INTERNAL_H

#include "drfe_internal.h"
#include "ransac_table.h"
#include "init_core.h"

/* the scoring kernel's LDS bound and rows per workgroup (ransac_device.h); an InitMatch is 16 bytes */
#define DRFE_INIT_LDS_MATCH 2048
#define DRFE_INIT_CHUNK 32

/* one solver on the device */
struct InitSolverRec {
    float K[9], T1[9], T2inv[9], T2t[9];   /* mK; Normalize's T1; T2.inv(); T2.t() */
    float sigma, invSigma2;
    int32_t nKeys1, key10;                 /* reference keys: count, first (over the call) */
    RansacSolverHead head;                 /* n, corr0: the matches; minInliers unused */
};

struct InitLaunch {
    const InitSolverRec* solver;
    int nSolvers, nHyp, maxHyp;            /* maxHyp: the largest hyp of a solver */
    /* in */
    const InitMatch* match;                /* per match of the call */
    const InitNorm* norm;                  /* its two normalised points */
    const int32_t* first;                  /* its reference key, within the solver */
    const int32_t* hypSolver;              /* per row */
    const int32_t* sample;                 /* 8 per row */
    /* scratch */
    float* H12;                            /* 9 per row */
    int32_t *lastH, *lastF;                /* per solver: the row that holds the model at the end, -1: none */
    /* out, rows compact over the call; zero before the launches */
    float *H21, *F21, *scoreH, *scoreF;
    int32_t *bestH, *bestF;
    uint64_t *maskH, *maskF;
    float *SH, *SF, *RH;                   /* per solver */
    int32_t *branch, *motions, *flags;
    float *mR, *mt, *mCos;                 /* per (solver, motion): 9, 3, 1 */
    int32_t *mGood, *mStatus;
    uint8_t* mVbGood;                      /* 8 per reference key of the call */
    float* mP3D;                           /* 8 x 3 per reference key */
};
hipError_t drfe_launch_init(const InitLaunch& L, hipStream_t s);
hipError_t drfe_launch_init_check(const InitLaunch& L, hipStream_t s);
void drfe_init_free(drfe_ctx* c);

/* Initialize's :117-123 for one solver on finished SH, SF: RH, the branch, the flag */
DRFE_HD void init_pick_branch(float SH, float SF, int N, float* RH, int32_t* branch, int32_t* flags)
{
    *RH = 0.f;
    *branch = DRFE_INIT_BRANCH_NONE;
    if (N < 8) { *flags = DRFE_INIT_TOO_FEW; return; }
    if (SH + SF == 0.f) { *flags = DRFE_INIT_NO_MODEL; return; }
    *RH = init_canon(SH / (SH + SF));
    *branch = (double)*RH > 0.40 ? DRFE_INIT_BRANCH_H : DRFE_INIT_BRANCH_F;
    *flags = 0;
}

/* ReconstructH / ReconstructF up to their CheckRT calls for one solver: the motion hypotheses of `model` (H21 or F21 of the row
 * that holds the best model) into mR (8 x 9) and mt (8 x 3), NaN canonical; returns their number and adds to *flags */
DRFE_HD int init_solver_motions(const float K[9], int branch, const float model[9], float* mR, float* mt, int32_t* flags)
{
    float R[8][9], t[8][3];
    int n = 0;
    if (branch == DRFE_INIT_BRANCH_H) {
        if (init_motions_h(model, K, R, t)) n = 8;
        else *flags |= DRFE_INIT_H_DEGENERATE;
    } else if (branch == DRFE_INIT_BRANCH_F) {
        init_motions_f(model, K, R, t);
        n = 4;
    }
    for (int m = 0; m < n; m++) {
        for (int k = 0; k < 9; k++) mR[m * 9 + k] = init_canon(R[m][k]);
        for (int k = 0; k < 3; k++) mt[m * 3 + k] = init_canon(t[m][k]);
    }
    return n;
}

#endif
