/* sim3_opt_internal.h — the records sim3_opt.cpp stages for sim3_opt_kernels.hip. */
#ifndef DRFE_SIM3_OPT_INTERNAL_H
#define DRFE_SIM3_OPT_INTERNAL_H

#include "drfe_internal.h"
#include "sim3_opt_core.h"

/* threads of a problem's workgroup = edges of a chunk (128 matches, e12 and e21 of each); a chunk's 35 terms and its chi2 term per
 * edge live in LDS, rows padded by one double so that the 36 summing lanes read 36 different banks */
#define SO_THREADS 256
#define SO_TERM_STRIDE (SO_THREADS + 1)
#define SO_ROWS (SO_TERMS + 1)

/* per-problem diagnostics, in the order of drfe_sim3_opt_out.diag */
enum { SO_DIAG_REJECTED = 0, SO_DIAG_LAST_REJECTED, SO_DIAG_NBAD_STOPS, SO_DIAG_SMALL_THETA, SO_DIAG_BIG_THETA, SO_DIAG_EARLY_RETURN,
       SO_DIAG_STALE_DECIDED, SO_DIAG_N = 8 };

/* one problem on the device: its matches are match0 .. match0 + nMatches of the call's match list, in index order */
struct SoProbRec {
    double S12[8];
    SoCam cam;
    float R2w[9], t2w[3];
    int32_t match0, nMatches, fixScale, pad;
};

struct SoProbOut {
    double S12[8];
    float T12[16], Scw[16];
    int32_t ret, nBad, iterations[2], trials[2];
    int32_t diag[SO_DIAG_N];
    int32_t handBack, pad;
};

/* T12 and Scw of a finished problem */
DRFE_HD void so_finish(const SoProbRec& P, const SoSim3& S, SoProbOut& O)
{
    for (int k = 0; k < 4; k++) O.S12[k] = S.q[k];
    for (int k = 0; k < 3; k++) O.S12[4 + k] = S.t[k];
    O.S12[7] = S.s;
    so_to_cvmat(S, O.T12);
    SoSim3 Smw, Scw;
    so_from_pose(P.R2w, P.t2w, Smw);
    so_mul(S, Smw, Scw);
    so_to_cvmat(Scw, O.Scw);
}

struct SoLaunch {
    int nProblems;
    const SoProbRec* prob;
    const SoMatch* match;
    double* err;                   /* scratch, 4 per match: _error of e12 and e21 as the last computeError left them */
    uint8_t* flag;                 /* out, per match: nulled by either classification; zero before the launch */
    SoProbOut* out;
};
hipError_t drfe_launch_sim3_opt(const SoLaunch& L, hipStream_t s);
void drfe_sim3_opt_free(drfe_ctx* c);

#endif
