/* pose_opt_internal.h — the records pose_opt.cpp stages for pose_opt_kernels.hip. */
#ifndef DRFE_POSE_OPT_INTERNAL_H
#define DRFE_POSE_OPT_INTERNAL_H

#include "drfe_internal.h"
#include "pose_opt_core.h"

/* threads of a frame's workgroup = edges of a chunk; a chunk's 27 terms per edge live in LDS, rows padded by one double so that
 * the 27 summing lanes read 27 different banks */
#define PO_THREADS 256
#define PO_TERM_STRIDE (PO_THREADS + 1)

/* per-frame diagnostics beside rounds / iterations / trials, in the order of drfe_pose_opt_out.diag */
enum { PO_DIAG_REJECTED = 0, PO_DIAG_LAST_REJECTED, PO_DIAG_NBAD_STOPS, PO_DIAG_SMALL_THETA, PO_DIAG_BIG_THETA, PO_DIAG_EMPTY_ROUNDS,
       PO_DIAG_N = 8 };

/* plane edges of a group: the twelve perturbations of each take twelve lanes, 192 of the 256 */
#define PO_PLANE_GROUP 16

/* one frame on the device: its edges are edge0 .. edge0 + nEdges of the call's edge list in the order the reference inserts them:
 * the points (index order), start and end of every line, the plane edges */
struct PoFrameRec {
    float Tcw[16];
    PoCam cam;
    int32_t edge0, nEdges, nPoints, nLines;
    int32_t nPlaneEdges, pad[3];   /* after the lines: the matched planes, then with bStruct the parallel and the vertical ones */
};

struct PoFrameOut {
    float Tcw[16];
    int32_t ret, rounds, iterations, trials;
    int32_t diag[PO_DIAG_N];
    int32_t handBack, pad[3];
};

struct PoLaunch {
    int nFrames;
    const PoFrameRec* frame;
    const PoEdge* edge;
    double* err;                   /* scratch, 3 per edge: _error as the last computeError left it */
    uint8_t* flag;                 /* out, per edge: outlier = level 1; zero before the launch */
    PoFrameOut* out;
};
hipError_t drfe_launch_pose_opt(const PoLaunch& L, hipStream_t s);
void drfe_pose_opt_free(drfe_ctx* c);

#endif
