/* trans_opt_internal.h — what trans_opt.cpp hands to trans_opt_kernels.hip. */
#ifndef DRFE_TRANS_OPT_INTERNAL_H
#define DRFE_TRANS_OPT_INTERNAL_H

#include "pose_opt_internal.h"
#include "trans_opt_core.h"

/* threads of a frame's workgroup = point / line edges of a pass's chunk; a chunk's nine terms per edge live in LDS, rows padded
 * by one double so that the nine summing lanes read nine different banks */
#define TO_THREADS 256
#define TO_TERM_STRIDE (TO_THREADS + 1)
/* plane edges of a group: the six perturbations of each take six lanes, 192 of the 256; lanes 192..223 own the edges */
#define TO_PLANE_GROUP 32
#define TO_WAVE 64

struct ToLaunch {
    int nFrames;
    ToView view;                   /* device pointers; the flags zero before the launch */
    double* err;                   /* scratch, 3 per edge slot: points, then 2 per line, then 3 per plane slot */
    int64_t lineErr0, planeErr0;   /* edge slots before the first line end / the first plane slot */
    PoFrameOut* out;
};
hipError_t drfe_launch_trans_opt(const ToLaunch& L, hipStream_t s);
void drfe_trans_opt_free(drfe_ctx* c);

/* where a frame's edge k keeps its _error in ToLaunch::err (both entries index their scratch the same way) */
DRFE_HD size_t to_err_slot(const ToFrame& F, const uint8_t* planeAt, int64_t lineErr0, int64_t planeErr0, int k)
{
    if (k < F.nPoints) return (size_t)F.point0 + k;
    if (k < F.nPoints + 2 * F.nLines) return (size_t)lineErr0 + 2 * (size_t)F.line0 + (k - F.nPoints);
    const int at = planeAt[k - F.nPoints - 2 * F.nLines];
    return (size_t)planeErr0 + 3 * (size_t)F.slot0 + (size_t)(at >> 6) * F.nSlots + (at & 63);
}

#endif
