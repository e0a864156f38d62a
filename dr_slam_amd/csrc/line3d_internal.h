/* line3d_internal.h — what lines_3d_batch.cpp stages for lines_3d_kernels.hip. */
#ifndef DRFE_LINE3D_INTERNAL_H
#define DRFE_LINE3D_INTERNAL_H

#include "drfe_internal.h"
#include "line3d_core.h"

/* key lines whose lifted samples the call scratch holds at once (4.8 KiB a line: 96 MiB when full); a call with more
 * nframes * cap runs in chunks of drfe_line3d_chunk_frames(cap) frames */
#define DRFE_LINE3D_SCRATCH_LINES 20480
/* rand() draws a frame can consume per key line: L3_MAX_ITERATIONS iterations of two */
#define DRFE_LINE3D_DRAWS (2 * L3_MAX_ITERATIONS)

/* what the RANSAC walk leaves of a key line for k_line3d_finish */
struct L3Best {
    uint64_t mask;                 /* the best verified inlier set over the line's lifted samples, 0: none */
    L3P A, B;                      /* the pair that gave it */
};

/* a frame's counters, summed into drfe_line3d_stats [3..6] */
struct L3FrameStats {
    int32_t ransacLines, iterations, coincident, rejected;
};

struct Line3dLaunch {
    int nframes, cap, w, h;
    int maxLines;                  /* the most key lines of a frame of the call */
    size_t frameStride, stride;    /* of depth, in floats */
    float cx, cy, invfx, invfy;
    double f;                      /* l3_focal */
    /* in */
    const drfe_keyline* lines;     /* nframes x cap */
    const int32_t* nLines;         /* nframes */
    const int32_t* draws;          /* nframes x cap x DRFE_LINE3D_DRAWS: the frame's rand() stream */
    const float* depth;
    /* scratch, per key line (slot f * cap + i) */
    int32_t* nPts;
    L3Point* pts;                  /* L3_MAX_SAMPLES a slot, the lifted samples in sample order */
    L3Best* best;
    /* out; nGood zero before the launches */
    float* depthLine;
    double* lines3d;               /* 6 a slot */
    int32_t* nInliers;
    int32_t* nGood;                /* per frame */
    L3FrameStats* frameStats;      /* per frame */
};
hipError_t drfe_launch_line3d(const Line3dLaunch& L, hipStream_t s);
void drfe_line3d_free(drfe_ctx* c);

#endif
