/* triangulate_internal.h — the records triangulate.cpp stages for triangulate_kernels.hip. */
#ifndef DRFE_TRIANGULATE_INTERNAL_H
#define DRFE_TRIANGULATE_INTERNAL_H

#include "drfe_internal.h"
#include "triangulate_core.h"

/* one match: kf1 (-1 when its pair is skipped), kf2, idx1, idx2 */
struct TriMatch { int32_t kf1, kf2, idx1, idx2; };

struct TriLaunch {
    TriView V;
    const TriMatch* match;
    int n, line;
    uint8_t *status, *branch;
    float* x3d;                        /* 3 / 6 per match */
};
hipError_t drfe_launch_triangulate(const TriLaunch& L, hipStream_t s);
/* out[i] = drfe_atan2f(y[i], x[i]) (which 0), drfe_cosf(y[i]) (1, x is not read), drfe_cosf(2 * drfe_atan2f(y[i] / 2, x[i])) (2) */
hipError_t drfe_launch_triangulate_math(int which, const float* y, const float* x, int n, float* out, hipStream_t s);
void drfe_triangulate_free(drfe_ctx* c);

#endif
