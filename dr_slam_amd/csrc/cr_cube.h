/* cr_cube.h — x * x * x of a double, CORRECTLY ROUNDED, from + - * fma only: identical bits on x86-64 and gfx950.
 *
 * Why: g2o calls pow(., 3) in two places that decide output bits of Optimizer::PoseOptimization - SE3Quat::exp's
 * (theta - sin theta) / pow(theta, 3) and Levenberg's 1 - pow(2 rho - 1, 3).  glibc's pow is correctly
 * rounded in all but a vanishing share of its arguments and exact cases are exact, so the correctly rounded cube is what the
 * host's libm returns; the device has no libm to call.
 *
 * Method: x * x as an exact double-double (two_prod), times x: the high product again exact, the low one rounded once
 * (relative error below 2^-104).  The high word after normalisation is certified by Ziv's test of cr_sincos.h at 2^-100.  The
 * test cannot pass on an exact tie (x with at most 18 significant bits whose cube has 54) and is not trusted where a partial
 * product may have left the normal range: then the routine returns 0 and the caller must not use the value. */
#ifndef DRFE_CR_CUBE_H
#define DRFE_CR_CUBE_H

#include "cr_sincos.h"

DRFE_CR_HD int drfe_cr_cube(double x, double* out)
{
    if (x == 0.0) { *out = x; return 1; }                  /* pow(+-0, 3) = +-0 */
    const double ax = fabs(x);
    if (!(ax > 0x1p-300 && ax < 0x1p+300)) return 0;       /* also NaN and inf */
    const drfe_dd sq = drfe_dd_two_prod(x, x);
    drfe_dd p = drfe_dd_two_prod(sq.h, x);
    p.l += sq.l * x;
    p = drfe_dd_fast_two_sum(p.h, p.l);
    *out = p.h;
    return drfe_cr_certain(p, 0x1p-100);
}

#endif
