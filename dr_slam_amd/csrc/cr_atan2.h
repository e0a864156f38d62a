/* cr_atan2.h — atan2(y, x) of doubles for y >= 0, CORRECTLY ROUNDED, from + - * / sqrt fma only: identical bits on x86-64 and
 * gfx950.  A sibling of cr_sincos.h, whose double-double sine and cosine it uses.
 *
 * Why: Sim3Solver::ComputeSim3 takes `atan2(norm(vec), evec.at<float>(0,0))` in double from the host's libm (reference
 * src/Sim3Solver.cc:282) and every bit of the transform follows from it.  On the device there is no libm to call.  The first
 * argument is a norm (>= 0, possibly 0 or NaN), the second a quaternion's real part of either sign.
 *
 * Method: the exact cases first (a zero, an infinity, a NaN).  When one argument is below 2^-61 of the other the result is the
 * rounded quotient, pi/2 or pi: atan t = t (1 - t^2/3 + ..) differs from t by less than 2^-122 relative, a quotient of doubles is
 * never nearer than 2^-107 relative to a rounding boundary of the normal range, and pi/2 and pi lie 0.22 ulp from theirs.  (A
 * quotient in the subnormal range can sit exactly on a boundary: not certified.)  Otherwise both arguments are scaled by one
 * power of two into [2^-62, 1), a0 = atan2 in plain double (drfe_atan_unit_d, ~1 ulp), and one Newton step in double-double:
 * atan2(y, x) = a0 + atan((y cos a0 - x sin a0) / (x cos a0 + y sin a0)), where the quotient d is below 2^-50 a0 and atan d = d
 * to 2^-150.  The error of a0 + d is that of sin / cos a0 (2^-64 or 2^-100 relative) times sin a0 cos a0 <= a0.  The final double
 * is certified by Ziv's test as in cr_sincos.h, first with the cheap series, then with the full one. */
#ifndef DRFE_CR_ATAN2_H
#define DRFE_CR_ATAN2_H

#include "../../include/drfe_math.h"
#include "cr_sincos.h"

#define DRFE_CR_PI 0x1.921fb54442d18p+1        /* the doubles nearest pi, pi/2, pi/4, 3pi/4; pi = PI + PI_LO */
#define DRFE_CR_PI_LO 0x1.1a62633145c07p-53
#define DRFE_CR_PIO2 0x1.921fb54442d18p+0
#define DRFE_CR_PIO2_LO 0x1.1a62633145c07p-54
#define DRFE_CR_PIO4 0x1.921fb54442d18p-1
#define DRFE_CR_3PIO4 0x1.2d97c7f3321d2p+1

/* a0 + d of the Newton step, normalised; y > 0, x != 0, both scaled; a0 in (0, pi] */
DRFE_CR_HD drfe_dd drfe_cr_atan2_step(double y, double x, double a0, int ddTerms)
{
    drfe_dd s, c;
    (void)drfe_sincos_dd(a0, &s, &c, ddTerms);
    const drfe_dd yd = {y, 0.0}, xd = {x, 0.0};
    const drfe_dd num = drfe_dd_add(drfe_dd_mul(yd, c), drfe_dd_neg(drfe_dd_mul(xd, s)));
    const double den = x * c.h + y * s.h;
    return drfe_dd_fast_two_sum(a0, num.h / den);
}

/* atan2(y, x) for y >= 0 (or NaN).  Returns 1 with the correctly rounded double in *out, or 0 when it cannot certify it (*out
 * then holds an approximation the caller must not use): y < 0, a quotient in the subnormal range, or a value within 2^-96 of a
 * rounding boundary. */
DRFE_CR_HD int drfe_cr_atan2(double y, double x, double* out)
{
    if (y != y || x != x) { *out = y + x; return 1; }
    if (y < 0.0) { *out = NAN; return 0; }
    const int xneg = signbit(x) ? 1 : 0;
    if (y == 0.0) { *out = xneg ? DRFE_CR_PI : 0.0; return 1; }
    if (x == 0.0) { *out = DRFE_CR_PIO2; return 1; }
    const int yinf = y == INFINITY, xinf = fabs(x) == INFINITY;
    if (yinf) { *out = xinf ? (xneg ? DRFE_CR_3PIO4 : DRFE_CR_PIO4) : DRFE_CR_PIO2; return 1; }
    if (xinf) { *out = xneg ? DRFE_CR_PI : 0.0; return 1; }
    int ey, ex;
    (void)frexp(y, &ey);
    (void)frexp(x, &ex);
    if (ex - ey > 62) {                              /* y / |x| < 2^-61 */
        if (xneg) { *out = DRFE_CR_PI; return 1; }
        const double q = y / x;
        *out = q;
        return q >= 0x1p-1022;
    }
    if (ey - ex > 62) { *out = DRFE_CR_PIO2; return 1; }
    const int e = ey > ex ? ey : ex;
    const double ys = ldexp(y, -e), xs = ldexp(x, -e), ax = fabs(xs);
    double a0 = ys <= ax ? drfe_atan_unit_d(ys / ax) : (DRFE_CR_PIO2 - drfe_atan_unit_d(ax / ys)) + DRFE_CR_PIO2_LO;
    if (xneg) a0 = (DRFE_CR_PI - a0) + DRFE_CR_PI_LO;
    drfe_dd v = drfe_cr_atan2_step(ys, xs, a0, 3);
    *out = v.h;
    if (drfe_cr_certain(v, 0x1p-60)) return 1;
    v = drfe_cr_atan2_step(ys, xs, a0, 8);
    *out = v.h;
    return drfe_cr_certain(v, 0x1p-96);
}

#endif
