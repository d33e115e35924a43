// The pure functions of the Ahmad-Cohen neighbour scheme (include/murbac.h has the definition): the regular force's polynomial
// between two regular steps and the update of its derivatives at a regular step.  Host code that g++ compiles without a device
// (tests/test_ac_host.py builds it alone and under the sanitizers); the kernels (murb_kernels_ac.h) call the same inline functions.
// fp64 intermediates, no contraction, left to right as written, ONE rounding to fp32 at the end: the convention of the Hermite
// predictor and corrector (murb_kernels_hermite.h).  clang takes the pragma below; a g++ build passes -ffp-contract=off.
#ifndef MURB_AC_H_
#define MURB_AC_H_

#include "murb_layout.h"   // MURB_HD

#define MURB_AC_NIRR_MAX 4096   /* regular steps are at least this often */

inline bool murb_ac_nirr_valid(const int n_irr) { return n_irr >= 1 && n_irr <= MURB_AC_NIRR_MAX; }

// the time since the last regular step after `steps` steps of dt (tau = (m + 1) dt; T = n_irr dt): both factors exact in fp64
MURB_HD double murb_ac_elapsed(const int steps, const float dt)
{
    return (double)steps * (double)dt;
}

// aR(tR + tau) = aR + jR tau + a2R tau^2 / 2 + a3R tau^3 / 6
MURB_HD float murb_ac_poly_a(const float aR, const float jR, const float a2R, const float a3R, const double tau)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (float)((((double)aR + (double)jR * tau) + (double)a2R * (tau * tau * 0.5)) + (double)a3R * (tau * tau * tau / 6.0));
}

// jR(tR + tau) = jR + a2R tau + a3R tau^2 / 2
MURB_HD float murb_ac_poly_j(const float jR, const float a2R, const float a3R, const double tau)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (float)(((double)jR + (double)a2R * tau) + (double)a3R * (tau * tau * 0.5));
}

// Makino & Aarseth's interpolation through (A0, J0) at the start and (A1, J1) at the end of an interval T, both ends taken on
// the same list: x2, x3 the second and third derivative at the START, the stored ones those at the END.
MURB_HD void murb_ac_derivatives(const float A0, const float J0, const float A1, const float J1, const double T, float& a2R, float& a3R)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = (double)A0 - (double)A1;
    const double x2 = (-6.0 * d - T * (4.0 * (double)J0 + 2.0 * (double)J1)) / (T * T);
    const double x3 = (12.0 * d + 6.0 * T * ((double)J0 + (double)J1)) / (T * T * T);
    a2R = (float)(x2 + T * x3);
    a3R = (float)x3;
}

#endif
