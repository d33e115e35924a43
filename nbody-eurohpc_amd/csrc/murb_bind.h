// The two pure functions of the bound-pair read-out (include/murbbind.h has the definition): the total order of the candidates
// and the two-body elements of one pair.  Host code that g++ compiles without a device, so that tests/test_bind_host.py checks
// them through murbbind_elements; the kernels (murb_kernels_bind.h) call the same inline functions.
#ifndef MURB_BIND_H_
#define MURB_BIND_H_

#include <cmath>

#include "murb_layout.h"   // MURB_HD

#define MURB_BIND_ELEMS 6   // {a, e, P, h64, E_b, r}

// The total order: (h as fp32, index), "no candidate" (index -1, h = +inf) behind everything.  An index is compared as
// unsigned, which puts -1 last without a test of its own.  h is never NaN here: a NaN is never a candidate's key.
MURB_HD bool murb_bind_before(const float h_a, const int idx_a, const float h_b, const int idx_b)
{
    return h_a < h_b || (h_a == h_b && (unsigned int)idx_a < (unsigned int)idx_b);
}

// The elements of one pair in fp64 from the fp32 state (include/murbbind.h fixes the order; each line is one operation,
// none contracted).  q, v: three floats each; gm: the fp32 G * m of the records; m: the masses as uploaded.
MURB_HD void murb_bind_elements(const float soft2, const float* qi, const float* vi, const float gmi, const float mi,
                                const float* qj, const float* vj, const float gmj, const float mj, double* out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dx = (double)qj[0] - (double)qi[0], dy = (double)qj[1] - (double)qi[1], dz = (double)qj[2] - (double)qi[2];
    const double wx = (double)vj[0] - (double)vi[0], wy = (double)vj[1] - (double)vi[1], wz = (double)vj[2] - (double)vi[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const double w2 = (wx * wx + wy * wy) + wz * wz;
    const double r = sqrt(d2);
    const double rs = sqrt(d2 + (double)soft2);
    const double GM = (double)gmi + (double)gmj;
    const double h64 = 0.5 * w2 - GM / rs;
    const double a = GM / (-2.0 * h64);
    const double cx = dy * wz - dz * wy, cy = dz * wx - dx * wz, cz = dx * wy - dy * wx;
    const double L2 = (cx * cx + cy * cy) + cz * cz;
    const double e = sqrt(fmax(0.0, 1.0 + ((2.0 * h64) * L2) / (GM * GM)));
    const double P = 6.283185307179586 * sqrt(((a * a) * a) / GM);
    const double ms = (double)mi + (double)mj;
    const double mu = ms == 0.0 ? 0.0 : ((double)mi * (double)mj) / ms;
    out[0] = a;
    out[1] = e;
    out[2] = P;
    out[3] = h64;
    out[4] = mu * h64;
    out[5] = r;
}

#endif
