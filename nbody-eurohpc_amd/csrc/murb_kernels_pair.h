// gfx950 (CDNA4) device code of the Hermite sweeps: one i body against two j bodies, packed.  Included by murb_kernels_side.h.
#ifndef MURB_KERNELS_PAIR_H_
#define MURB_KERNELS_PAIR_H_

#include "murb_kernels.h"

// ---- one i body against two j bodies (packed): acceleration and jerk ----------------------------------------------
// 6 pk_add + 6 pk_fma (|d|^2 + soft^2, d.w) + 2 rsq + 5 pk_mul + 9 pk_fma
// It hands out two things it makes on the way: r2, the pair of |d|^2 + soft^2 (the nearest-neighbour sweeps keep its minimum,
// the contact sweeps that of the gap made from it), and gi, the pair of GM_j * inv (the potential sweeps and the field keep
// its sum).  A caller that uses neither drops them, and the compiler with it.
__device__ __forceinline__ void murb_interact_jerk_pk_gi(const murb_f2 xj, const murb_f2 yj, const murb_f2 zj, const murb_f2 gj,
                                                         const murb_f2 uj, const murb_f2 vj, const murb_f2 wj,
                                                         const float xi, const float yi, const float zi,
                                                         const float ui, const float vi, const float wi, const float soft2,
                                                         murb_f2& ax, murb_f2& ay, murb_f2& az,
                                                         murb_f2& jx, murb_f2& jy, murb_f2& jz, murb_f2& r2, murb_f2& gi)
{
    const murb_f2 dx = xj - xi, dy = yj - yi, dz = zj - zi;
    const murb_f2 wx = uj - ui, wy = vj - vi, wz = wj - wi;
    r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
    r2 = __builtin_elementwise_fma(dy, dy, r2);
    r2 = __builtin_elementwise_fma(dz, dz, r2);
    murb_f2 dw = dx * wx;
    dw = __builtin_elementwise_fma(dy, wy, dw);
    dw = __builtin_elementwise_fma(dz, wz, dw);
    murb_f2 inv;
    inv.x = __builtin_amdgcn_rsqf(r2.x);
    inv.y = __builtin_amdgcn_rsqf(r2.y);
    const murb_f2 inv2 = inv * inv;
    gi = gj * inv;
    const murb_f2 s = gi * inv2;            // GM_j * inv^3, never G*inv^3 alone (fp32 range)
    const murb_f2 c = (dw * inv2) * -3.0f;  // -3 (d.w) / (|d|^2 + soft^2)
    ax = __builtin_elementwise_fma(s, dx, ax);
    ay = __builtin_elementwise_fma(s, dy, ay);
    az = __builtin_elementwise_fma(s, dz, az);
    jx = __builtin_elementwise_fma(s, __builtin_elementwise_fma(c, dx, wx), jx);
    jy = __builtin_elementwise_fma(s, __builtin_elementwise_fma(c, dy, wy), jy);
    jz = __builtin_elementwise_fma(s, __builtin_elementwise_fma(c, dz, wz), jz);
}

#endif
