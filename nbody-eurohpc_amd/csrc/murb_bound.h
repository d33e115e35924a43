// The pure functions of the bound-member read-out (include/murbbound.h has the definition): a body's energy in the members'
// frame, the removal rule, the terms of the block sums and the Lagrangian radii.  Host code that g++ compiles without a device,
// so that tests/test_bound_host.py checks it through murbbound_radii; the kernels (murb_kernels_pot.h) call the same inline
// functions.  fp64 throughout, one operation per line, none contracted.
#ifndef MURB_BOUND_H_
#define MURB_BOUND_H_

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "murb_layout.h"   // MURB_HD

#define MURB_BOUND_SUMS 12   // a block row: {members, m, m vx, m vy, m vz, m x, m y, m z, K, m phi, bodies with e >= 0, 0}

// |v - V|^2 of one body: w = (double)v - V, then (wx*wx + wy*wy) + wz*wz
MURB_HD double murb_bound_w2(const float vx, const float vy, const float vz, const double* V)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double wx = (double)vx - V[0];
    const double wy = (double)vy - V[1];
    const double wz = (double)vz - V[2];
    const double xx = wx * wx;
    const double yy = wy * wy;
    const double zz = wz * wz;
    const double xy = xx + yy;
    return xy + zz;
}

// e = 0.5 |v - V|^2 - phi: the energy per unit mass of a body in the frame V against the potential of the members
MURB_HD double murb_bound_energy(const float vx, const float vy, const float vz, const double* V, const float phi)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double w2 = murb_bound_w2(vx, vy, vz, V);
    const double half = 0.5 * w2;
    return half - (double)phi;
}

// the removal rule: a member stays while e < 0; 0, positive and NaN leave
MURB_HD bool murb_bound_stays(const double e) { return e < 0.0; }

// the frame of a set from its sums: V = (sum m v) / (sum m), 0 when that mass is 0
MURB_HD void murb_bound_frame(const double mass, const double* mv, double* V)
{
    V[0] = mass == 0.0 ? 0.0 : mv[0] / mass;
    V[1] = mass == 0.0 ? 0.0 : mv[1] / mass;
    V[2] = mass == 0.0 ? 0.0 : mv[2] / mass;
}

// Lagrangian radii of the members about centre3 (include/murbbound.h, 3): host only.  The members are ordered by (d2, index),
// the mass runs in that order, and radii[f] is sqrt(d2) of the first body at which it reaches frac[f] times the total of the
// same order.  NaN when that total is 0 (no members, or massless ones alone).
inline void murb_bound_radii(const unsigned long n, const float* qx, const float* qy, const float* qz, const float* m,
                             const unsigned char* member, const double* centre3, const int nfrac, const double* frac, double* radii)
{
    struct Entry {
        double d2;
        unsigned long index;
    };
    std::vector<Entry> order;
    order.reserve(n);
    for (unsigned long i = 0; i < n; ++i) {
        if (member && !member[i]) continue;
        const double dx = (double)qx[i] - centre3[0];
        const double dy = (double)qy[i] - centre3[1];
        const double dz = (double)qz[i] - centre3[2];
        const double xx = dx * dx;
        const double yy = dy * dy;
        const double zz = dz * dz;
        const double xy = xx + yy;
        order.push_back({xy + zz, i});
    }
    std::sort(order.begin(), order.end(),
              [](const Entry& a, const Entry& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.index < b.index); });
    double total = 0.0;
    for (const Entry& e : order) total += (double)m[e.index];
    for (int f = 0; f < nfrac; ++f) {
        radii[f] = std::numeric_limits<double>::quiet_NaN();
        if (!(total > 0.0)) continue;
        const double want = frac[f] * total;
        double run = 0.0;
        for (const Entry& e : order) {
            run += (double)m[e.index];
            if (run >= want) {
                radii[f] = std::sqrt(e.d2);
                break;
            }
        }
    }
}

#endif
