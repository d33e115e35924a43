// The two pure functions of the k-nearest-neighbour read-out (include/murbknn.h has the definition): the total order of the
// candidates with the merge of two sorted lists under it, and the density of one list.  Host code that g++ compiles without a
// device, so that tests/test_knn_host.py checks them through murbknn_merge and murbknn_density; the kernels
// (murb_kernels_knn.h) call the same inline functions.
#ifndef MURB_KNN_H_
#define MURB_KNN_H_

#include <cmath>
#include <limits>

#include "murb_layout.h"   // MURB_HD

#define MURB_KNN_KMAX 32

// The total order: (r2 as fp32, index), "no candidate" (index -1, r2 = +inf) behind everything.  An index is compared as
// unsigned, which puts -1 last without a test of its own.
MURB_HD bool murb_knn_before(const float r2_a, const int idx_a, const float r2_b, const int idx_b)
{
    return r2_a < r2_b || (r2_a == r2_b && (unsigned int)idx_a < (unsigned int)idx_b);
}

// The k first entries of the merge of two lists that are sorted under the order above (each k long, tails of -1 / +inf).
// The two hold different candidates, or the same entry in both (then it is taken once).  The outputs alias no input.
MURB_HD void murb_knn_merge(const int k, const int* idx_a, const float* r2_a, const int* idx_b, const float* r2_b,
                            int* idx_out, float* r2_out)
{
    int a = 0, b = 0;
    for (int l = 0; l < k; ++l) {
        const bool end_a = a >= k, end_b = b >= k;
        if (end_a && end_b) {
            idx_out[l] = -1;
            r2_out[l] = std::numeric_limits<float>::infinity();
            continue;
        }
        if (!end_a && !end_b && idx_a[a] == idx_b[b] && r2_a[a] == r2_b[b]) ++b;   // one entry, listed twice
        const bool take_a = !(a >= k) && (b >= k || !murb_knn_before(r2_b[b], idx_b[b], r2_a[a], idx_a[a]));
        idx_out[l] = take_a ? idx_a[a] : idx_b[b];
        r2_out[l] = take_a ? r2_a[a] : r2_b[b];
        if (take_a) ++a; else ++b;
    }
}

// The general-mass form of Casertano & Hut's unbiased estimator for one sorted list (include/murbknn.h): the mass of the
// k - 1 nearest over the volume of the sphere through the k-th.  One fp64 operation per step, none contracted.
MURB_HD float murb_knn_density(const int k, const int* idx, const float* r2, const float* masses, const float soft2)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (idx[k - 1] < 0) return 0.f;   // fewer than k candidates
    const double d2 = (double)r2[k - 1] - (double)soft2;
    if (d2 == 0.0) return std::numeric_limits<float>::infinity();   // k bodies on one point
    double m = 0.0;
    for (int l = 0; l + 1 < k; ++l) m = m + (double)masses[idx[l]];
    const double vol = 4.1887902047863905 * (d2 * sqrt(d2));
    return (float)(m / vol);
}

#endif
