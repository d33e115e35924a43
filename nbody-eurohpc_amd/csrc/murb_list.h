// The pure functions of the listed-source read-out (include/murblist.h has the definition): where an entry of a list sits in
// the wave that sums it, and the checks that keep the sweep inside the records.  Host code that g++ compiles without a device;
// the kernel (murb_kernels_list.h) calls the same inline functions.
#ifndef MURB_LIST_H_
#define MURB_LIST_H_

#include "murb_layout.h"   // MURB_HD

#define MURB_LIST_STEP 128                 /* entries of a lane step: 64 lanes, two halves */
#define MURB_LIST_MAX_LEN (1ul << 30)      /* entries of one list at the most: the sweep's places are 32-bit */

// entry e of a list: its lane, its half of the lane's packed pair, its lane step
MURB_HD int murb_list_lane(const unsigned int e) { return (int)((e >> 1) & 63u); }
MURB_HD int murb_list_half(const unsigned int e) { return (int)(e & 1u); }
MURB_HD int murb_list_lane_step(const unsigned int e) { return (int)(e >> 7); }

// lane steps of a list of `length` entries; the slots of the last one past the list add +0
MURB_HD int murb_list_lane_steps(const unsigned int length) { return (int)((length + MURB_LIST_STEP - 1) / MURB_LIST_STEP); }

// A CSR pair as murblist_of / murblist_at accept it: offsets[0] == 0, non-decreasing, no list longer than MURB_LIST_MAX_LEN,
// idx given where there is an entry, every entry a body index in [0, n).  Nothing is read past offsets[count] entries of idx.
inline bool murb_list_valid(const unsigned long count, const unsigned long* offsets, const int* idx, const unsigned long n)
{
    if (!offsets || offsets[0] != 0) return false;
    for (unsigned long p = 0; p < count; ++p)
        if (offsets[p + 1] < offsets[p] || offsets[p + 1] - offsets[p] > MURB_LIST_MAX_LEN) return false;
    const unsigned long total = offsets[count];
    if (total > 0 && !idx) return false;
    for (unsigned long e = 0; e < total; ++e)
        if (idx[e] < 0 || (unsigned long)idx[e] >= n) return false;
    return true;
}

#endif
