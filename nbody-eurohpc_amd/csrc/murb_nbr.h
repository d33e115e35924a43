// The pure functions of the neighbours-within-a-radius read-out (include/murbnbr.h has the definition): a point's threshold,
// the "list_entries" option and the cut of a launch's points into ranges whose lists fit the device list buffer.  Host code
// that g++ compiles without a device, so that tests/test_nbr_host.py checks them through murbnbr_threshold and murbnbr_cut.
#ifndef MURB_NBR_H_
#define MURB_NBR_H_

#include "murb_layout.h"   // MURB_HD

constexpr long kNbrListDefault = 1l << 26;   // "list_entries" 0: 512 MiB of indices and r2 at the most
constexpr long kNbrListMin = 16, kNbrListMax = 1l << 30;   // the fill sweep's places are 32-bit

inline bool murb_nbr_option_valid(long entries) { return entries == 0 || (entries >= kNbrListMin && entries <= kNbrListMax); }
inline unsigned long murb_nbr_entries(long option) { return (unsigned long)(option > 0 ? option : kNbrListDefault); }

// murbhip_set_encounter's rule: both products are exact in fp64, one rounding in the sum, one in the conversion
MURB_HD float murb_nbr_threshold(const float h, const float soft2)
{
    return (float)((double)h * (double)h + (double)soft2);
}

// The furthest point `last` in (first, count] with offsets[last] - offsets[first] <= entries; first + 1 where even the first
// point's list does not fit (the caller grows its buffer to that list).  offsets: count + 1 non-decreasing entries; first < count.
inline unsigned long murb_nbr_cut(unsigned long count, const unsigned long* offsets, unsigned long first, unsigned long entries)
{
    unsigned long last = first + 1;
    while (last < count && offsets[last + 1] - offsets[first] <= entries) ++last;
    return last;
}

#endif
