// The pure functions of the pair-separation read-out (include/murbsep.h has the definition): the float-bit bin of a squared
// separation, the bins' edges, the slot of the workgroup's counter table, and how many points a launch may take before a 32-bit
// counter could wrap.  Host code that g++ compiles without a device, so that tests/test_sep_host.py checks it through
// murbsep_bin / murbsep_edges and a stand-alone program; the kernels (murb_kernels_sep.h) call the same inline functions.
#ifndef MURB_SEP_H_
#define MURB_SEP_H_

#include <cmath>
#include <cstring>

#include "murb_field.h"   // MurbFieldLayout, MURB_FIELD_GROUP; murb_layout.h: MURB_HD, MURB_TILE_BODIES

#define MURB_SEP_SUB_MAX 6
#define MURB_SEP_BINS_MAX 1022
#define MURB_SEP_TABLE (MURB_SEP_BINS_MAX + 2)   /* 32-bit counters of a workgroup: below | the bins | above: 4 KiB */

// bits(d2) >> sh decides the bin: the exponent and the top `sub` bits of the mantissa
MURB_HD int murb_sep_shift(const int sub) { return 23 - sub; }

// bits(2^lo_exp) >> sh: the key of the lowest edge
MURB_HD int murb_sep_base(const int lo_exp, const int sub) { return (lo_exp + 127) << sub; }

// lo_exp a normal float's exponent, sub and bins in range, and a top edge that is finite (its key below that of +inf)
MURB_HD bool murb_sep_params_valid(const int lo_exp, const int sub, const int bins)
{
    if (lo_exp < -126 || lo_exp > 127 || sub < 0 || sub > MURB_SEP_SUB_MAX || bins < 1 || bins > MURB_SEP_BINS_MAX) return false;
    return murb_sep_base(lo_exp, sub) + bins < (255 << sub);
}

// The slot of the counter table a pair adds to, from the bits of its d2: 0 below, 1 + k for bin k, and every slot past the last
// bin above; the clamp's bounds are constants (one v_med3_i32).  base1 is murb_sep_base - 1.  The bits are read as unsigned, so
// +inf, every NaN and a set sign bit (which a sum of squares never has) lie above.
MURB_HD int murb_sep_slot(const unsigned int bits, const int sh, const int base1)
{
    const int k1 = (int)(bits >> sh) - base1;
    const int lo = k1 < 0 ? 0 : k1;
    return lo > MURB_SEP_TABLE - 1 ? MURB_SEP_TABLE - 1 : lo;
}

// The same slot as a byte offset into the table, the form the kernel uses: one shift, one shift-and-add (minus4 = -4 * base1)
// and the clamp.  bits >> sh is below 2^15, so nothing overflows.
MURB_HD int murb_sep_slot_bytes(const unsigned int bits, const int sh, const int minus4)
{
    const int b = (int)((bits >> sh) << 2) + minus4;
    const int lo = b < 0 ? 0 : b;
    return lo > 4 * (MURB_SEP_TABLE - 1) ? 4 * (MURB_SEP_TABLE - 1) : lo;
}

// -1 below, bins above, else the bin
inline int murb_sep_bin(const int lo_exp, const int sub, const int bins, const float d2)
{
    unsigned int bits;
    std::memcpy(&bits, &d2, sizeof bits);
    const int k = murb_sep_slot(bits, murb_sep_shift(sub), murb_sep_base(lo_exp, sub) - 1) - 1;
    return k > bins ? bins : k;
}

// edge k of bins + 1 edges, an exact float: the lowest d2 of bin k (and of "above" for k == bins)
inline float murb_sep_edge2(const int lo_exp, const int sub, const int k)
{
    const unsigned int bits = (unsigned int)(murb_sep_base(lo_exp, sub) + k) << murb_sep_shift(sub);
    float e;
    std::memcpy(&e, &bits, sizeof e);
    return e;
}

// The slots of the longest chunk of a layout: chunk c takes tiles [tiles * c / chunks, tiles * (c + 1) / chunks).
inline unsigned long murb_sep_unit_pairs(const MurbFieldLayout& l)
{
    const unsigned long longest = ((unsigned long)l.tiles + (unsigned long)l.chunks - 1) / (unsigned long)l.chunks;
    return (unsigned long)MURB_FIELD_GROUP * longest * MURB_TILE_BODIES;
}

// The most pairs one workgroup of a launch of `points` points counts (points in whole groups): its units times 16 times the longest
// chunk's slots.  The grid is min(units, grid), and workgroup b walks units b, b + grid, ...
inline unsigned long murb_sep_worst_pairs(const MurbFieldLayout& l, const long grid, const unsigned long points)
{
    const unsigned long units = points / MURB_FIELD_GROUP * (unsigned long)l.chunks;
    const unsigned long wgs = units < (unsigned long)grid ? units : (unsigned long)grid;
    if (wgs == 0) return 0;
    return (units + wgs - 1) / wgs * murb_sep_unit_pairs(l);
}

// The largest number of points (a multiple of 16) a launch may take so that no 32-bit counter of a workgroup's table can wrap:
// murb_sep_worst_pairs stays below 2^32.  0: not even one group fits (the call is refused).
inline unsigned long murb_sep_max_points(const MurbFieldLayout& l, const long grid)
{
    if (grid < 1) return 0;
    const unsigned long may = 0xfffffffful / murb_sep_unit_pairs(l);   // units a workgroup may take
    // ceil(groups * chunks / grid) <= may  <=>  groups * chunks <= may * grid
    const unsigned long groups = may * (unsigned long)grid / (unsigned long)l.chunks;
    return groups * MURB_FIELD_GROUP;
}

// the points of a launch: the smaller of "field_batch" and the bound above
inline unsigned long murb_sep_cut(const MurbFieldLayout& l, const long grid)
{
    const unsigned long most = murb_sep_max_points(l, grid);
    return most < l.batch ? most : l.batch;
}

#endif
