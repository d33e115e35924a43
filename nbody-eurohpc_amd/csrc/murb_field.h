// Planning of the field read-out (murbfield_at / murbfield_of; include/murbfield.h has the definition) and of every read-out
// that sweeps packed points the same way: how the j tiles are cut into chunks, a call's points into launches, and one launch
// into workgroups.  Pure host code that g++ compiles too, so that tests/test_field_host.py checks it through murbfield_layout
// and a stand-alone program without a device.
//
// The rule that matters: the chunk count is a function of the BODY count and of "field_chunks" alone.  A point's partial sums
// are cut by the chunks, so its bits would otherwise depend on how many points the caller happened to ask for.
#ifndef MURB_FIELD_H_
#define MURB_FIELD_H_

#include <algorithm>

#include "murb_layout.h"

#define MURB_FIELD_GROUP 16   /* points per workgroup of the sweep (4 waves x 4 points) */

// "field_chunks" 0: chunks of at least 8 tiles, 16 chunks at the most (profiles/field_sweep.txt: a (group, chunk) unit costs
// about two tiles' time on top of its tiles, so long chunks win wherever there are points enough to fill the chip, and the
// smallest call, which they slow down, is bound by the call's fixed cost anyway)
constexpr long kFieldTilesPerChunk = 8, kFieldChunksMax = 16;
constexpr long kFieldBatchDefault = 16384;     // "field_batch" 0: points per launch
constexpr long kFieldBatchMax = 1l << 20;

struct MurbFieldLayout {
    int tiles;               // layout tiles that hold real bodies: the j side of the sweep
    int chunks;              // j chunks: chunk c takes tiles [tiles * c / chunks, tiles * (c + 1) / chunks)
    unsigned long batch;     // points per full launch
    unsigned long groups;    // ... in groups of MURB_FIELD_GROUP
    unsigned long rows;      // entries of a partial-row buffer: batch * chunks
};

inline bool murb_field_options_valid(long chunks_option, long batch_option)
{
    return chunks_option >= 0 && batch_option >= 0 && batch_option <= kFieldBatchMax && batch_option % MURB_FIELD_GROUP == 0;
}

inline MurbFieldLayout murb_field_layout(unsigned long n, long chunks_option, long batch_option)
{
    MurbFieldLayout l{};
    const unsigned long tiles = n == 0 ? 1ul : (n + MURB_TILE_BODIES - 1) / MURB_TILE_BODIES;
    const unsigned long by_rule = std::min<unsigned long>(std::max<unsigned long>(tiles / kFieldTilesPerChunk, 1ul), kFieldChunksMax);
    const unsigned long want = chunks_option > 0 ? (unsigned long)chunks_option : by_rule;
    l.tiles = (int)tiles;
    l.chunks = (int)(want < tiles ? want : tiles);
    l.batch = (unsigned long)(batch_option > 0 ? batch_option : kFieldBatchDefault);
    l.groups = l.batch / MURB_FIELD_GROUP;
    l.rows = l.batch * (unsigned long)l.chunks;
    return l;
}

// launches a call of `count` points is cut into: points [b * batch, min(count, (b + 1) * batch))
inline unsigned long murb_field_batches(const MurbFieldLayout& l, unsigned long count)
{
    return (count + l.batch - 1) / l.batch;
}

// points rounded up to whole groups of MURB_FIELD_GROUP: the packed records a sweep reads (the filler points are computed and
// never read back)
inline unsigned long murb_field_padded(unsigned long points)
{
    return (points + MURB_FIELD_GROUP - 1) / MURB_FIELD_GROUP * MURB_FIELD_GROUP;
}

// workgroups of a launch of groups x chunks (group, chunk) units on a chip that holds grid_full of them: workgroup b walks the
// units b, b + grid, ...
inline long murb_field_grid(long groups, long chunks, long grid_full)
{
    return std::max(1l, std::min(groups * chunks, grid_full));
}

// How one launch of `padded` points (whole groups, at least one) is cut.
struct MurbFieldCut {
    int groups;        // groups of points
    int chunks;        // j chunks of this launch
    int tiles_each;    // chunk c holds tiles_each tiles, the first tiles_more chunks one more ...
    int tiles_more;    // ... for the sweeps that cut by these two rather than by tiles * c / chunks
    long grid;         // workgroups
};

// fill_grid false: the layout's chunk count whatever the launch holds, for a result that depends on the cut (a sum: the rule at
// the top).  fill_grid true: the layout's chunk count is the MOST the launch is cut into, for a result that does not (a list, a
// count, a minimum).  Every chunk pays its start again, so a launch whose groups fill the chip on their own is not cut at all,
// and one with fewer groups into as many chunks as fill it.
inline MurbFieldCut murb_field_cut(const MurbFieldLayout& l, unsigned long padded, long grid_full, bool fill_grid)
{
    MurbFieldCut k{};
    k.groups = (int)(padded / MURB_FIELD_GROUP);
    k.chunks = fill_grid ? (int)std::min<long>(l.chunks, std::max<long>(1, (grid_full + k.groups - 1) / k.groups)) : l.chunks;
    k.tiles_each = l.tiles / k.chunks;   // chunks <= tiles: every chunk holds a tile
    k.tiles_more = l.tiles % k.chunks;
    k.grid = murb_field_grid(k.groups, k.chunks, grid_full);
    return k;
}

#endif
