// Planning of the field read-out (murbfield_at / murbfield_of; include/murbfield.h has the definition): how the j tiles
// are cut into chunks and a call's points into launches.  Pure host code that g++ compiles too, so that
// tests/test_field_host.py checks it through murbfield_layout without a device.
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

#endif
