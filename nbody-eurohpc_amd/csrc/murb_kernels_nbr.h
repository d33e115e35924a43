// gfx950 (CDNA4) kernels of the neighbours-within-a-radius read-out (murbnbr_of / murbnbr_at).  Device code only; included by
// murb_ctx.h.
#ifndef MURB_KERNELS_NBR_H_
#define MURB_KERNELS_NBR_H_

#include "murb_field.h"
#include "murb_kernels_side.h"
#include "murb_nbr.h"

// ---- neighbours within a radius of arbitrary points (include/murbnbr.h has the definition) -----------------------------------
// The k-nearest-neighbour sweep's walk (murb_kernels_knn.h) with a count, then a list of variable length, in the place of the
// sorted list: `count` points against ALL bodies at their current positions, per point the bodies with r2 <= thr, one body
// slot left out.  No atomic operation anywhere: a point's place in the output comes from a prefix sum over counts.
//     1  murb_nbr_pack_kernel    a pack step of its own: {x, y, z, skip} {thr, 0, 0, 0}; thr rides in the point's second record,
//                                which the field read-out's pack step leaves empty for points at rest.  The points that fill
//                                up the last group of 16 get thr = -1, which no r2 (>= soft2 >= 0) passes: they take no place
//                                in any count and write nothing
//     2  murb_nbr_count_kernel   the walk over (group of 16 points, j chunk) units on the fixed grid; per unit and point one
//                                32-bit count: part[chunk * stride + point]
//     3  murb_nbr_rows_kernel    one thread per point: its count, and in the place of part[chunk * stride + point] the sum of
//                                its earlier chunks' counts ("within": where a chunk's entries start inside the point's list)
//        (host)                  downloads the counts, extends the offsets by a prefix sum, cuts the launch's points into
//                                ranges whose lists fit the list buffer (murb_nbr_cut) and uploads per range the points' bases
//     4  murb_nbr_fill_kernel    the same walk over the range's groups: a unit starts at base[point] + within[chunk][point]
//                                and writes its entries in ascending index
// Both sweeps take the "which of this lane step's 128 slots are neighbours" decision from ONE function, murb_nbr_lane_step, so
// that the places the count gives and the entries the fill writes cannot disagree.
#define MURB_NBR_NO_BASE 0xffffffffu   // base of a point that is not in the range being filled

struct MurbNbrPackArgs {
    const float* in;        // murbnbr_at: px | py | pz, in_stride floats each; null: murbnbr_of
    const float* thr;       // a threshold per point of the launch
    const int* idx;         // murbnbr_at: the skip entries, or null (none); murbnbr_of: the bodies
    const float4* rec;      // murbnbr_of: where the bodies' q are read
    float4* pts;
    int count;              // points of the launch
    int padded;             // ... rounded up to whole groups
    unsigned int in_stride;
};

__global__ __launch_bounds__(256) void murb_nbr_pack_kernel(const MurbNbrPackArgs a)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= a.padded) return;
    const bool real = p < a.count;
    const int src = real ? p : p / MURB_FIELD_GROUP * MURB_FIELD_GROUP;   // the group's first point: < count
    float x, y, z;
    int skip = -1;
    if (a.in) {
        x = a.in[src]; y = a.in[a.in_stride + src]; z = a.in[2 * a.in_stride + src];
        if (a.idx) skip = a.idx[src];
    } else {
        skip = a.idx[src];
        const unsigned long ra = murb_rec_a((unsigned long)(skip >> 1));
        const float* const q = (const float*)(a.rec + ra) + (skip & 1);
        x = q[0]; y = q[2]; z = q[4 * MURB_TILE_PAIRS];
    }
    a.pts[2 * p] = make_float4(x, y, z, __builtin_bit_cast(float, skip));
    a.pts[2 * p + 1] = make_float4(real ? a.thr[p] : -1.f, 0.f, 0.f, 0.f);
}

struct MurbNbrArgs {
    const float4* rec;          // current positions + GM, all slots
    const float4* pts;          // two records per point (murb_nbr_pack_kernel)
    unsigned int* part;         // count: part[chunk * stride + point] written; fill: read as `within` (murb_nbr_rows_kernel)
    const unsigned int* base;   // fill: base[point - 16 * group_first], relative to the list buffer, or MURB_NBR_NO_BASE
    int* out_idx;               // fill: the list buffer
    float* out_r2;
    unsigned int capacity;      // fill: entries the list buffer holds
    int group_first, groups;    // the launch's groups of points: [group_first, group_first + groups)
    int chunks;
    int tiles_each, tiles_more; // the j cut: every chunk takes tiles_each layout tiles, the first tiles_more chunks one more
    int count;                  // real bodies: slots >= count are padding and never candidates
    unsigned int stride;        // points per chunk row of part
    float soft2;
};

// One lane step for one point: the r2 of the lane's two slots (j0 = j_first + 2 * lane and j0 + 1), and as two ballots which
// of the wave's 128 slots are neighbours: bit l of `first` is slot j_first + 2 l, bit l of `second` slot j_first + 2 l + 1.
// The point's values, j_first and count are wave-uniform.  `index < n` and `index != skip` cost nothing per pair: the body
// itself always passes the compare (r2 = soft2 <= thr) and the padding at the origin may, so a lane step whose 128 slots
// hold the skipped slot or reach past the last real body — two scalar tests on j_first — takes the exact path, which strikes
// those slots' bits off the ballots in scalar registers; every other lane step is 3 packed subtractions, 3 packed fmas
// and one compare per half.  EXACT == false: the caller has made sure, for the whole tile of 4 lane steps, that neither can
// happen (murb_nbr_sweep: the same two tests on the tile's first slot), and the scalar tests are not even made.
__device__ __forceinline__ unsigned long murb_nbr_low_bits(const int n)   // the n lowest bits; n <= 0: none, n >= 64: all
{
    return n >= 64 ? ~0ul : n <= 0 ? 0ul : (1ul << n) - 1ul;
}

template <bool EXACT>
__device__ __forceinline__ void murb_nbr_lane_step(const murb_f2 xj, const murb_f2 yj, const murb_f2 zj, const float xi, const float yi,
                                                   const float zi, const float soft2, const float thr, const int j_first, const int skip,
                                                   const int count, murb_f2& r2, unsigned long& first, unsigned long& second)
{
    const murb_f2 dx = xj - xi, dy = yj - yi, dz = zj - zi;
    r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
    r2 = __builtin_elementwise_fma(dy, dy, r2);
    r2 = __builtin_elementwise_fma(dz, dz, r2);
    first = __builtin_amdgcn_ballot_w64(r2.x <= thr);
    second = __builtin_amdgcn_ballot_w64(r2.y <= thr);
    if constexpr (EXACT) {
        const unsigned int to_skip = (unsigned int)(skip - j_first);   // skip == -1 never lands in [0, 128)
        const int real = count - j_first;                              // slots of this lane step that hold real bodies, if < 128
        if (real < 128 || to_skip < 128u) {                            // wave-uniform, scalar throughout
            if (to_skip < 128u) {
                const unsigned long bit = 1ul << (to_skip >> 1);
                if (to_skip & 1u) second &= ~bit; else first &= ~bit;
            }
            if (real < 128) {   // slot 2 l is real for l < ceil(real / 2), slot 2 l + 1 for l < floor(real / 2)
                first &= murb_nbr_low_bits((real + 1) >> 1);
                second &= murb_nbr_low_bits(real >> 1);
            }
        }
    }
}

struct MurbNbrPoint {   // wave-uniform, in scalar registers
    float x, y, z, thr;
    unsigned int at;    // the counter, or the cursor
};

// One lane step of a staged tile (512 slots from j_tile on, 4 lane steps) against a wave's R points.
// FILL == false: per point a wave-uniform counter of the two ballots' population counts.
// FILL == true: per point a wave-uniform cursor, the next free place of its list.  In a lane step with a non-empty ballot a
// lane's place is the cursor plus the set bits below it in both ballots in slot order (lane-major, the first half before the
// second): ascending index without a sort.  The entries leave through ordinary vector stores from the lanes that hold them.
template <int R, bool FILL, bool EXACT>
__device__ __forceinline__ void murb_nbr_step(const MurbNbrArgs& a, const float4* tq, const int q, const int j_tile, const int lane,
                                              const float soft2, const int count, MurbNbrPoint (&pt)[R], const int (&skip)[R])
{
    const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y};
    const int j_first = j_tile + 2 * q;   // lane 0's first slot
#pragma unroll
    for (int r = 0; r < R; ++r) {
        murb_f2 r2;
        unsigned long first, second;
        murb_nbr_lane_step<EXACT>(xj, yj, zj, pt[r].x, pt[r].y, pt[r].z, soft2, pt[r].thr, j_first, skip[r], count, r2, first, second);
        const unsigned int found = (unsigned int)(__builtin_popcountll(first) + __builtin_popcountll(second));
        if constexpr (FILL) {
            if (found != 0u) {   // wave-uniform
                const bool in0 = (first >> lane) & 1ul, in1 = (second >> lane) & 1ul;
                // the set bits below this lane, of both ballots
                unsigned int below = __builtin_amdgcn_mbcnt_hi((unsigned int)(first >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)first, 0u));
                below = __builtin_amdgcn_mbcnt_hi((unsigned int)(second >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)second, below));
                const unsigned int place0 = pt[r].at + below;
                const unsigned int place1 = place0 + (in0 ? 1u : 0u);
                const int j0 = j_first + 2 * lane;
                // the places follow from the counts of the same predicate; the bound keeps a fault in either from
                // writing outside the list buffer
                if (in0 && place0 < a.capacity) { a.out_idx[place0] = j0; a.out_r2[place0] = r2.x; }
                if (in1 && place1 < a.capacity) { a.out_idx[place1] = j0 + 1; a.out_r2[place1] = r2.y; }
            }
        }
        pt[r].at += found;
    }
}

// launches 2 and 4.  murb_knn_sweep_kernel's mapping: a workgroup takes a group of 16 points, 4 per wave, their point, skip
// and thr wave-uniform, and walks units u = blockIdx.x, += gridDim.x with (group, chunk) =
// (group_first + u % groups, u / groups).  STAGE tiles of 8 KiB each in LDS: positions alone.  Chunk c takes
// tiles_each tiles, the first tiles_more chunks one more: tiles_each * chunks + tiles_more = tiles (a count and a list do not
// depend on the cut, so it need not be the field sweep's).
template <int R, int WAVES, int STAGE, bool FILL>
__device__ __forceinline__ void murb_nbr_sweep(const MurbNbrArgs& a, float4* lds)
{
    static_assert(R % 2 == 0 && WAVES * R == MURB_FIELD_GROUP, "a workgroup takes one group of points");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
    static_assert(STAGE * MURB_TILE_F4 * sizeof(float4) * 4 <= 160 * 1024, "4 workgroups per CU share its LDS");
    const float soft2 = a.soft2;
    const int count = a.count;

    // Through the loop the scalar registers hold the points' coordinates (a packed instruction reads a scalar as a pair: 6
    // registers a point), thr and the counters; the skip entries wait in one vector register and are read per tile.  Of the
    // kernel's argument only rec, soft2, count and the fill's three stay, the rest is read again once per unit
    // (murb_kernarg_again).
    for (int u = blockIdx.x;; u += (int)gridDim.x) {
        const auto* now = murb_kernarg_again<MurbNbrArgs>();   // `a` is the kernel's first argument
        const int groups = now->groups, chunks = now->chunks;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, local = u - chunk * groups;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));   // made here, per unit: nothing derived from it is held in scalar registers across units
        const int lane = tid & 63;
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int i_first = ((now->group_first + local) * WAVES + wave) * R;   // point of the launch, wave-uniform

        MurbNbrPoint pt[R];
        int who = -1;   // the points' skip entries wait in lanes 0 .. R - 1 of one vector register, like the field sweep's
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 P = now->pts[2 * (i_first + r)], T = now->pts[2 * (i_first + r) + 1];
            pt[r].x = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.x)));
            pt[r].y = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.y)));
            pt[r].z = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.z)));
            who = lane == r ? __builtin_bit_cast(int, P.w) : who;
            pt[r].thr = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, T.x)));
            pt[r].at = 0u;
            if constexpr (FILL) {
                const unsigned int b = now->base[(local * WAVES + wave) * R + r];   // < 16 * groups
                const unsigned int w = now->part[(unsigned long)chunk * now->stride + (unsigned long)(i_first + r)];
                const unsigned int base = (unsigned int)__builtin_amdgcn_readfirstlane((int)b);
                if (base == MURB_NBR_NO_BASE) pt[r].thr = -1.f;   // not in this range: nothing passes
                pt[r].at = base + (unsigned int)__builtin_amdgcn_readfirstlane((int)w);
            }
        }

        const int each = now->tiles_each, more = now->tiles_more;
        const int vt0 = chunk * each + (chunk < more ? chunk : more);
        const int vt1 = vt0 + each + (chunk < more ? 1 : 0);   // <= tiles

        for (int vs = vt0; vs < vt1; vs += STAGE) {
            const int nt = (vt1 - vs) < STAGE ? (vt1 - vs) : STAGE;
            __syncthreads();   // previous stage (of this unit or the one before) fully consumed
            for (int t = 0; t < nt; ++t) {
                const float4* srcq = a.rec + (unsigned long)(vs + t) * MURB_TILE_F4;   // vs + t < vt1 <= tiles
#pragma unroll
                for (int c = 0; c < MURB_TILE_F4 / (WAVES * 64); ++c) {
                    const int e = tid + c * WAVES * 64;
                    lds[t * MURB_TILE_F4 + e] = srcq[e];
                }
            }
            __syncthreads();
            for (int t = 0; t < nt; ++t) {
                const float4* tq = lds + t * MURB_TILE_F4;
                const int j_tile = (vs + t) * MURB_TILE_BODIES;
                int held = who, skip[R];
                asm volatile("" : "+v"(held));   // read here, per tile: not held in scalar registers through the loops
                bool exact = j_tile + MURB_TILE_BODIES > count;   // the tile reaches past the last real body, ...
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    skip[r] = __builtin_amdgcn_readlane(held, r);
                    exact = exact || (unsigned int)(skip[r] - j_tile) < (unsigned int)MURB_TILE_BODIES;   // ... or holds a skipped slot
                }
                if (exact) {   // wave-uniform; rare, and its masks want scalar registers: not unrolled
#pragma unroll 1
                    for (int q = 0; q < MURB_TILE_PAIRS; q += 64) murb_nbr_step<R, FILL, true>(a, tq, q, j_tile, lane, soft2, count, pt, skip);
                } else {
#pragma unroll 2
                    for (int q = 0; q < MURB_TILE_PAIRS; q += 64) murb_nbr_step<R, FILL, false>(a, tq, q, j_tile, lane, soft2, count, pt, skip);
                }
            }
        }

        if constexpr (!FILL) {
            const auto* end = murb_kernarg_again<MurbNbrArgs>();
            unsigned int* const row = end->part + ((unsigned long)chunk * end->stride + (unsigned long)i_first);   // < chunks * stride
            int slot = lane;
            asm volatile("" : "+v"(slot));   // compared here, not before the loops
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (slot == r) row[r] = pt[r].at;
        }
    }
}

template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_nbr_count_kernel(const MurbNbrArgs a)
{
    __shared__ float4 lds[STAGE * MURB_TILE_F4];
    murb_nbr_sweep<R, WAVES, STAGE, false>(a, lds);
}

template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_nbr_fill_kernel(const MurbNbrArgs a)
{
    __shared__ float4 lds[STAGE * MURB_TILE_F4];
    murb_nbr_sweep<R, WAVES, STAGE, true>(a, lds);
}

// launch 3: one thread per point of the launch.  Integers only: counts[p] = the sum of the point's chunk counts, and each
// part[chunk * stride + p] becomes the sum of the chunks before it.
__global__ __launch_bounds__(256) void murb_nbr_rows_kernel(unsigned int* part, unsigned int* counts, const int count, const int chunks,
                                                            const unsigned int stride)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= count) return;
    unsigned int sum = 0u;
    for (int c = 0; c < chunks; ++c) {
        const unsigned long e = (unsigned long)c * stride + (unsigned long)p;
        const unsigned int v = part[e];
        part[e] = sum;
        sum += v;
    }
    counts[p] = sum;
}

#endif
