// gfx950 (CDNA4) kernels of the bound-pair read-out (murbbind_of / murbbind_at / murbbind_pairs).  Device code only; included
// by murb_ctx.h.
#ifndef MURB_KERNELS_BIND_H_
#define MURB_KERNELS_BIND_H_

#include "murb_bind.h"
#include "murb_field.h"
#include "murb_kernels_side.h"

// ---- most bound partner of arbitrary points (include/murbbind.h has the definition) ------------------------------------------
// The field read-out's rectangular sweep (murb_kernels_field.h) with a lexicographic minimum in the place of the sums: `count`
// points with velocities and G m of their own against ALL bodies at their current state, per point the smallest (h, index)
// with one body slot left out, h the specific two-body energy of the softened pair.
//     1  murb_bind_pack_kernel    the uploaded SoA points, or the listed bodies' own q, v and G m gathered from the records,
//                                 into two records per point: {x, y, z, skip} {u, v, w, gm}; the last group of 16 is filled
//                                 up with copies of its first point (murb_field_pack_kernel's rule; their rows are never read)
//     2  murb_bind_sweep_kernel   the field sweep's walk over (group of 16 points, j chunk) units on the same fixed grid; per
//                                 unit and point one (key, index): part[chunk * stride + point]
//     3  murb_bind_rows_kernel    one thread per point: the chunks' entries folded in chunk order
//     4  murb_bind_pairs_kernel   murbbind_pairs: one thread per body; the elements of the bound pairs into dense per-body
//                                 arrays and 256-body block sums in fp64 (murb_metrics_kernel's order)
// The running minimum is kept the way the nearest-neighbour sweeps keep theirs (murb_kernels_side.h): every lane keeps, per
// point, the minimum of the h it has formed (one three-operand minimum per pair of interactions) and the lane step
// S = 4 * tile + q / 64 at which it last fell (a compare and a select).  j slots rise with S in a lane and the select takes a
// strictly smaller value only, so S is the EARLIEST step that holds the lane's minimum.  Behind the loop the lane forms that one
// step's two h again from the records in memory, through the same inline function: every operation of it is correctly
// rounded and v_rsq_f32 is the same instruction, hence the same bits, and the first of the two that holds the minimum is the
// lowest slot.  The wave then folds (key, slot) lexicographically.  A v_min_f32 never returns a NaN while one operand is a
// number, and `<` is false for one: a candidate whose h is NaN (or +inf) is never chosen.
// h may be negative, so (h, slot) travel as the order-preserving unsigned key of the contact sweeps (murb_ct_key).
// `index < n` and `index != skip` cost the plain tiles nothing: the tiles that hold one of the wave's skipped slots or reach
// past the last real body run the EXACT form of the step, which replaces such a slot's h by +inf before the minimum
// (murb_nbr_step's split); the step behind the loop always tests.
#define MURB_BIND_NONE 0x7fffffffu   // "no candidate" in the rows (the public index is -1)

struct MurbBindPackArgs {
    const float* in;        // murbbind_at: px | py | pz | pvx | pvy | pvz | gm, in_stride floats each; null: murbbind_of
    const int* idx;         // murbbind_at: the skip entries, or null (none); murbbind_of: the bodies
    const float4* rec;      // murbbind_of: where the bodies' q, G m and v are read
    const float4* vel;
    float4* pts;
    int count;              // points of the launch
    int padded;             // ... rounded up to whole groups
    unsigned int in_stride;
    int has_vel;            // murbbind_at: 0 = points at rest
    int has_gm;             // murbbind_at: 0 = massless points
};

__global__ __launch_bounds__(256) void murb_bind_pack_kernel(const MurbBindPackArgs a)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= a.padded) return;
    const int src = p < a.count ? p : p / MURB_FIELD_GROUP * MURB_FIELD_GROUP;   // the group's first point: < count
    float x, y, z, u = 0.f, v = 0.f, w = 0.f, gm = 0.f;
    int skip = -1;
    if (a.in) {
        x = a.in[src]; y = a.in[a.in_stride + src]; z = a.in[2 * a.in_stride + src];
        if (a.has_vel) { u = a.in[3 * a.in_stride + src]; v = a.in[4 * a.in_stride + src]; w = a.in[5 * a.in_stride + src]; }
        if (a.has_gm) gm = a.in[6 * a.in_stride + src];
        if (a.idx) skip = a.idx[src];
    } else {
        skip = a.idx[src];
        const unsigned long ra = murb_rec_a((unsigned long)(skip >> 1));
        const float* const q = (const float*)(a.rec + ra) + (skip & 1);
        const float* const qv = (const float*)(a.vel + ra) + (skip & 1);
        x = q[0]; y = q[2]; z = q[4 * MURB_TILE_PAIRS]; gm = q[4 * MURB_TILE_PAIRS + 2];
        u = qv[0]; v = qv[2]; w = qv[4 * MURB_TILE_PAIRS];   // lanes z, w of the B record may carry radii ("contact"): never read
    }
    a.pts[2 * p] = make_float4(x, y, z, __builtin_bit_cast(float, skip));
    a.pts[2 * p + 1] = make_float4(u, v, w, gm);
}

struct MurbBindArgs {
    const float4* rec;      // current positions + GM, all slots
    const float4* vel;      // current velocities (with "contact" on their B records carry radii in lanes z, w: never read)
    const float4* pts;      // two records per point (murb_bind_pack_kernel)
    uint2* part;            // part[chunk * stride + point] = {key, index}
    int groups, chunks;     // the launch's units
    int tiles_each, tiles_more; // the j cut: every chunk takes tiles_each layout tiles, the first tiles_more chunks one more
    int count;              // real bodies: slots >= count are padding and never candidates
    unsigned int stride;    // points per chunk row: 16 * groups
    float soft2;
};

// h of one point and two j bodies, packed (include/murbbind.h, one fp32 operation per line there): 6 packed subtractions,
// 3 packed fmas for r2, a packed multiply and 2 packed fmas for w2, 2 v_rsq_f32, a packed add, a packed multiply and a packed
// fma.  The loop and the step behind it share this one function.
__device__ __forceinline__ murb_f2 murb_bind_h_pk(const murb_f2 xj, const murb_f2 yj, const murb_f2 zj, const murb_f2 gj,
                                                  const murb_f2 uj, const murb_f2 vj, const murb_f2 wj,
                                                  const float xi, const float yi, const float zi,
                                                  const float ui, const float vi, const float wi, const float gi, const float soft2)
{
    const murb_f2 dx = xj - xi, dy = yj - yi, dz = zj - zi;
    const murb_f2 wx = uj - ui, wy = vj - vi, wz = wj - wi;
    murb_f2 r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
    r2 = __builtin_elementwise_fma(dy, dy, r2);
    r2 = __builtin_elementwise_fma(dz, dz, r2);
    murb_f2 w2 = wx * wx;
    w2 = __builtin_elementwise_fma(wy, wy, w2);
    w2 = __builtin_elementwise_fma(wz, wz, w2);
    murb_f2 inv;
    inv.x = __builtin_amdgcn_rsqf(r2.x);
    inv.y = __builtin_amdgcn_rsqf(r2.y);
    const murb_f2 gs = gj + gi;
    const murb_f2 half = w2 * 0.5f;
    return __builtin_elementwise_fma(-gs, inv, half);
}

struct MurbBindPoint {   // wave-uniform: x, y, z, u, v in scalar registers, w and gm in vector registers (murb_bind_sweep_kernel)
    float x, y, z, u, v, w, gm;
};

// One lane step of a staged tile (slots j_tile + 2 q ... on) against a wave's R points.  EXACT: the tile holds a skipped slot or
// reaches past the last real body, and every slot is tested; otherwise the caller has made sure that neither can happen.
template <int R, bool EXACT>
__device__ __forceinline__ void murb_bind_step(const float4* tq, const float4* tv, const int q, const int lane, const int tile,
                                               const int count, const float soft2, const MurbBindPoint (&pt)[R], const int (&skip)[R],
                                               float (&mn)[R], int (&st)[R])
{
    const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
    const float4 VA = tv[q + lane], VB = tv[q + lane + MURB_TILE_PAIRS];
    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
    const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y};
    const int S = tile * (MURB_TILE_PAIRS / 64) + q / 64;
    const int j0 = tile * MURB_TILE_BODIES + 2 * (q + lane);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        murb_f2 h = murb_bind_h_pk(xj, yj, zj, gj, uj, vj, wj, pt[r].x, pt[r].y, pt[r].z, pt[r].u, pt[r].v, pt[r].w, pt[r].gm, soft2);
        if constexpr (EXACT) {
            if (j0 == skip[r] || j0 >= count) h.x = __builtin_inff();
            if (j0 + 1 == skip[r] || j0 + 1 >= count) h.y = __builtin_inff();
        }
        const float m = __builtin_fminf(__builtin_fminf(mn[r], h.x), h.y);
        st[r] = m < mn[r] ? S : st[r];
        mn[r] = m;
    }
}

// launch 2.  murb_force_field_kernel's mapping: a workgroup takes a group of 16 points, 4 per wave, each point's eight values
// wave-uniform, and walks units u = blockIdx.x, += gridDim.x with (group, chunk) = (u % groups, u / groups).  A packed instruction
// reads a scalar operand as an aligned pair of registers, so the four points' x, y, z, u, v take 40 scalar registers; w and gm
// stay in vector registers, the same in every lane (with them in scalar registers too the build spilled scalar registers), and
// the skip entries wait in the lanes of one vector register, like the field sweep's, read out in the tiles that need them.
// STAGE tiles of positions and of velocities in LDS, 16 KiB a tile, staged as the tracer sweep stages them: with STAGE = 2 a
// workgroup holds 32 KiB and 4 workgroups share a CU's 160 KiB, the 4 waves per SIMD the attribute asks for.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_bind_sweep_kernel(const MurbBindArgs a)
{
    static_assert(R % 2 == 0 && WAVES * R == MURB_FIELD_GROUP, "a workgroup takes one group of points");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
    static_assert(2 * STAGE * MURB_TILE_F4 * sizeof(float4) * 4 <= 160 * 1024, "4 workgroups per CU share its LDS");
    static_assert(MURB_TILE_BODIES == 1 << 9, "a slot's tile is slot >> 9");
    __shared__ float4 lds[2 * STAGE * MURB_TILE_F4];
    const float soft2 = a.soft2;
    const int count = a.count;

    for (int u = blockIdx.x;; u += (int)gridDim.x) {
        const int groups = a.groups, chunks = a.chunks;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        const int i_first = (group * WAVES + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;   // point of the launch, wave-uniform

        MurbBindPoint pt[R];
        float mn[R];
        int st[R];
        // lane l: the skip entry of point l % R (-1: none); read out in the tiles that need it and behind the loop
        const int who = __builtin_bit_cast(int, a.pts[2 * (i_first + (lane & (R - 1)))].w);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 P = a.pts[2 * (i_first + r)], V = a.pts[2 * (i_first + r) + 1];
            pt[r].x = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.x)));
            pt[r].y = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.y)));
            pt[r].z = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.z)));
            pt[r].u = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, V.x)));
            pt[r].v = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, V.y)));
            pt[r].w = V.z;    // the same in every lane, in a vector register
            pt[r].gm = V.w;   // likewise
            mn[r] = __builtin_inff();
            st[r] = 0;
        }

        // tiles_each * chunks + tiles_more = tiles (a minimum does not depend on the cut, so it need not be the field sweep's)
        const int each = a.tiles_each, more = a.tiles_more;
        const int vt0 = chunk * each + (chunk < more ? chunk : more);
        const int vt1 = vt0 + each + (chunk < more ? 1 : 0);   // <= tiles

        for (int vs = vt0; vs < vt1; vs += STAGE) {
            const int nt = (vt1 - vs) < STAGE ? (vt1 - vs) : STAGE;
            __syncthreads();   // previous stage (of this unit or the one before) fully consumed
            for (int t = 0; t < nt; ++t) {
                const float4* srcq = a.rec + (unsigned long)(vs + t) * MURB_TILE_F4;   // vs + t < vt1 <= tiles
                const float4* srcv = a.vel + (unsigned long)(vs + t) * MURB_TILE_F4;
#pragma unroll
                for (int c = 0; c < MURB_TILE_F4 / (WAVES * 64); ++c) {
                    const int k = tid + c * WAVES * 64;
                    lds[(2 * t) * MURB_TILE_F4 + k] = srcq[k];
                    lds[(2 * t + 1) * MURB_TILE_F4 + k] = srcv[k];
                }
            }
            __syncthreads();
            for (int t = 0; t < nt; ++t) {
                const float4* tq = lds + (2 * t) * MURB_TILE_F4;
                const float4* tv = tq + MURB_TILE_F4;
                const int tile = vs + t;
                // the tile reaches past the last real body, or holds a skipped slot (-1 >> 9 = -1: no tile)
                const bool exact = (tile + 1) * MURB_TILE_BODIES > count || __builtin_amdgcn_ballot_w64((who >> 9) == tile) != 0;
                int skip[R];
                if (exact) {   // wave-uniform; rare: not unrolled
#pragma unroll
                    for (int r = 0; r < R; ++r) skip[r] = __builtin_amdgcn_readlane(who, r);
#pragma unroll 1
                    for (int q = 0; q < MURB_TILE_PAIRS; q += 64) murb_bind_step<R, true>(tq, tv, q, lane, tile, count, soft2, pt, skip, mn, st);
                } else {
#pragma unroll
                    for (int q = 0; q < MURB_TILE_PAIRS; q += 64) murb_bind_step<R, false>(tq, tv, q, lane, tile, count, soft2, pt, skip, mn, st);
                }
            }
        }

        // the slot behind every lane's minimum, then the fold over the wave: (key, slot) of every point, wave-uniform
        uint2 out[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int p = st[r] * 64 + lane;   // the pair of slots of lane step st[r] (0 where nothing fell): inside the tiles swept
            const unsigned long ra = murb_rec_a((unsigned long)p);
            const float4 A = a.rec[ra], B = a.rec[ra + MURB_TILE_PAIRS];
            const float4 VA = a.vel[ra], VB = a.vel[ra + MURB_TILE_PAIRS];
            const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
            const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y};
            const murb_f2 h = murb_bind_h_pk(xj, yj, zj, gj, uj, vj, wj, pt[r].x, pt[r].y, pt[r].z, pt[r].u, pt[r].v, pt[r].w, pt[r].gm, soft2);
            const int j0 = 2 * p;
            const bool first = h.x == mn[r] && j0 != __builtin_amdgcn_readlane(who, r) && j0 < count;
            const unsigned int idx = mn[r] < __builtin_inff() ? (unsigned int)(first ? j0 : j0 + 1) : MURB_BIND_NONE;
            const unsigned int key = murb_ct_key(mn[r]);
            out[r].x = murb_wave_min_bits(__builtin_bit_cast(float, key));   // an unsigned minimum of the bits
            out[r].y = murb_wave_min_bits(__builtin_bit_cast(float, key == out[r].x ? idx : MURB_BIND_NONE));
        }
        if (lane == 0) {
            uint2* const row = a.part + ((unsigned long)chunk * a.stride + (unsigned long)i_first);   // < chunks * 16 * groups
#pragma unroll
            for (int r = 0; r < R; ++r) row[r] = out[r];
        }
    }
}

// launch 3: one thread per point of the launch.  The chunks' (key, index) folded lexicographically in chunk order; -1 and +inf
// where there is no candidate.
__global__ __launch_bounds__(256) void murb_bind_rows_kernel(const uint2* part, int* out_idx, float* out_h, const int count,
                                                             const int chunks, const unsigned int stride)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= count) return;
    unsigned int key = murb_ct_key(__builtin_inff()), idx = MURB_BIND_NONE;
    for (int c = 0; c < chunks; ++c) {
        const uint2 e = part[(unsigned long)c * stride + p];
        if (e.x < key || (e.x == key && e.y < idx)) { key = e.x; idx = e.y; }
    }
    out_idx[p] = idx == MURB_BIND_NONE ? -1 : (int)idx;
    out_h[p] = idx == MURB_BIND_NONE ? __builtin_inff() : murb_ct_value(key);
}

// launch 4 (murbbind_pairs): one thread per body over the sweep's (partner, h) of all bodies.  A body that is the lower index
// of a bound pair writes the pair's elements (murb_bind_elements) into its own place of the dense array and sets its flag; the
// host compacts in index order.  Per block of 256 consecutive bodies the fp64 sums {bound pairs, E_b, bodies whose partner
// has h < 0, mutual pairs} in murb_metrics_kernel's fixed order (wave shuffle tree, then the 4 waves through LDS); the host
// adds the block rows in index order.  mass: the masses as uploaded, by body index.
#define MURB_BIND_SUMS 4
__global__ __launch_bounds__(256) void murb_bind_pairs_kernel(const float4* rec, const float4* vel, const float* mass, const int* partner,
                                                              const float* h, double* elems, int* flag, double* out, const int count,
                                                              const float soft2)
{
#pragma clang fp contract(off)
    __shared__ double red[3][MURB_BIND_SUMS];
    const int s = blockIdx.x * 256 + threadIdx.x;
    double v[MURB_BIND_SUMS] = {0.0, 0.0, 0.0, 0.0};
    if (s < count) {
        const int j = partner[s];
        const float hs = h[s];
        int bound = 0;
        if (j >= 0 && hs < 0.f) v[2] = 1.0;
        if (j > s && j < count && partner[j] == s) {   // mutual, and this body the lower index
            v[3] = 1.0;
            if (hs < 0.f) {
                float q[2][3], w[2][3], gm[2];
                const int who[2] = {s, j};
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const unsigned long ra = murb_rec_a((unsigned long)(who[b] >> 1));
                    const float* const pq = (const float*)(rec + ra) + (who[b] & 1);
                    const float* const pv = (const float*)(vel + ra) + (who[b] & 1);
                    q[b][0] = pq[0]; q[b][1] = pq[2]; q[b][2] = pq[4 * MURB_TILE_PAIRS]; gm[b] = pq[4 * MURB_TILE_PAIRS + 2];
                    w[b][0] = pv[0]; w[b][1] = pv[2]; w[b][2] = pv[4 * MURB_TILE_PAIRS];
                }
                double e[MURB_BIND_ELEMS];
                murb_bind_elements(soft2, q[0], w[0], gm[0], mass[s], q[1], w[1], gm[1], mass[j], e);
#pragma unroll
                for (int k = 0; k < MURB_BIND_ELEMS; ++k) elems[(unsigned long)s * MURB_BIND_ELEMS + k] = e[k];
                bound = 1;
                v[0] = 1.0;
                v[1] = e[4];
            }
        }
        flag[s] = bound;
    }
#pragma unroll
    for (int e = 0; e < MURB_BIND_SUMS; ++e)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[e] += __shfl_down(v[e], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0 && wave > 0) {
#pragma unroll
        for (int e = 0; e < MURB_BIND_SUMS; ++e) red[wave - 1][e] = v[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < MURB_BIND_SUMS; ++e) out[(unsigned long)blockIdx.x * MURB_BIND_SUMS + e] = ((v[e] + red[0][e]) + red[1][e]) + red[2][e];
    }
}

#endif
