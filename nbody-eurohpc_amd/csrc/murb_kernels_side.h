// gfx950 (CDNA4) device code of the Hermite sweeps: what a sweep may keep beside (a, j) in the rows' fourth floats, its
// side product: a nearest neighbour, a contact partner or a potential.  Included by murb_kernels_hermite.h.
#ifndef MURB_KERNELS_SIDE_H_
#define MURB_KERNELS_SIDE_H_

#include <type_traits>

#include "murb_kernels_pair.h"

// What a sweep keeps beside (a, j).  The host picks the kernel by it (murbhip.hip, sweep_side); the sweep bodies take it as a
// template argument, and the plain form's code does not change with the others.
enum class MurbSide { None, Nearest, Contact, Potential };

// minimum of a positive float (or +inf) over the wave: rows of 16 lanes by DPP, the four rows through v_readlane
__device__ __forceinline__ unsigned int murb_wave_min_bits(const float v)
{
    unsigned int m = __builtin_bit_cast(unsigned int, v);
    // quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror (murb_wave_sum's folds)
    unsigned int o = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, true);
    m = o < m ? o : m;
    o = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, true);
    m = o < m ? o : m;
    o = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, true);
    m = o < m ? o : m;
    o = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)m, 0x140, 0xF, 0xF, true);
    m = o < m ? o : m;
    const unsigned int r0 = (unsigned int)__builtin_amdgcn_readlane((int)m, 0), r1 = (unsigned int)__builtin_amdgcn_readlane((int)m, 16);
    const unsigned int r2 = (unsigned int)__builtin_amdgcn_readlane((int)m, 32), r3 = (unsigned int)__builtin_amdgcn_readlane((int)m, 48);
    const unsigned int lo = r0 < r1 ? r0 : r1, hi = r2 < r3 ? r2 : r3;
    return lo < hi ? lo : hi;
}

// ---- nearest neighbour beside the sweep (option "nearest"; include/murbhip.h has the definition) ----------------------------
// Every lane keeps, per i body, the minimum of the r2 it has formed (one three-operand minimum per pair of interactions)
// and the lane step S = 4 * tile + q / 64 at which that minimum last fell (a compare and a select).  j slots rise with S in a
// lane, and the select takes a strictly smaller value only, so S is the EARLIEST step holding the lane's minimum.  After
// the loop the lane forms that one step's two r2 again from the records in memory — the same subtractions and fused
// multiply-adds, hence the same bits — and takes the first of the two that holds the minimum: the lowest slot.  The wave
// then folds (r2 bits, slot) lexicographically, and lane r writes body r's pair into the fourth floats of its two
// partial-row records; whoever adds the rows up takes the lexicographic minimum beside the sums (murb_nn_fold_row).
// The body itself and the zero-mass padding are no candidates.  Testing that per pair would cost every pair; instead the
// wave asks per tile (wave-uniform) whether it holds one of its i bodies or slots >= count, and only those tiles run the
// masked form of the step, which replaces the r2 of such a slot by +inf before the minimum.
#define MURB_F32_INF_BITS 0x7f800000u
#define MURB_NN_NONE 0x7fffffffu   // "no candidate" in the rows (the public index is -1)
#define MURB_ENC_CAP 4096          // pairs the encounter list keeps

// (i, nn_i, r2_i) of the bodies whose r2 was within the encounter threshold in the step that ended the run; order unspecified
struct MurbEncList {
    int i[MURB_ENC_CAP], j[MURB_ENC_CAP];
    float r2[MURB_ENC_CAP];
};

// The kernel's first argument read again from the kernel-argument segment (scalar loads).  Behind the sweep's loop this
// re-makes what the fold and the stores need instead of holding it in scalar registers through the loop; the empty asm
// makes the pointer a new value to the compiler.
template <typename Args>
__device__ __forceinline__ const __attribute__((address_space(4))) Args* murb_kernarg_again()
{
    unsigned long p = (unsigned long)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (const __attribute__((address_space(4))) Args*)p;
}

// Does the tile hold padding or one of the wave's own bodies (self_tile: the layout tiles they lie in)?  Wave-uniform.
template <int RT>
__device__ __forceinline__ bool murb_nn_tile_masked(const int tile, const int (&self_tile)[RT], const int count)
{
    bool m = (tile + 1) * MURB_TILE_BODIES > count;
#pragma unroll
    for (int r = 0; r < RT; ++r) m |= self_tile[r] == tile;
    return m;
}

// r2 of one i body and one j body behind the loop, in single instructions: the same three subtractions and three fused
// multiply-adds as one half of the sweep's packed ones, hence the same bits.  Written as instructions so that the compiler
// does not pack them two by two again: the kernels' packed arithmetic stays exactly the sweep's (the code-object tests
// compare the instruction counts).
__device__ __forceinline__ float murb_nn_r2_single(const float xj, const float yj, const float zj,
                                                   const float xi, const float yi, const float zi, const float soft2)
{
#if defined(__HIP_DEVICE_COMPILE__)
    float dx, dy, dz, r2;
    asm("v_subrev_f32 %0, %1, %2" : "=v"(dx) : "s"(xi), "v"(xj));
    asm("v_subrev_f32 %0, %1, %2" : "=v"(dy) : "s"(yi), "v"(yj));
    asm("v_subrev_f32 %0, %1, %2" : "=v"(dz) : "s"(zi), "v"(zj));
    asm("v_fma_f32 %0, %1, %1, %2" : "=v"(r2) : "v"(dx), "v"(soft2));
    asm("v_fma_f32 %0, %1, %1, %2" : "=v"(r2) : "v"(dy), "v"(r2));
    asm("v_fma_f32 %0, %1, %1, %2" : "=v"(r2) : "v"(dz), "v"(r2));
    return r2;
#else
    const float dx = xj - xi, dy = yj - yi, dz = zj - zi;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, soft2)));
#endif
}

// Where rows are added up in chunk order: the lexicographic minimum of (r2 bits, slot) beside the sums.
__device__ __forceinline__ void murb_nn_fold_row(unsigned int& r2, unsigned int& idx, const float4 u, const float4 w)
{
    const unsigned int ub = __builtin_bit_cast(unsigned int, u.w), ib = __builtin_bit_cast(unsigned int, w.w);
    if (ub < r2 || (ub == r2 && ib < idx)) { r2 = ub; idx = ib; }
}

// ---- contact by radii beside the sweep (option "contact"; include/murbhip.h has the definition) ------------------------------
// The nearest-neighbour scheme with gap2 = (r2 - soft2) - (R_i + R_j)^2 in r2's place: a packed add for the sum of radii (the
// j radii ride in the two spare lanes of the velocity B record, the i radii in scalar registers), a packed add for r2 - soft2
// and a packed fma, then the minimum, the compare and the select of the lane step.  gap2 may be negative, so the sign trick of
// the nearest form does not carry over: a masked tile subtracts -inf instead of soft2 (a wave-uniform select per tile), every
// gap2 of it is +inf and nothing is recorded.  Where (gap2, slot) are folded they travel as an order-preserving unsigned key
// (murb_ct_key); the per-slot store decodes it.
__device__ __forceinline__ unsigned int murb_ct_key(const float g)
{
    const unsigned int b = __builtin_bit_cast(unsigned int, g);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}

__device__ __forceinline__ float murb_ct_value(const unsigned int k)
{
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// gap2 of one i body and one j body behind the loop, in single instructions that give the packed ones' bits (murb_nn_r2_single)
__device__ __forceinline__ float murb_ct_gap2_single(const float xj, const float yj, const float zj, const float rj,
                                                     const float xi, const float yi, const float zi, const float ri, const float soft2)
{
    const float r2 = murb_nn_r2_single(xj, yj, zj, xi, yi, zi, soft2);
#if defined(__HIP_DEVICE_COMPILE__)
    float s, e, g;
    asm("v_add_f32 %0, %1, %2" : "=v"(s) : "v"(ri), "v"(rj));
    asm("v_subrev_f32 %0, %1, %2" : "=v"(e) : "v"(soft2), "v"(r2));
    asm("v_fma_f32 %0, -%1, %1, %2" : "=v"(g) : "v"(s), "v"(e));
    return g;
#else
    const float s = rj + ri, e = r2 - soft2;
    return __builtin_fmaf(-s, s, e);
#endif
}

// ---- what the two minima share: the helpers behind the loop, over a metric -------------------------------------------------
// A metric names what a sweep keeps the minimum of.  RADII: the j radii are read from the velocity records and the i radii
// are live (the nearest form passes neither).  single(): the metric of one i body and one j body in single instructions that
// give the packed ones' bits.  key(): the order-preserving unsigned form (value, slot) are folded in; r2 is positive, so its
// key is its bits, and the rows of the nearest form hold r2 itself.  value() undoes key().  "No candidate" is key(+inf).
struct MurbNearestMetric {
    static constexpr bool RADII = false;
    static __device__ __forceinline__ float single(const float xj, const float yj, const float zj, const float,
                                                   const float xi, const float yi, const float zi, const float, const float soft2)
    {
        return murb_nn_r2_single(xj, yj, zj, xi, yi, zi, soft2);
    }
    static __device__ __forceinline__ unsigned int key(const float m) { return __builtin_bit_cast(unsigned int, m); }
    static __device__ __forceinline__ float value(const unsigned int k) { return __builtin_bit_cast(float, k); }
};

struct MurbContactMetric {
    static constexpr bool RADII = true;
    static __device__ __forceinline__ float single(const float xj, const float yj, const float zj, const float rj,
                                                   const float xi, const float yi, const float zi, const float ri, const float soft2)
    {
        return murb_ct_gap2_single(xj, yj, zj, rj, xi, yi, zi, ri, soft2);
    }
    static __device__ __forceinline__ unsigned int key(const float m) { return murb_ct_key(m); }
    static __device__ __forceinline__ float value(const unsigned int k) { return murb_ct_value(k); }
};

// The pairs of one masked tile, from the records in memory: the metric alone, formed like the sweep forms it (the same bits),
// with the body itself and the padding left out.  Runs after the loop, so the steps no longer rise: an equal value at an
// earlier step takes the place.
template <int R, typename M>
__device__ __forceinline__ void murb_side_masked_tile(const float4* rec, const float4* vel, const int lane, const int tile,
                                                      const float (&xi)[R], const float (&yi)[R], const float (&zi)[R],
                                                      const float (&ri)[R], const float soft2,
                                                      float (&mn)[R], int (&st)[R], const int (&self)[R], const int count)
{
#pragma unroll 1
    for (int qs = 0; qs < MURB_TILE_PAIRS / 64; ++qs) {
        const unsigned long ra = (unsigned long)tile * MURB_TILE_F4 + qs * 64 + lane;
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
        float4 VB = {};
        if constexpr (M::RADII) VB = vel[ra + MURB_TILE_PAIRS];
        const int S = tile * (MURB_TILE_PAIRS / 64) + qs;
        const int j0 = tile * MURB_TILE_BODIES + 2 * (qs * 64 + lane);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float rr = M::RADII ? ri[r] : 0.f;
            float gx = M::single(A.x, A.z, B.x, VB.z, xi[r], yi[r], zi[r], rr, soft2);
            float gy = M::single(A.y, A.w, B.y, VB.w, xi[r], yi[r], zi[r], rr, soft2);
            if (j0 == self[r] || j0 >= count) gx = __builtin_inff();
            if (j0 + 1 == self[r] || j0 + 1 >= count) gy = __builtin_inff();
            const float m = __builtin_fminf(gx, gy);
            if (m < mn[r] || (m == mn[r] && S < st[r])) { mn[r] = m; st[r] = S; }
        }
    }
}

// After the loop: the slot behind every lane's minimum, the fold over the wave; lane r gets body r's (key, slot).
template <int R, typename M>
__device__ __forceinline__ void murb_side_finish(const float4* rec, const float4* vel, const int lane,
                                                 const float (&xi)[R], const float (&yi)[R], const float (&zi)[R], const float (&ri)[R],
                                                 const float soft2, const float (&mn)[R], const int (&st)[R],
                                                 const int (&self)[R], const int count, unsigned int& out_key, unsigned int& out_idx)
{
    out_key = M::key(__builtin_inff());
    out_idx = MURB_NN_NONE;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int p = st[r] * 64 + lane;   // the pair of slots of lane step st[r]
        const unsigned long ra = murb_rec_a((unsigned long)p);
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
        float4 VB = {};
        if constexpr (M::RADII) VB = vel[ra + MURB_TILE_PAIRS];
        const float gx = M::single(A.x, A.z, B.x, VB.z, xi[r], yi[r], zi[r], M::RADII ? ri[r] : 0.f, soft2);
        const int j0 = 2 * p;
        const bool first = gx == mn[r] && j0 != self[r] && j0 < count;
        const unsigned int idx = mn[r] < __builtin_inff() ? (unsigned int)(first ? j0 : j0 + 1) : MURB_NN_NONE;
        const unsigned int key = M::key(mn[r]);
        const unsigned int kb = murb_wave_min_bits(__builtin_bit_cast(float, key));   // an unsigned minimum of the bits
        const unsigned int cand = key == kb ? idx : MURB_NN_NONE;
        const unsigned int ib = murb_wave_min_bits(__builtin_bit_cast(float, cand));
        if (lane == r) { out_key = kb; out_idx = ib; }
    }
}

// The per-slot store of the correctors: the key decoded, -1 and +inf where there was no candidate.
template <typename M>
__device__ __forceinline__ void murb_side_store(int* nn_idx, float* nn_r2, const int s, const unsigned int key, const unsigned int idx)
{
    nn_idx[s] = idx == MURB_NN_NONE ? -1 : (int)idx;
    nn_r2[s] = idx == MURB_NN_NONE ? __builtin_inff() : M::value(key);
}

// ... and their hit test.  A body that took the step with a value <= thr (r2 against radius^2 + soft^2, gap2 against 0) is a
// hit: it takes a place in the list (a vector atomic, like the active list's).
template <typename M>
__device__ __forceinline__ void murb_side_test(unsigned int* hits, MurbEncList* list, const float thr, const int i,
                                               const unsigned int key, const unsigned int idx)
{
    if (idx == MURB_NN_NONE || !(M::value(key) <= thr)) return;
    const unsigned int at = atomicAdd(hits, 1u);
    if (at < MURB_ENC_CAP) { list->i[at] = i; list->j[at] = (int)idx; list->r2[at] = M::value(key); }
}

// ---- per-body potential beside the sweep (option "potential"; include/murbhip.h has the definition) --------------------------
// phi_i = sum_{j != i} GM_j inv_ij: the sum of the gi the force arithmetic forms anyway, one more packed fma per pair of
// interactions and R more packed accumulators.  The body's own term GM_i / soft is orders of magnitude above the pair terms
// where the softening is small, so it never enters an fp32 sum: the accumulation is phi = fma(gi, pm, phi) with a wave-uniform
// pm that is 0 in the layout tile holding the i body and 1 elsewhere (murb_sweep_tile; the nearest form's sign, in kind), and that tile's terms are
// added behind the loop from the records in memory with the own slot left out (murb_pot_own_tile).  The fixed sweep's wave has
// its R bodies in one tile and one pm (RT = 1).  The active sweep's R bodies come from the list and can lie in R tiles: there
// pm is per body (RT = R) and murb_pot_own_tile adds a tile to its own bodies alone, so that every body's sum receives "all
// other tiles in layout order, then its own" whoever shares its wave, and phi does not depend on the list's order.
// Padding has GM = 0: its gi is +0 and needs no mask.  The loop nest keeps ONE copy of the arithmetic.
template <int RT>
__device__ __forceinline__ bool murb_pot_tile_own(const int tile, const int (&self_tile)[RT])   // wave-uniform
{
    bool m = false;
#pragma unroll
    for (int r = 0; r < RT; ++r) m |= self_tile[r] == tile;
    return m;
}

// GM_j * inv of one i body and one j body behind the loop, in single instructions that give the packed ones' bits
__device__ __forceinline__ float murb_pot_gi_single(const float xj, const float yj, const float zj, const float gj,
                                                    const float xi, const float yi, const float zi, const float soft2)
{
    const float inv = __builtin_amdgcn_rsqf(murb_nn_r2_single(xj, yj, zj, xi, yi, zi, soft2));
#if defined(__HIP_DEVICE_COMPILE__)
    float g;
    asm("v_mul_f32 %0, %1, %2" : "=v"(g) : "v"(gj), "v"(inv));
    return g;
#else
    return gj * inv;
#endif
}

// The terms of one tile that holds own bodies, from the records in memory, every body's own SLOT left out (another body at the
// same place counts).  Runs after the loop; the order is fixed: lane steps rising, the two slots of a pair in their halves.
template <int R, bool EACH = false>
__device__ __forceinline__ void murb_pot_own_tile(const float4* rec, const int lane, const int tile,
                                                  const float (&xi)[R], const float (&yi)[R], const float (&zi)[R], const float soft2,
                                                  murb_f2 (&ph)[R], const int (&self)[R])
{
#pragma unroll 1
    for (int qs = 0; qs < MURB_TILE_PAIRS / 64; ++qs) {
        const unsigned long ra = (unsigned long)tile * MURB_TILE_F4 + qs * 64 + lane;
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
        const int j0 = tile * MURB_TILE_BODIES + 2 * (qs * 64 + lane);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float gx = murb_pot_gi_single(A.x, A.z, B.x, B.z, xi[r], yi[r], zi[r], soft2);
            const float gy = murb_pot_gi_single(A.y, A.w, B.y, B.w, xi[r], yi[r], zi[r], soft2);
            if constexpr (EACH) {   // the wave's bodies lie in several tiles: a body takes the terms of its own tile alone
                const bool other = self[r] / MURB_TILE_BODIES != tile;   // wave-uniform; + 0 changes no bit of a sum of positive terms
                ph[r].x += other || j0 == self[r] ? 0.f : gx;
                ph[r].y += other || j0 + 1 == self[r] ? 0.f : gy;
                continue;
            }
            ph[r].x += j0 == self[r] ? 0.f : gx;
            ph[r].y += j0 + 1 == self[r] ? 0.f : gy;
        }
    }
}

// ---- the inner tile step of both sweeps ---------------------------------------------------------------------------------------
// One staged tile against the wave's i bodies: the load and unpack of a lane step and the pair arithmetic, with the side
// product beside it.  self_tile: the layout tiles the wave's bodies lie in, one for the wave (RT = 1) or one per body (RT = R).
// No pair is excluded here; what must not count is masked per tile, wave-uniformly, each form in its own way:
//   Nearest    a masked tile (murb_nn_tile_masked) runs the same code with the minima's signs set: r2 >= 0, so nothing is
//              smaller than -mn, the minimum stays and no step is recorded; the signs are cleared behind the tile.  That is 8
//              vector instructions per masked or unmasked tile of 1 900.
//   Contact    gap2 may be negative, so the sign trick does not carry over: a masked tile subtracts -inf instead of soft2 (a
//              select per tile), every gap2 of it is +inf and nothing is recorded.
//   Potential  phi = fma(gi, pm, phi) with pm 0 in the body's OWN tile alone, whatever tiles the wave's other bodies lie in,
//              and 1 elsewhere.
// So the loop nest keeps ONE copy of the arithmetic (a second, masked copy as the other arm of a branch made the register
// allocator spill hundreds of values in both arms).  murb_side_masked_tile and murb_pot_own_tile look at such a tile's pairs
// after the loop.  mn, st, ri, ph: what the form in question keeps; the others leave them alone.
template <int R, MurbSide SIDE, int RT>
__device__ __forceinline__ void murb_sweep_tile(const float4* tq, const float4* tv, const int lane, const int tile,
                                                const int (&self_tile)[RT], const int count,
                                                const float (&xi)[R], const float (&yi)[R], const float (&zi)[R],
                                                const float (&ui)[R], const float (&vi)[R], const float (&wi)[R],
                                                const float (&ri)[R], const float soft2,
                                                murb_f2 (&ax)[R], murb_f2 (&ay)[R], murb_f2 (&az)[R],
                                                murb_f2 (&jx)[R], murb_f2 (&jy)[R], murb_f2 (&jz)[R],
                                                float (&mn)[R], int (&st)[R], murb_f2 (&ph)[R])
{
    constexpr bool NN = SIDE == MurbSide::Nearest, CT = SIDE == MurbSide::Contact, POT = SIDE == MurbSide::Potential;
    static_assert(RT == 1 || RT == R, "one tile for the wave, or one per body");
    float c = soft2, pm[RT];
    if constexpr (NN) {
        const float sign = murb_nn_tile_masked<RT>(tile, self_tile, count) ? -1.f : 1.f;   // wave-uniform
#pragma unroll
        for (int r = 0; r < R; ++r) mn[r] *= sign;
    }
    if constexpr (CT) {
        c = murb_nn_tile_masked<RT>(tile, self_tile, count) ? -__builtin_inff() : soft2;   // wave-uniform, kept in a vector register: no scalar one is free
        asm volatile("" : "+v"(c));
    }
    if constexpr (POT) {
#pragma unroll
        for (int r = 0; r < RT; ++r) pm[r] = self_tile[r] == tile ? 0.f : 1.f;   // wave-uniform
    }
#pragma unroll
    for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
        const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
        const float4 VA = tv[q + lane], VB = tv[q + lane + MURB_TILE_PAIRS];
        const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
        const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y}, rj = {VB.z, VB.w};   // rj: the contact form's radii
        const int S = tile * (MURB_TILE_PAIRS / 64) + q / 64;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            murb_f2 r2, gi;
            murb_interact_jerk_pk_gi(xj, yj, zj, gj, uj, vj, wj, xi[r], yi[r], zi[r], ui[r], vi[r], wi[r], soft2,
                                     ax[r], ay[r], az[r], jx[r], jy[r], jz[r], r2, gi);
            if constexpr (POT) ph[r] = __builtin_elementwise_fma(gi, (murb_f2)(pm[RT == 1 ? 0 : r]), ph[r]);
            if constexpr (NN || CT) {
                murb_f2 g = r2;
                if constexpr (CT) {
                    const murb_f2 s = rj + ri[r];
                    const murb_f2 e = r2 - c;
                    g = __builtin_elementwise_fma(-s, s, e);
                }
                const float m = __builtin_fminf(__builtin_fminf(mn[r], g.x), g.y);
                st[r] = m < mn[r] ? S : st[r];
                mn[r] = m;
            }
        }
    }
    if constexpr (NN) {
#pragma unroll
        for (int r = 0; r < R; ++r) mn[r] = __builtin_fabsf(mn[r]);
    }
}

#endif
