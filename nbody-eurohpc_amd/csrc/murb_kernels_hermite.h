// gfx950 (CDNA4) kernels of the 4th-order Hermite predictor-corrector (Makino & Aarseth 1992), option "integrator" 2.
// Device code only; included by murbhip.hip.  Replaces the reference's first-order update (Bodies.cpp:260-278).
//
// One step = predictor, ONE all-pairs sweep at the predicted state, corrector:
//     predict   qp = q + v dt + a0 dt^2/2 + j0 dt^3/6          vp = v + a0 dt + j0 dt^2/2
//     evaluate  (a1, j1) at (qp, vp)
//     correct   v1 = v + (a0 + a1) dt/2 + (j0 - j1) dt^2/12
//               q1 = q + (v + v1) dt/2  + (a0 - a1) dt^2/12     (a0, j0) <- (a1, j1)
// The sweep computes accelerations and their time derivatives ("jerks") together, fp32, full N^2 form:
//     d = q_j - q_i    w = v_j - v_i    s = GM_j (|d|^2 + soft^2)^(-3/2)
//     a_i += s d       j_i += s (w - 3 (d.w) inv^2 d)           inv = (|d|^2 + soft^2)^(-1/2)
// (the j == i term is exactly 0 in both sums: d = w = 0 and soft > 0; a zero-mass slot has s = 0).
//
// Mapping: that of the one-sided force kernel (murb_kernels.h) — the wave's R i bodies wave-uniform in SGPRs, now six
// values each, the j bodies two per lane in the pair layout, so a stage is one 8 KiB position tile plus one 8 KiB velocity
// tile (velocities have the same layout), both linear copies global -> LDS, four ds_read_b128 feeding 2 R interactions per
// lane.  Per pair of interactions 26 packed instructions + 2 v_rsq_f32 (murb_interact_pk: 12 + 2).  j is split into
// chunks over gridDim.y; every (chunk, i) gets six floats in the partial rows, which the corrector adds in fixed order.
//
// Two ways to drive a step.  Fixed: dt is a launch argument (murbhip_step).  Adaptive: dt, the clock and the end of the run
// live in a control block in device memory and the device chooses every step's size (murbhip_evolve; second half of this
// file).  Sweep, predictor and corrector are device functions that both sets of kernels call.
#ifndef MURB_KERNELS_HERMITE_H_
#define MURB_KERNELS_HERMITE_H_

#include "murb_field.h"
#include "murb_kernels.h"

struct MurbJerkArgs {
    const float4* rec;    // positions + GM, all slots (murb_layout.h)
    const float4* vel;    // velocities, same layout (one shard: the local slice is all slots)
    float4* part_a;       // partial sums: part_a[chunk * stride + slot] = {ax, ay, az, 0}
    float4* part_j;       // ... and {jx, jy, jz, 0}
    int tiles;            // layout tiles swept as j
    int nchunks;          // gridDim.y
    unsigned int stride;  // slots per partial row
    float soft2;
};

// ---- one i body against two j bodies (packed): acceleration and jerk ----------------------------------------------
// 6 pk_add + 6 pk_fma (|d|^2 + soft^2, d.w) + 2 rsq + 5 pk_mul + 9 pk_fma
// (the _r2 form hands out the pair of |d|^2 + soft^2 the force arithmetic uses: the nearest-neighbour sweeps keep its minimum;
// the _gi form also the pair of GM_j * inv it makes on the way to s: the potential sweeps keep its sum)
__device__ __forceinline__ void murb_interact_jerk_pk_gi(const murb_f2 xj, const murb_f2 yj, const murb_f2 zj, const murb_f2 gj,
                                                         const murb_f2 uj, const murb_f2 vj, const murb_f2 wj,
                                                         const float xi, const float yi, const float zi,
                                                         const float ui, const float vi, const float wi, const float soft2,
                                                         murb_f2& ax, murb_f2& ay, murb_f2& az,
                                                         murb_f2& jx, murb_f2& jy, murb_f2& jz, murb_f2& r2, murb_f2& gi)
{
    const murb_f2 dx = xj - xi, dy = yj - yi, dz = zj - zi;
    const murb_f2 wx = uj - ui, wy = vj - vi, wz = wj - wi;
    r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
    r2 = __builtin_elementwise_fma(dy, dy, r2);
    r2 = __builtin_elementwise_fma(dz, dz, r2);
    murb_f2 dw = dx * wx;
    dw = __builtin_elementwise_fma(dy, wy, dw);
    dw = __builtin_elementwise_fma(dz, wz, dw);
    murb_f2 inv;
    inv.x = __builtin_amdgcn_rsqf(r2.x);
    inv.y = __builtin_amdgcn_rsqf(r2.y);
    const murb_f2 inv2 = inv * inv;
    gi = gj * inv;
    const murb_f2 s = gi * inv2;            // GM_j * inv^3, never G*inv^3 alone (fp32 range)
    const murb_f2 c = (dw * inv2) * -3.0f;  // -3 (d.w) / (|d|^2 + soft^2)
    ax = __builtin_elementwise_fma(s, dx, ax);
    ay = __builtin_elementwise_fma(s, dy, ay);
    az = __builtin_elementwise_fma(s, dz, az);
    jx = __builtin_elementwise_fma(s, __builtin_elementwise_fma(c, dx, wx), jx);
    jy = __builtin_elementwise_fma(s, __builtin_elementwise_fma(c, dy, wy), jy);
    jz = __builtin_elementwise_fma(s, __builtin_elementwise_fma(c, dz, wz), jz);
}

__device__ __forceinline__ void murb_interact_jerk_pk_r2(const murb_f2 xj, const murb_f2 yj, const murb_f2 zj, const murb_f2 gj,
                                                         const murb_f2 uj, const murb_f2 vj, const murb_f2 wj,
                                                         const float xi, const float yi, const float zi,
                                                         const float ui, const float vi, const float wi, const float soft2,
                                                         murb_f2& ax, murb_f2& ay, murb_f2& az,
                                                         murb_f2& jx, murb_f2& jy, murb_f2& jz, murb_f2& r2)
{
    murb_f2 gi;
    murb_interact_jerk_pk_gi(xj, yj, zj, gj, uj, vj, wj, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, r2, gi);
}

__device__ __forceinline__ void murb_interact_jerk_pk(const murb_f2 xj, const murb_f2 yj, const murb_f2 zj, const murb_f2 gj,
                                                      const murb_f2 uj, const murb_f2 vj, const murb_f2 wj,
                                                      const float xi, const float yi, const float zi,
                                                      const float ui, const float vi, const float wi, const float soft2,
                                                      murb_f2& ax, murb_f2& ay, murb_f2& az,
                                                      murb_f2& jx, murb_f2& jy, murb_f2& jz)
{
    murb_f2 r2;
    murb_interact_jerk_pk_r2(xj, yj, zj, gj, uj, vj, wj, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, r2);
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

__device__ __forceinline__ unsigned int murb_wave_min_bits(const float v);   // below

struct MurbNNJerkArgs : MurbJerkArgs {
    int count;   // real bodies: slots >= count are padding
};

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

// One staged tile against the wave's i bodies: the sweep's inner loop with the minimum beside it, no exclusion.  A masked
// tile runs the same code with the minima's signs set: r2 >= 0, so nothing is smaller than -mn, the minimum stays and no
// step is recorded; the signs are cleared behind the tile.  That is 8 vector instructions per masked or unmasked tile of
// 1 900, and the loop nest keeps ONE copy of the arithmetic (a second, masked copy as the other arm of a branch made the
// register allocator spill hundreds of values in both arms).  murb_nn_masked_tile looks at such a tile's pairs after the loop.
template <int R>
__device__ __forceinline__ void murb_nn_tile(const float4* tq, const float4* tv, const int lane, const int tile, const bool masked,
                                             const float (&xi)[R], const float (&yi)[R], const float (&zi)[R],
                                             const float (&ui)[R], const float (&vi)[R], const float (&wi)[R], const float soft2,
                                             murb_f2 (&ax)[R], murb_f2 (&ay)[R], murb_f2 (&az)[R],
                                             murb_f2 (&jx)[R], murb_f2 (&jy)[R], murb_f2 (&jz)[R],
                                             float (&mn)[R], int (&st)[R])
{
    const float sign = masked ? -1.f : 1.f;   // wave-uniform
#pragma unroll
    for (int r = 0; r < R; ++r) mn[r] *= sign;
#pragma unroll
    for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
        const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
        const float4 VA = tv[q + lane], VB = tv[q + lane + MURB_TILE_PAIRS];
        const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
        const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y};
        const int S = tile * (MURB_TILE_PAIRS / 64) + q / 64;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            murb_f2 r2;
            murb_interact_jerk_pk_r2(xj, yj, zj, gj, uj, vj, wj, xi[r], yi[r], zi[r], ui[r], vi[r], wi[r], soft2,
                                     ax[r], ay[r], az[r], jx[r], jy[r], jz[r], r2);
            const float m = __builtin_fminf(__builtin_fminf(mn[r], r2.x), r2.y);
            st[r] = m < mn[r] ? S : st[r];
            mn[r] = m;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) mn[r] = __builtin_fabsf(mn[r]);
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

// The pairs of one masked tile, from the records in memory: r2 alone, formed like the sweep forms it (the same bits), with
// the body itself and the padding left out.  Runs after the loop, so the steps no longer rise: an equal r2 at an earlier
// step takes the place.
template <int R>
__device__ __forceinline__ void murb_nn_masked_tile(const float4* rec, const int lane, const int tile,
                                                    const float (&xi)[R], const float (&yi)[R], const float (&zi)[R], const float soft2,
                                                    float (&mn)[R], int (&st)[R], const int (&self)[R], const int count)
{
#pragma unroll 1
    for (int qs = 0; qs < MURB_TILE_PAIRS / 64; ++qs) {
        const unsigned long ra = (unsigned long)tile * MURB_TILE_F4 + qs * 64 + lane;
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
        const int S = tile * (MURB_TILE_PAIRS / 64) + qs;
        const int j0 = tile * MURB_TILE_BODIES + 2 * (qs * 64 + lane);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float r2x = murb_nn_r2_single(A.x, A.z, B.x, xi[r], yi[r], zi[r], soft2);
            float r2y = murb_nn_r2_single(A.y, A.w, B.y, xi[r], yi[r], zi[r], soft2);
            if (j0 == self[r] || j0 >= count) r2x = __builtin_inff();
            if (j0 + 1 == self[r] || j0 + 1 >= count) r2y = __builtin_inff();
            const float m = __builtin_fminf(r2x, r2y);
            if (m < mn[r] || (m == mn[r] && S < st[r])) { mn[r] = m; st[r] = S; }
        }
    }
}

// After the loop: the slot behind every lane's minimum, the fold over the wave; lane r gets body r's (r2 bits, slot).
template <int R>
__device__ __forceinline__ void murb_nn_finish(const float4* rec, const int lane, const float (&xi)[R], const float (&yi)[R],
                                               const float (&zi)[R], const float soft2, const float (&mn)[R], const int (&st)[R],
                                               const int (&self)[R], const int count, unsigned int& out_r2, unsigned int& out_idx)
{
    out_r2 = MURB_F32_INF_BITS;
    out_idx = MURB_NN_NONE;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int p = st[r] * 64 + lane;   // the pair of slots of lane step st[r]
        const unsigned long ra = murb_rec_a((unsigned long)p);
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
        const float r2x = murb_nn_r2_single(A.x, A.z, B.x, xi[r], yi[r], zi[r], soft2);
        const int j0 = 2 * p;
        const bool first = r2x == mn[r] && j0 != self[r] && j0 < count;
        const unsigned int idx = mn[r] < __builtin_inff() ? (unsigned int)(first ? j0 : j0 + 1) : MURB_NN_NONE;
        const unsigned int mb = murb_wave_min_bits(mn[r]);
        const unsigned int cand = __builtin_bit_cast(unsigned int, mn[r]) == mb ? idx : MURB_NN_NONE;
        const unsigned int ib = murb_wave_min_bits(__builtin_bit_cast(float, cand));   // an unsigned minimum of the bits
        if (lane == r) { out_r2 = mb; out_idx = ib; }
    }
}

// Where rows are added up in chunk order: the lexicographic minimum of (r2 bits, slot) beside the sums.
__device__ __forceinline__ void murb_nn_fold_row(unsigned int& r2, unsigned int& idx, const float4 u, const float4 w)
{
    const unsigned int ub = __builtin_bit_cast(unsigned int, u.w), ib = __builtin_bit_cast(unsigned int, w.w);
    if (ub < r2 || (ub == r2 && ib < idx)) { r2 = ub; idx = ib; }
}

__device__ __forceinline__ void murb_nn_store(int* nn_idx, float* nn_r2, const int s, const unsigned int r2, const unsigned int idx)
{
    nn_idx[s] = idx == MURB_NN_NONE ? -1 : (int)idx;
    nn_r2[s] = idx == MURB_NN_NONE ? __builtin_inff() : __builtin_bit_cast(float, r2);
}

// A body that took the step with r2 <= thr is a hit: it takes a place in the list (a vector atomic, like the active list's).
__device__ __forceinline__ void murb_enc_test(unsigned int* hits, MurbEncList* list, const float thr, const int i,
                                              const unsigned int r2, const unsigned int idx)
{
    if (idx == MURB_NN_NONE || !(__builtin_bit_cast(float, r2) <= thr)) return;
    const unsigned int at = atomicAdd(hits, 1u);
    if (at < MURB_ENC_CAP) { list->i[at] = i; list->j[at] = (int)idx; list->r2[at] = __builtin_bit_cast(float, r2); }
}

// ---- contact by radii beside the sweep (option "contact"; include/murbhip.h has the definition) ------------------------------
// The nearest-neighbour scheme with gap2 = (r2 - soft2) - (R_i + R_j)^2 in r2's place: a packed add for the sum of radii (the
// j radii ride in the two spare lanes of the velocity B record, the i radii in scalar registers), a packed add for r2 - soft2
// and a packed fma, then the minimum, the compare and the select of the lane step.  gap2 may be negative, so the sign trick of
// murb_nn_tile does not carry over: a masked tile subtracts -inf instead of soft2 (a wave-uniform select per tile), every
// gap2 of it is +inf and nothing is recorded.  Where (gap2, slot) are folded they travel as an order-preserving unsigned key
// (murb_ct_key); the per-slot store decodes it.
#define MURB_CT_NONE_KEY 0xff800000u   // the key of +inf: "no candidate"

__device__ __forceinline__ unsigned int murb_ct_key(const float g)
{
    const unsigned int b = __builtin_bit_cast(unsigned int, g);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}

__device__ __forceinline__ float murb_ct_value(const unsigned int k)
{
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

template <int R>
__device__ __forceinline__ void murb_ct_tile(const float4* tq, const float4* tv, const int lane, const int tile, const bool masked,
                                             const float (&xi)[R], const float (&yi)[R], const float (&zi)[R],
                                             const float (&ui)[R], const float (&vi)[R], const float (&wi)[R],
                                             const float (&ri)[R], const float soft2,
                                             murb_f2 (&ax)[R], murb_f2 (&ay)[R], murb_f2 (&az)[R],
                                             murb_f2 (&jx)[R], murb_f2 (&jy)[R], murb_f2 (&jz)[R],
                                             float (&mn)[R], int (&st)[R])
{
    float c = masked ? -__builtin_inff() : soft2;   // wave-uniform, kept in a vector register: no scalar one is free
    asm volatile("" : "+v"(c));
#pragma unroll
    for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
        const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
        const float4 VA = tv[q + lane], VB = tv[q + lane + MURB_TILE_PAIRS];
        const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
        const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y}, rj = {VB.z, VB.w};
        const int S = tile * (MURB_TILE_PAIRS / 64) + q / 64;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            murb_f2 r2;
            murb_interact_jerk_pk_r2(xj, yj, zj, gj, uj, vj, wj, xi[r], yi[r], zi[r], ui[r], vi[r], wi[r], soft2,
                                     ax[r], ay[r], az[r], jx[r], jy[r], jz[r], r2);
            const murb_f2 s = rj + ri[r];
            const murb_f2 e = r2 - c;
            const murb_f2 g = __builtin_elementwise_fma(-s, s, e);
            const float m = __builtin_fminf(__builtin_fminf(mn[r], g.x), g.y);
            st[r] = m < mn[r] ? S : st[r];
            mn[r] = m;
        }
    }
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

// The pairs of one masked tile from the records in memory, the body itself and the padding left out (murb_nn_masked_tile).
template <int R>
__device__ __forceinline__ void murb_ct_masked_tile(const float4* rec, const float4* vel, const int lane, const int tile,
                                                    const float (&xi)[R], const float (&yi)[R], const float (&zi)[R],
                                                    const float (&ri)[R], const float soft2,
                                                    float (&mn)[R], int (&st)[R], const int (&self)[R], const int count)
{
#pragma unroll 1
    for (int qs = 0; qs < MURB_TILE_PAIRS / 64; ++qs) {
        const unsigned long ra = (unsigned long)tile * MURB_TILE_F4 + qs * 64 + lane;
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS], VB = vel[ra + MURB_TILE_PAIRS];
        const int S = tile * (MURB_TILE_PAIRS / 64) + qs;
        const int j0 = tile * MURB_TILE_BODIES + 2 * (qs * 64 + lane);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float gx = murb_ct_gap2_single(A.x, A.z, B.x, VB.z, xi[r], yi[r], zi[r], ri[r], soft2);
            float gy = murb_ct_gap2_single(A.y, A.w, B.y, VB.w, xi[r], yi[r], zi[r], ri[r], soft2);
            if (j0 == self[r] || j0 >= count) gx = __builtin_inff();
            if (j0 + 1 == self[r] || j0 + 1 >= count) gy = __builtin_inff();
            const float m = __builtin_fminf(gx, gy);
            if (m < mn[r] || (m == mn[r] && S < st[r])) { mn[r] = m; st[r] = S; }
        }
    }
}

// After the loop: the slot behind every lane's minimum, the fold over the wave; lane r gets body r's (key of gap2, slot).
template <int R>
__device__ __forceinline__ void murb_ct_finish(const float4* rec, const float4* vel, const int lane,
                                               const float (&xi)[R], const float (&yi)[R], const float (&zi)[R], const float (&ri)[R],
                                               const float soft2, const float (&mn)[R], const int (&st)[R],
                                               const int (&self)[R], const int count, unsigned int& out_key, unsigned int& out_idx)
{
    out_key = MURB_CT_NONE_KEY;
    out_idx = MURB_NN_NONE;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int p = st[r] * 64 + lane;   // the pair of slots of lane step st[r]
        const unsigned long ra = murb_rec_a((unsigned long)p);
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS], VB = vel[ra + MURB_TILE_PAIRS];
        const float gx = murb_ct_gap2_single(A.x, A.z, B.x, VB.z, xi[r], yi[r], zi[r], ri[r], soft2);
        const int j0 = 2 * p;
        const bool first = gx == mn[r] && j0 != self[r] && j0 < count;
        const unsigned int idx = mn[r] < __builtin_inff() ? (unsigned int)(first ? j0 : j0 + 1) : MURB_NN_NONE;
        const unsigned int key = murb_ct_key(mn[r]);
        const unsigned int kb = murb_wave_min_bits(__builtin_bit_cast(float, key));   // an unsigned minimum of the bits
        const unsigned int cand = key == kb ? idx : MURB_NN_NONE;
        const unsigned int ib = murb_wave_min_bits(__builtin_bit_cast(float, cand));
        if (lane == r) { out_key = kb; out_idx = ib; }
    }
}

// The per-slot store and the hit test of the correctors: the key decoded; a body that took the step with gap2 <= 0 is a hit.
__device__ __forceinline__ void murb_ct_store(int* nn_idx, float* nn_r2, const int s, const unsigned int key, const unsigned int idx)
{
    nn_idx[s] = idx == MURB_NN_NONE ? -1 : (int)idx;
    nn_r2[s] = idx == MURB_NN_NONE ? __builtin_inff() : murb_ct_value(key);
}

__device__ __forceinline__ void murb_ct_test(unsigned int* hits, MurbEncList* list, const int i, const unsigned int key, const unsigned int idx)
{
    if (idx == MURB_NN_NONE || !(murb_ct_value(key) <= 0.f)) return;
    const unsigned int at = atomicAdd(hits, 1u);
    if (at < MURB_ENC_CAP) { list->i[at] = i; list->j[at] = (int)idx; list->r2[at] = murb_ct_value(key); }
}

// ---- per-body potential beside the sweep (option "potential"; include/murbhip.h has the definition) --------------------------
// phi_i = sum_{j != i} GM_j inv_ij: the sum of the gi the force arithmetic forms anyway, one more packed fma per pair of
// interactions and R more packed accumulators.  The body's own term GM_i / soft is orders of magnitude above the pair terms
// where the softening is small, so it never enters an fp32 sum: the accumulation is phi = fma(gi, pm, phi) with a wave-uniform
// pm that is 0 in the layout tile holding the i body and 1 elsewhere (murb_nn_tile's sign, in kind), and that tile's terms are
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

template <int R, int RT>
__device__ __forceinline__ void murb_pot_tile(const float4* tq, const float4* tv, const int lane, const int tile, const int (&self_tile)[RT],
                                              const float (&xi)[R], const float (&yi)[R], const float (&zi)[R],
                                              const float (&ui)[R], const float (&vi)[R], const float (&wi)[R], const float soft2,
                                              murb_f2 (&ax)[R], murb_f2 (&ay)[R], murb_f2 (&az)[R],
                                              murb_f2 (&jx)[R], murb_f2 (&jy)[R], murb_f2 (&jz)[R], murb_f2 (&ph)[R])
{
    static_assert(RT == 1 || RT == R, "one tile for the wave, or one per body");
    float pm[RT];   // wave-uniform, per body: 0 in the body's OWN tile alone, whatever tiles the wave's other bodies lie in
#pragma unroll
    for (int r = 0; r < RT; ++r) pm[r] = self_tile[r] == tile ? 0.f : 1.f;
#pragma unroll
    for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
        const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
        const float4 VA = tv[q + lane], VB = tv[q + lane + MURB_TILE_PAIRS];
        const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
        const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            murb_f2 r2, gi;
            murb_interact_jerk_pk_gi(xj, yj, zj, gj, uj, vj, wj, xi[r], yi[r], zi[r], ui[r], vi[r], wi[r], soft2,
                                     ax[r], ay[r], az[r], jx[r], jy[r], jz[r], r2, gi);
            ph[r] = __builtin_elementwise_fma(gi, (murb_f2)(pm[RT == 1 ? 0 : r]), ph[r]);
        }
    }
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

// ---- the sweep -------------------------------------------------------------------------------------------------------
// grid.x = i groups of WAVES*R bodies, grid.y = j chunks.  LDS: STAGE position tiles + STAGE velocity tiles (16 KiB a stage).
// The body is a device function so that the adaptive launch (murb_force_jerk_adaptive_kernel, below) runs the same code.
// MODE 1: the nearest-neighbour form, 2: the contact form, 3: the potential form (Args = MurbNNJerkArgs); the plain form's code
// does not change with them.  NN names what the three share (the copy in whole rounds, the kernel arguments read again behind
// the loop); the potential form (POT) keeps R packed sums in the place of the minima and steps.
template <int R, int WAVES, int STAGE, int MODE = 0, typename Args = MurbJerkArgs>
__device__ __forceinline__ void murb_force_jerk_sweep(const Args a)
{
    constexpr bool NN = MODE != 0, CT = MODE == 2, POT = MODE == 3;
    static_assert(R % 2 == 0 && MURB_TILE_BODIES % (WAVES * R) == 0, "i groups must tile the layout");
    __shared__ float4 lds[2 * STAGE * MURB_TILE_F4];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i_slot = (blockIdx.x * WAVES + wave) * R;   // wave-uniform; the host keeps the grid inside the slots

    // the wave's R i bodies -> scalar registers
    float xi[R], yi[R], zi[R], ui[R], vi[R], wi[R], ri[R];   // ri: the contact form's radii
    {
        const unsigned long ra = murb_rec_a((unsigned long)(i_slot >> 1));
#pragma unroll
        for (int h = 0; h < R / 2; ++h) {
            const float4 A = a.rec[ra + h], B = a.rec[ra + h + MURB_TILE_PAIRS];
            const float4 VA = a.vel[ra + h], VB = a.vel[ra + h + MURB_TILE_PAIRS];
            xi[2 * h] = A.x; xi[2 * h + 1] = A.y; yi[2 * h] = A.z; yi[2 * h + 1] = A.w; zi[2 * h] = B.x; zi[2 * h + 1] = B.y;
            ui[2 * h] = VA.x; ui[2 * h + 1] = VA.y; vi[2 * h] = VA.z; vi[2 * h + 1] = VA.w; wi[2 * h] = VB.x; wi[2 * h + 1] = VB.y;
            if constexpr (CT) { ri[2 * h] = VB.z; ri[2 * h + 1] = VB.w; }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            xi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, xi[r])));
            yi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, yi[r])));
            zi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, zi[r])));
            ui[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ui[r])));
            vi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, vi[r])));
            wi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wi[r])));
            if constexpr (CT) asm volatile("" : "+v"(ri[r]));   // every lane has loaded it: it stays in a vector register (no scalar one is free)
        }
    }

    // this block's j chunk: tiles [vt0, vt1)
    const int chunk = blockIdx.y;
    const int vt0 = (int)(((long)a.tiles * chunk) / a.nchunks);
    const int vt1 = (int)(((long)a.tiles * (chunk + 1)) / a.nchunks);
    const float soft2 = a.soft2;

    murb_f2 ax[R], ay[R], az[R], jx[R], jy[R], jz[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        ax[r] = (murb_f2)(0.f); ay[r] = (murb_f2)(0.f); az[r] = (murb_f2)(0.f);
        jx[r] = (murb_f2)(0.f); jy[r] = (murb_f2)(0.f); jz[r] = (murb_f2)(0.f);
    }
    float mn[R];   // NN: the lane's smallest r2 per i body, and the lane step it fell at
    int st[R], self_tile[1] = {0}, count = 0;
    murb_f2 ph[R];   // POT: the sums of GM_j * inv
    if constexpr (NN) {
        if constexpr (!POT) count = a.count;
        self_tile[0] = i_slot / MURB_TILE_BODIES;   // a wave's i bodies lie in one layout tile
#pragma unroll
        for (int r = 0; r < R; ++r) { mn[r] = __builtin_inff(); st[r] = 0; ph[r] = (murb_f2)(0.f); }
    }

    for (int vs = vt0; vs < vt1; vs += STAGE) {
        const int nt = (vt1 - vs) < STAGE ? (vt1 - vs) : STAGE;
        __syncthreads();   // previous stage fully consumed
        for (int t = 0; t < nt; ++t) {
            const float4* srcq = a.rec + (unsigned long)(vs + t) * MURB_TILE_F4;
            const float4* srcv = a.vel + (unsigned long)(vs + t) * MURB_TILE_F4;
            if constexpr (NN) {   // whole rounds, like the active sweep's copy: no bounds tests held in scalar registers
                static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
#pragma unroll
                for (int c = 0; c < MURB_TILE_F4 / (WAVES * 64); ++c) {
                    const int k = threadIdx.x + c * WAVES * 64;
                    lds[(2 * t) * MURB_TILE_F4 + k] = srcq[k];
                    lds[(2 * t + 1) * MURB_TILE_F4 + k] = srcv[k];
                }
                continue;
            }
#pragma unroll
            for (int k = threadIdx.x; k < MURB_TILE_F4; k += WAVES * 64) {
                lds[(2 * t) * MURB_TILE_F4 + k] = srcq[k];
                lds[(2 * t + 1) * MURB_TILE_F4 + k] = srcv[k];
            }
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const float4* tq = lds + (2 * t) * MURB_TILE_F4;
            const float4* tv = tq + MURB_TILE_F4;
            if constexpr (POT) {
                murb_pot_tile<R, 1>(tq, tv, lane, vs + t, self_tile, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, ph);
                continue;
            }
            if constexpr (NN) {
                const bool masked = murb_nn_tile_masked<1>(vs + t, self_tile, count);   // wave-uniform
                if constexpr (CT) murb_ct_tile<R>(tq, tv, lane, vs + t, masked, xi, yi, zi, ui, vi, wi, ri, soft2, ax, ay, az, jx, jy, jz, mn, st);
                else murb_nn_tile<R>(tq, tv, lane, vs + t, masked, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, mn, st);
                continue;
            }
#pragma unroll
            for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
                const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
                const float4 VA = tv[q + lane], VB = tv[q + lane + MURB_TILE_PAIRS];
                const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
                const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y};
#pragma unroll
                for (int r = 0; r < R; ++r)
                    murb_interact_jerk_pk(xj, yj, zj, gj, uj, vj, wj, xi[r], yi[r], zi[r], ui[r], vi[r], wi[r], soft2,
                                          ax[r], ay[r], az[r], jx[r], jy[r], jz[r]);
            }
        }
    }

    float nn_a = 0.f, nn_j = 0.f;   // the rows' fourth floats
    if constexpr (POT) {
        const auto* again = murb_kernarg_again<Args>();   // `a` is the kernel's first argument
        const float4* const rec = again->rec;
        int self[R], first = i_slot;
        asm volatile("" : "+s"(first));   // the bodies' slots are made here, not held through the loop
#pragma unroll
        for (int r = 0; r < R; ++r) self[r] = first + r;
        const int tiles = again->tiles, nchunks = again->nchunks;
        const int t0 = (int)(((long)tiles * chunk) / nchunks), t1 = (int)(((long)tiles * (chunk + 1)) / nchunks);   // vt0, vt1 again
        const int own = first / MURB_TILE_BODIES;
        if (own >= t0 && own < t1) murb_pot_own_tile<R>(rec, lane, own, xi, yi, zi, soft2, ph, self);   // wave-uniform
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float sp = murb_wave_sum(ph[r].x + ph[r].y);
            if (lane == r) nn_a = sp;   // part_j.w stays 0
        }
    } else if constexpr (NN) {
        const auto* again = murb_kernarg_again<Args>();   // `a` is the nearest-neighbour kernel's first argument
        const float4* const rec = again->rec;
        const int cnt = again->count;
        int self[R], first = i_slot;
        asm volatile("" : "+s"(first));   // the bodies' slots are made here, not held through the loop
#pragma unroll
        for (int r = 0; r < R; ++r) self[r] = first + r;
        const int tiles = again->tiles, nchunks = again->nchunks;
        const int t0 = (int)(((long)tiles * chunk) / nchunks), t1 = (int)(((long)tiles * (chunk + 1)) / nchunks);   // vt0, vt1 again
        const int own[1] = {first / MURB_TILE_BODIES};
        unsigned int nn_r2, nn_idx;
        if constexpr (CT) {
            const float4* const vel = again->vel;
            for (int tile = t0; tile < t1; ++tile)
                if (murb_nn_tile_masked<1>(tile, own, cnt)) murb_ct_masked_tile<R>(rec, vel, lane, tile, xi, yi, zi, ri, soft2, mn, st, self, cnt);
            murb_ct_finish<R>(rec, vel, lane, xi, yi, zi, ri, soft2, mn, st, self, cnt, nn_r2, nn_idx);
        } else {
            for (int tile = t0; tile < t1; ++tile)
                if (murb_nn_tile_masked<1>(tile, own, cnt)) murb_nn_masked_tile<R>(rec, lane, tile, xi, yi, zi, soft2, mn, st, self, cnt);
            murb_nn_finish<R>(rec, lane, xi, yi, zi, soft2, mn, st, self, cnt, nn_r2, nn_idx);
        }
        nn_a = __builtin_bit_cast(float, nn_r2);
        nn_j = __builtin_bit_cast(float, nn_idx);
    }

    // fold the 64 lanes x 2 halves of every accumulator; lane r keeps body r's totals
    float oa[3] = {0.f, 0.f, 0.f}, oj[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float sx = murb_wave_sum(ax[r].x + ax[r].y), sy = murb_wave_sum(ay[r].x + ay[r].y), sz = murb_wave_sum(az[r].x + az[r].y);
        const float tx = murb_wave_sum(jx[r].x + jx[r].y), ty = murb_wave_sum(jy[r].x + jy[r].y), tz = murb_wave_sum(jz[r].x + jz[r].y);
        if (lane == r) { oa[0] = sx; oa[1] = sy; oa[2] = sz; oj[0] = tx; oj[1] = ty; oj[2] = tz; }
    }
    if (lane < R) {
        if constexpr (NN) {
            const auto* again = murb_kernarg_again<Args>();
            const unsigned long at = (unsigned long)chunk * again->stride + (unsigned long)i_slot + lane;
            again->part_a[at] = make_float4(oa[0], oa[1], oa[2], nn_a);
            again->part_j[at] = make_float4(oj[0], oj[1], oj[2], nn_j);
        } else {
            const unsigned long at = (unsigned long)chunk * a.stride + (unsigned long)i_slot + lane;
            a.part_a[at] = make_float4(oa[0], oa[1], oa[2], nn_a);
            a.part_j[at] = make_float4(oj[0], oj[1], oj[2], nn_j);
        }
    }
}

template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) void murb_force_jerk_kernel(const MurbJerkArgs a)
{
    murb_force_jerk_sweep<R, WAVES, STAGE>(a);
}

// ---- predictor and corrector ------------------------------------------------------------------------------------------
// The project's convention for the reference update (murb_drift / murb_kick): no contraction, fp64 intermediates, ONE
// rounding to fp32 at the store, so that an fp64 restatement fed with the same fp32 q, v, a, j reproduces the update bit
// for bit.  The order of the additions is part of the definition (left to right as written); the coefficients are formed
// in fp64 from the fp32 dt: dt/2 = dt*0.5, dt^2/2 = dt*dt*0.5, dt^3/6 = dt*dt*dt/6, dt^2/12 = dt*dt/12.
struct MurbHermiteArgs {
    const float4* rec_in;   // current positions + GM, all slots
    float4* rec_out;        // predictor: the predicted records ; corrector: the other position buffer
    float4* vel;            // current velocities (the corrector updates them in place)
    float4* vel_out;        // predictor: the predicted velocities
    float* a0;              // ax | ay | az (stride each) of the remembered evaluation; the corrector replaces them
    float* j0;              // jx | jy | jz likewise
    const float4* part_a;   // corrector: partial rows of the sweep
    const float4* part_j;
    float* acc_out;         // corrector: the summed accelerations once more, where murbhip_download_acc reads them
    int nparts;             // rows to add, in index order
    int count;              // real bodies
    unsigned int stride;    // slots
    float dt;
    int update_state;       // corrector: 0 = only sum the rows into a0 / j0 (evaluation at the current state)
    int* nn_idx;            // "nearest": every slot's nearest neighbour and its r2, folded beside the row sums; null = off
    float* nn_r2;
    MurbEncList* enc;       // ... and the encounter list of murbhip_evolve
    int contact;            // "contact": the rows' fourth floats are (key of gap2, slot), kept in nn_idx / nn_r2; 2 = with the contact stop
    float* phi;             // "potential": part_a's fourth floats are partial potentials, added in chunk order beside a1; null = off
};

__device__ __forceinline__ float murb_hermite_predict_q(float q, float v, float a, float j, double dt, double c2, double c3)
{
#pragma clang fp contract(off)
    return (float)((((double)q + (double)v * dt) + (double)a * c2) + (double)j * c3);
}

__device__ __forceinline__ float murb_hermite_predict_v(float v, float a, float j, double dt, double c2)
{
#pragma clang fp contract(off)
    return (float)(((double)v + (double)a * dt) + (double)j * c2);
}

// v1 = v + (a0 + a1) dt/2 + (j0 - j1) dt^2/12
__device__ __forceinline__ float murb_hermite_correct_v(float v, float a0, float a1, float j0, float j1, double h, double c12)
{
#pragma clang fp contract(off)
    return (float)(((double)v + ((double)a0 + (double)a1) * h) + ((double)j0 - (double)j1) * c12);
}

// q1 = q + (v + v1) dt/2 + (a0 - a1) dt^2/12, v1 being the fp32 value just stored
__device__ __forceinline__ float murb_hermite_correct_q(float q, float v, float v1, float a0, float a1, double h, double c12)
{
#pragma clang fp contract(off)
    return (float)(((double)q + ((double)v + (double)v1) * h) + ((double)a0 - (double)a1) * c12);
}

// One thread per pair of slots (lp); slots past `count` (zero-mass padding) are copied unchanged.  The bodies of predictor
// and corrector are device functions taking dt, so that the fixed-step kernels (dt a launch argument) and the adaptive
// ones (dt read from the control block, below) run the same code.
__device__ __forceinline__ void murb_hermite_predict_pair(const MurbHermiteArgs& a, const int lp, const float dt32)
{
#pragma clang fp contract(off)
    const int s0 = 2 * lp;
    const unsigned long ra = murb_rec_a((unsigned long)lp);
    float4 A = a.rec_in[ra], B = a.rec_in[ra + MURB_TILE_PAIRS];
    float4 VA = a.vel[ra], VB = a.vel[ra + MURB_TILE_PAIRS];
    const double dt = (double)dt32, c2 = dt * dt * 0.5, c3 = dt * dt * dt / 6.0;
    const unsigned int n = a.stride;
    if (s0 < a.count) {
        const float ax = a.a0[s0], ay = a.a0[n + s0], az = a.a0[2u * n + s0];
        const float jx = a.j0[s0], jy = a.j0[n + s0], jz = a.j0[2u * n + s0];
        A.x = murb_hermite_predict_q(A.x, VA.x, ax, jx, dt, c2, c3);
        A.z = murb_hermite_predict_q(A.z, VA.z, ay, jy, dt, c2, c3);
        B.x = murb_hermite_predict_q(B.x, VB.x, az, jz, dt, c2, c3);
        VA.x = murb_hermite_predict_v(VA.x, ax, jx, dt, c2);
        VA.z = murb_hermite_predict_v(VA.z, ay, jy, dt, c2);
        VB.x = murb_hermite_predict_v(VB.x, az, jz, dt, c2);
    }
    if (s0 + 1 < a.count) {
        const float ax = a.a0[s0 + 1], ay = a.a0[n + s0 + 1], az = a.a0[2u * n + s0 + 1];
        const float jx = a.j0[s0 + 1], jy = a.j0[n + s0 + 1], jz = a.j0[2u * n + s0 + 1];
        A.y = murb_hermite_predict_q(A.y, VA.y, ax, jx, dt, c2, c3);
        A.w = murb_hermite_predict_q(A.w, VA.w, ay, jy, dt, c2, c3);
        B.y = murb_hermite_predict_q(B.y, VB.y, az, jz, dt, c2, c3);
        VA.y = murb_hermite_predict_v(VA.y, ax, jx, dt, c2);
        VA.w = murb_hermite_predict_v(VA.w, ay, jy, dt, c2);
        VB.y = murb_hermite_predict_v(VB.y, az, jz, dt, c2);
    }
    a.rec_out[ra] = A; a.rec_out[ra + MURB_TILE_PAIRS] = B;
    a.vel_out[ra] = VA; a.vel_out[ra + MURB_TILE_PAIRS] = VB;
}

__global__ __launch_bounds__(256) void murb_hermite_predict_kernel(const MurbHermiteArgs a)
{
    const int lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * lp >= (int)a.stride) return;
    murb_hermite_predict_pair(a, lp, a.dt);
}

// The two evaluations a corrector thread holds for its two slots: [slot][component]
struct MurbHermiteForces {
    float a0[2][3], j0[2][3], a1[2][3], j1[2][3];
    unsigned int nn_r2[2], nn_idx[2];   // "nearest": (r2 bits, slot) of the evaluation that gave (a1, j1); "contact": (key of gap2, slot)
};

// Partial rows -> (a1, j1) in fixed order; (a0, j0) are read, then replaced by (a1, j1).
__device__ __forceinline__ void murb_hermite_sum_rows(const MurbHermiteArgs& a, const int s0, MurbHermiteForces& f)
{
#pragma clang fp contract(off)
    const unsigned int n = a.stride;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int k = 0; k < 3; ++k) { f.a1[h][k] = 0.f; f.j1[h][k] = 0.f; }
    f.nn_r2[0] = f.nn_r2[1] = a.contact ? MURB_CT_NONE_KEY : MURB_F32_INF_BITS;
    f.nn_idx[0] = f.nn_idx[1] = MURB_NN_NONE;
    float ph[2] = {0.f, 0.f};
    for (int p = 0; p < a.nparts; ++p) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 u = a.part_a[(unsigned long)p * n + s0 + h];
            const float4 w = a.part_j[(unsigned long)p * n + s0 + h];
            f.a1[h][0] += u.x; f.a1[h][1] += u.y; f.a1[h][2] += u.z;
            f.j1[h][0] += w.x; f.j1[h][1] += w.y; f.j1[h][2] += w.z;
            if (a.phi) ph[h] += u.w;
            murb_nn_fold_row(f.nn_r2[h], f.nn_idx[h], u, w);
        }
    }
    if (a.phi) { a.phi[s0] = ph[0]; a.phi[s0 + 1] = ph[1]; }
    if (a.nn_idx) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (a.contact) murb_ct_store(a.nn_idx, a.nn_r2, s0 + h, f.nn_r2[h], f.nn_idx[h]);
            else murb_nn_store(a.nn_idx, a.nn_r2, s0 + h, f.nn_r2[h], f.nn_idx[h]);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned int at = (unsigned int)k * n + s0 + h;
            f.a0[h][k] = a.a0[at]; f.j0[h][k] = a.j0[at];
            a.a0[at] = f.a1[h][k]; a.j0[at] = f.j1[h][k];
            a.acc_out[at] = f.a1[h][k];
        }
}

// The state update of the pair of slots from both evaluations.
__device__ __forceinline__ void murb_hermite_correct_pair(const MurbHermiteArgs& a, const int lp, const MurbHermiteForces& f,
                                                          const float dt32)
{
#pragma clang fp contract(off)
    const int s0 = 2 * lp;
    const unsigned long ra = murb_rec_a((unsigned long)lp);
    float4 A = a.rec_in[ra], B = a.rec_in[ra + MURB_TILE_PAIRS];
    float4 VA = a.vel[ra], VB = a.vel[ra + MURB_TILE_PAIRS];
    const double dt = (double)dt32, h2 = dt * 0.5, c12 = dt * dt / 12.0;
    if (s0 < a.count) {
        const float vx = murb_hermite_correct_v(VA.x, f.a0[0][0], f.a1[0][0], f.j0[0][0], f.j1[0][0], h2, c12);
        const float vy = murb_hermite_correct_v(VA.z, f.a0[0][1], f.a1[0][1], f.j0[0][1], f.j1[0][1], h2, c12);
        const float vz = murb_hermite_correct_v(VB.x, f.a0[0][2], f.a1[0][2], f.j0[0][2], f.j1[0][2], h2, c12);
        A.x = murb_hermite_correct_q(A.x, VA.x, vx, f.a0[0][0], f.a1[0][0], h2, c12);
        A.z = murb_hermite_correct_q(A.z, VA.z, vy, f.a0[0][1], f.a1[0][1], h2, c12);
        B.x = murb_hermite_correct_q(B.x, VB.x, vz, f.a0[0][2], f.a1[0][2], h2, c12);
        VA.x = vx; VA.z = vy; VB.x = vz;
    }
    if (s0 + 1 < a.count) {
        const float vx = murb_hermite_correct_v(VA.y, f.a0[1][0], f.a1[1][0], f.j0[1][0], f.j1[1][0], h2, c12);
        const float vy = murb_hermite_correct_v(VA.w, f.a0[1][1], f.a1[1][1], f.j0[1][1], f.j1[1][1], h2, c12);
        const float vz = murb_hermite_correct_v(VB.y, f.a0[1][2], f.a1[1][2], f.j0[1][2], f.j1[1][2], h2, c12);
        A.y = murb_hermite_correct_q(A.y, VA.y, vx, f.a0[1][0], f.a1[1][0], h2, c12);
        A.w = murb_hermite_correct_q(A.w, VA.w, vy, f.a0[1][1], f.a1[1][1], h2, c12);
        B.y = murb_hermite_correct_q(B.y, VB.y, vz, f.a0[1][2], f.a1[1][2], h2, c12);
        VA.y = vx; VA.w = vy; VB.y = vz;
    }
    a.rec_out[ra] = A; a.rec_out[ra + MURB_TILE_PAIRS] = B;
    a.vel[ra] = VA; a.vel[ra + MURB_TILE_PAIRS] = VB;
}

// Partial rows -> (a1, j1) in fixed order -> state; (a0, j0) <- (a1, j1).
__global__ __launch_bounds__(256) void murb_hermite_correct_kernel(const MurbHermiteArgs a)
{
    const int lp = blockIdx.x * blockDim.x + threadIdx.x;
    const int s0 = 2 * lp;
    if (s0 >= (int)a.stride) return;
    MurbHermiteForces f;
    murb_hermite_sum_rows(a, s0, f);
    if (!a.update_state) return;
    murb_hermite_correct_pair(a, lp, f, a.dt);
}

// ---- shared adaptive time step (murbhip_evolve) ------------------------------------------------------------------------
// All bodies take one step size, which the device chooses; the host enqueues whole batches of steps without reading
// anything back.  Step size, clock and the "finished" decision therefore live in a control block in device memory:
//     predictor, sweep and corrector of an adaptive step read dt and the done flag from it (wave-uniform loads);
//     the corrector also evaluates the step criterion below for its bodies and folds the minimum into `cand`;
//     a one-thread bookkeeping launch behind every corrector advances the clock, records the step and chooses the next.
// Launches of one stream run in order, so a launch sees what the launches enqueued before it wrote: nothing here is
// concurrent except the corrector's workgroups among themselves, which meet in one atomicMin each — a minimum does not
// depend on the order of its operands, so the result is deterministic.  Once `done` is set the rest of a batch does
// nothing: the sweep returns before it touches LDS, the predictor returns, the corrector only copies the records through
// to the other position buffer (the host flips its buffer index once per enqueued step, whatever the device decided).
//
// Criterion (Makino & Aarseth 1992, with Aarseth's form of the step), per real body (slot < count, massless ones included):
//     a2 = (-6 (a0 - a1) - dt (4 j0 + 2 j1)) / dt^2     a3 = (12 (a0 - a1) + 6 dt (j0 + j1)) / dt^3     a2 += dt a3
//     dt_i = sqrt( eta (|a1| |a2| + |j1|^2) / (|j1| |a3| + |a2|^2) )
// in fp64 without contraction, in exactly the order written in murb_evolve_body_step (|x|^2 is the sum of squares
// (x.x + y.y) + z.z, |x| its square root); a dt_i that is not a finite positive number counts as +inf.  The candidate is
// min_i dt_i rounded to fp32 — rounding is monotonic, so the minimum of the rounded values is the rounded minimum — and
// positive floats order like their bit patterns, which is what the atomicMin compares.
#define MURB_EVOLVE_RING 4096

struct MurbEvolveCtl {
    double t;                       // model time advanced in this call
    double duration;
    double eta;
    unsigned long long steps, max_steps;
    float dt;                       // the step in flight (what predictor and corrector of the next enqueued step use)
    unsigned int cand;              // running minimum of the criterion over the bodies, as the bits of a positive float
    float raw;                      // the unclamped proposal the step in flight was taken from / for the next step
    float prop;                     // ... clamped to [dt_lo, dt_hi]
    float dt_lo, dt_hi;
    float used_min, used_max;       // smallest and largest step taken in this call
    int done;                       // duration reached or max_steps taken: every later launch of the batch is a no-op
    int last;                       // the step in flight ends at `duration` exactly
    unsigned int enc_hits;          // bodies of the step just taken with r2 <= enc_thr ("nearest"): non-zero ends the run
    float enc_thr;                  // radius^2 + soft^2, or -1: no encounter stop
    float ring[MURB_EVOLVE_RING];   // ring[k % MURB_EVOLVE_RING] = step k of this call
};

__device__ __forceinline__ double murb_sumsq3(const double x, const double y, const double z)
{
#pragma clang fp contract(off)
    return (x * x + y * y) + z * z;
}

__device__ __forceinline__ float murb_positive_or_inf(const double d)
{
    return (d > 0.0 && d < __builtin_inf()) ? (float)d : __builtin_inff();   // a NaN fails both comparisons
}

// dt_i of one body from both evaluations of the step of size dt
__device__ __forceinline__ float murb_evolve_body_step(const float (&a0)[3], const float (&j0)[3], const float (&a1)[3],
                                                       const float (&j1)[3], const double dt, const double eta)
{
#pragma clang fp contract(off)
    const double dt2 = dt * dt, dt3 = dt2 * dt;
    double a2[3], a3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double d = (double)a0[k] - (double)a1[k];
        a2[k] = ((-6.0 * d) - dt * ((4.0 * (double)j0[k]) + (2.0 * (double)j1[k]))) / dt2;
        a3[k] = ((12.0 * d) + (6.0 * dt) * ((double)j0[k] + (double)j1[k])) / dt3;
        a2[k] = a2[k] + dt * a3[k];
    }
    const double s_a1 = murb_sumsq3(a1[0], a1[1], a1[2]), s_j1 = murb_sumsq3(j1[0], j1[1], j1[2]);
    const double s_a2 = murb_sumsq3(a2[0], a2[1], a2[2]), s_a3 = murb_sumsq3(a3[0], a3[1], a3[2]);
    const double num = eta * (__builtin_sqrt(s_a1) * __builtin_sqrt(s_a2) + s_j1);
    const double den = __builtin_sqrt(s_j1) * __builtin_sqrt(s_a3) + s_a2;
    return murb_positive_or_inf(__builtin_sqrt(num / den));
}

// the first step of a call that finds no proposal: eta_start |a0| / |j0|
__device__ __forceinline__ float murb_evolve_body_first_step(const float ax, const float ay, const float az,
                                                             const float jx, const float jy, const float jz, const double eta_start)
{
#pragma clang fp contract(off)
    return murb_positive_or_inf(eta_start * (__builtin_sqrt(murb_sumsq3(ax, ay, az)) / __builtin_sqrt(murb_sumsq3(jx, jy, jz))));
}

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

// ... then over the workgroup of 256 through LDS, and one atomicMin per workgroup (issued by one lane: a vector atomic)
__device__ __forceinline__ void murb_evolve_fold_min(MurbEvolveCtl* ctl, const float mine)
{
    __shared__ unsigned int wave_min[4];
    const unsigned int m = murb_wave_min_bits(mine);
    if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int lo = wave_min[0] < wave_min[1] ? wave_min[0] : wave_min[1];
        const unsigned int hi = wave_min[2] < wave_min[3] ? wave_min[2] : wave_min[3];
        atomicMin(&ctl->cand, lo < hi ? lo : hi);
    }
}

// The step in flight from the unclamped proposal at the clock: clamp, and end exactly at `duration`.
__device__ __forceinline__ void murb_evolve_choose(MurbEvolveCtl* c)
{
    float dt = fmaxf(fminf(c->raw, c->dt_hi), c->dt_lo);
    c->prop = dt;
    const double rest = c->duration - c->t;
    const int last = (double)dt >= rest;
    if (last) dt = (float)rest;
    c->dt = dt;
    c->last = last;
}

// Head of a call, one thread.  fresh: no proposal is retained for the remembered (a0, j0) — murb_evolve_first_kernel and
// murb_evolve_start_kernel follow; otherwise `raw` is the previous adaptive step's and the first step is chosen here.
__global__ void murb_evolve_begin_kernel(MurbEvolveCtl* c, const double duration, const double eta, const float dt_lo,
                                         const float dt_hi, const unsigned long long max_steps, const int fresh,
                                         const float enc_thr)
{
    c->enc_hits = 0u;
    c->enc_thr = enc_thr;
    c->t = 0.0;
    c->duration = duration;
    c->eta = eta;
    c->steps = 0;
    c->max_steps = max_steps;
    c->dt_lo = dt_lo;
    c->dt_hi = dt_hi;
    c->used_min = __builtin_inff();
    c->used_max = 0.f;
    c->done = 0;
    c->cand = MURB_F32_INF_BITS;
    if (!fresh) murb_evolve_choose(c);
}

// min_i eta_start |a0| / |j0| over the real bodies into `cand`; one thread per pair of slots, like the corrector
__global__ __launch_bounds__(256) void murb_evolve_first_kernel(const MurbHermiteArgs a, MurbEvolveCtl* ctl, const double eta_start)
{
    const int s0 = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    const unsigned int n = a.stride;
    float mine = __builtin_inff();
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (s0 + h < a.count)
            mine = fminf(mine, murb_evolve_body_first_step(a.a0[s0 + h], a.a0[n + s0 + h], a.a0[2u * n + s0 + h],
                                                           a.j0[s0 + h], a.j0[n + s0 + h], a.j0[2u * n + s0 + h], eta_start));
    murb_evolve_fold_min(ctl, mine);
}

__global__ void murb_evolve_start_kernel(MurbEvolveCtl* c)
{
    c->raw = __builtin_bit_cast(float, c->cand);
    c->cand = MURB_F32_INF_BITS;
    murb_evolve_choose(c);
}

// Behind every adaptive corrector, one thread: the step in flight has been taken.
__global__ void murb_evolve_book_kernel(MurbEvolveCtl* c)
{
#pragma clang fp contract(off)
    if (c->done) return;
    const float dt = c->dt;
    const int was_last = c->last;
    c->ring[c->steps % MURB_EVOLVE_RING] = dt;
    c->steps += 1;
    c->t = was_last ? c->duration : c->t + (double)dt;
    c->used_min = fminf(c->used_min, dt);
    c->used_max = fmaxf(c->used_max, dt);
    c->raw = __builtin_bit_cast(float, c->cand);
    c->cand = MURB_F32_INF_BITS;
    murb_evolve_choose(c);
    if (was_last || c->steps >= c->max_steps || c->enc_hits) c->done = 1;
}

__global__ __launch_bounds__(256) void murb_hermite_predict_adaptive_kernel(const MurbHermiteArgs a, const MurbEvolveCtl* ctl)
{
    if (ctl->done) return;
    const int lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * lp >= (int)a.stride) return;
    murb_hermite_predict_pair(a, lp, ctl->dt);
}

template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) void murb_force_jerk_adaptive_kernel(const MurbJerkArgs a, const MurbEvolveCtl* ctl)
{
    if (ctl->done) return;   // one wave-uniform load, before anything else
    murb_force_jerk_sweep<R, WAVES, STAGE>(a);
}

// The nearest-neighbour form of both launches (ctl null: the fixed-step one).  104+ vector registers: 4 waves per SIMD.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_nn_sweep_kernel(const MurbNNJerkArgs a, const MurbEvolveCtl* ctl)
{
    if (ctl && ctl->done) return;   // wave-uniform
    murb_force_jerk_sweep<R, WAVES, STAGE, 1, MurbNNJerkArgs>(a);
}

// The contact form of both launches (ctl null: the fixed-step one); 4 waves per SIMD like the nearest-neighbour form.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_contact_sweep_kernel(const MurbNNJerkArgs a, const MurbEvolveCtl* ctl)
{
    if (ctl && ctl->done) return;   // wave-uniform
    murb_force_jerk_sweep<R, WAVES, STAGE, 2, MurbNNJerkArgs>(a);
}

// The potential form of both launches (ctl null: the fixed-step one).  R more packed accumulators: 4 waves per SIMD.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_force_jerk_pot_kernel(const MurbNNJerkArgs a, const MurbEvolveCtl* ctl)
{
    if (ctl && ctl->done) return;   // wave-uniform
    murb_force_jerk_sweep<R, WAVES, STAGE, 3, MurbNNJerkArgs>(a);
}

// The corrector of an adaptive step: murb_hermite_correct_kernel's work with dt from the control block, then the criterion.
// The grid covers the slots exactly or overshoots (threads past `stride` only take part in the fold).
__global__ __launch_bounds__(256) void murb_hermite_correct_adaptive_kernel(const MurbHermiteArgs a, MurbEvolveCtl* ctl)
{
    const int lp = blockIdx.x * blockDim.x + threadIdx.x;
    const int s0 = 2 * lp;
    const bool live = s0 < (int)a.stride;
    if (ctl->done) {   // wave-uniform: the state moves to the other buffer unchanged, (a0, j0) stay
        if (live) {
            const unsigned long ra = murb_rec_a((unsigned long)lp);
            a.rec_out[ra] = a.rec_in[ra];
            a.rec_out[ra + MURB_TILE_PAIRS] = a.rec_in[ra + MURB_TILE_PAIRS];
        }
        return;
    }
    float mine = __builtin_inff();
    if (live) {
        const float dt = ctl->dt;
        const double eta = ctl->eta;
        MurbHermiteForces f;
        murb_hermite_sum_rows(a, s0, f);
        murb_hermite_correct_pair(a, lp, f, dt);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (s0 + h < a.count) mine = fminf(mine, murb_evolve_body_step(f.a0[h], f.j0[h], f.a1[h], f.j1[h], (double)dt, eta));
        if (a.contact == 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (s0 + h < a.count) murb_ct_test(&ctl->enc_hits, a.enc, s0 + h, f.nn_r2[h], f.nn_idx[h]);
        } else if (a.nn_idx && !a.contact) {
            const float thr = ctl->enc_thr;
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (s0 + h < a.count) murb_enc_test(&ctl->enc_hits, a.enc, thr, s0 + h, f.nn_r2[h], f.nn_idx[h]);
        }
    }
    murb_evolve_fold_min(ctl, mine);
}

// ---- individual block time steps (murbhip_evolve_block) --------------------------------------------------------------------
// Every body has its own step dt_max 2^-k (its level k in [0, kmax]) and its own time, counted in ticks of dt_max 2^-kmax
// inside the block of dt_max in flight (T = 2^kmax ticks; include/murbhip.h spells the scheme out).  A block step advances
// only the bodies whose next time is the earliest one — the active set — and sweeps those few i bodies against ALL bodies
// predicted to that time.  The host never learns how many they are: the set's size, the shape of the sweep made from it and
// the end of the run live in a control block, like murbhip_evolve's, and every launch has a size fixed by the host.
//     1  murb_block_min_kernel       t_next = min_i (t_i + (T >> k_i))                      (one atomicMin per workgroup)
//     2  murb_block_predict_kernel   every body -> herm_rec / herm_vel at t_next; the active ones also get a place in the
//                                    list (atomicAdd) and their predicted q, v in a compact buffer of the same pair layout
//     3  murb_block_plan_kernel      one thread: groups of 16 list entries, j chunks, row stride
//     4  murb_force_jerk_block_kernel  workgroups walk (group, chunk) units; rows part[chunk * stride + list index]
//     5  murb_block_correct_kernel   one thread per list entry: row sum in chunk order, corrector in place, criterion, level
//     6  murb_block_book_kernel      one thread: clock, counters, done, reset of t_next and the list length
// All on one stream.  Concurrent writers meet only in integer atomics (a minimum, a maximum, a count, a list position): a
// body's place in the list varies from run to run, its numbers do not — its sums depend on the j order and the chunk cut
// alone, and the cut on the SIZE of the list.
#define MURB_BLOCK_GROUP 16   // list entries per workgroup of the sweep (4 waves x 4 i bodies)

struct MurbBlockCtl {
    double tick_sec;                 // (double)dt_max * 2^-kmax: seconds = (double)ticks * tick_sec, exact for kmax <= 20
    double eta;
    unsigned long long ticks_done;   // model time advanced in this call, in ticks
    unsigned long long steps, max_steps, body_steps;
    float dt_max;
    int kmax;
    unsigned int T;                  // ticks per block, 2^kmax
    unsigned int clock;              // time of the last block step inside the block in flight, [0, T); 0 = synchronised
    unsigned int blocks_left;
    unsigned int t_next;             // step in flight: its time (running minimum of launch 1; ~0u between steps)
    unsigned int n_act;              // ... length of the active list
    int groups, chunks;              // ... the sweep's units
    unsigned int stride;             // ... entries per partial row, 16 * groups
    int units, tiles;                // "block_units", layout tiles swept as j
    unsigned int row_cap;            // entries a partial-row buffer holds
    unsigned int clamped;            // steps whose criterion asked for less than dt_max 2^-kmax
    unsigned int max_act;
    unsigned int k_lo, k_hi;         // smallest and largest level a step of this call was taken at
    int done;
    // the i side and the rows of the active sweep, which reads them here once per unit instead of holding four more pointers
    // in scalar registers through its inner loop
    const float4* rec_act;
    const float4* vel_act;
    float4* part_a;
    float4* part_j;
    // "nearest"
    const int* list;                 // the active list, where the nearest-neighbour sweep finds its i bodies' slots
    unsigned int enc_hits;           // active bodies of the step just taken with r2 <= enc_thr: non-zero ends the run
    float enc_thr;                   // radius^2 + soft^2, or -1: no encounter stop
};

struct MurbBlockArgs {
    float4* rec;           // current positions + GM: the corrector updates active bodies in place
    float4* vel;
    float4* rec_pred;      // every body predicted to t_next (herm_rec / herm_vel): the j side of the sweep
    float4* vel_pred;
    float4* rec_act;       // predicted q, v of the active bodies by list index, pair layout: the i side
    float4* vel_act;
    float* a0;             // remembered evaluation of every body at its own time
    float* j0;
    float* acc_out;
    float4* part_a;        // partial rows
    float4* part_j;
    unsigned int* ticks;   // t_i
    int* levels;           // k_i
    int* list;             // active bodies, unordered
    int* nn_idx;           // "nearest": every body's nearest neighbour and its r2 at its own time; null = off
    float* nn_r2;
    MurbEncList* enc;
    int count;
    unsigned int stride;   // slots
    float soft2;
    int contact;           // "contact": see MurbHermiteArgs
    float* phi;            // "potential": every body's potential at its own time; null = off
};

// what the active sweep holds of it through its inner loop
struct MurbBlockSweepArgs {
    const float4* rec_pred;
    const float4* vel_pred;
    float soft2;
};

struct MurbBlockNNSweepArgs : MurbBlockSweepArgs {
    int count;                  // real bodies: slots >= count are padding
    int grid;                   // workgroups of the launch
    const MurbBlockCtl* ctl;    // the control block once more: the sweep reads both here, once per unit (murb_kernarg_again)
};

// dt_max 2^-k: exact while the result is a normal number
__device__ __forceinline__ float murb_block_dt(const float dt_max, const int k)
{
    return dt_max * __builtin_bit_cast(float, (unsigned int)(127 - k) << 23);
}

// smallest k in [0, kmax] with dt_max 2^-k <= req (+inf: 0); none: kmax, and the step counts as clamped
__device__ __forceinline__ int murb_block_level_of(const float req, const float dt_max, const int kmax, bool& clamped)
{
    clamped = false;
    for (int k = 0; k <= kmax; ++k)
        if (murb_block_dt(dt_max, k) <= req) return k;
    clamped = true;
    return kmax;
}

// the level after a step that ended at t_next: any number of halvings, one doubling where the coarser grid has a point
__device__ __forceinline__ int murb_block_new_level(const int k, const int k_req, const unsigned int t_next, const unsigned int T)
{
    if (k_req > k) return k_req;
    if (k_req < k && t_next % (2u * (T >> k)) == 0u) return k - 1;
    return k;
}

// one float of a body's place in the pair layout: c = 0, 1, 2 for x, y, z
__device__ __forceinline__ float* murb_block_slot(float4* recs, const unsigned int slot, const int c)
{
    float* const base = (float*)(recs + murb_rec_a((unsigned long)(slot >> 1)) + (c == 2 ? MURB_TILE_PAIRS : 0));
    return base + (c == 1 ? 2 : 0) + (slot & 1u);
}

// Head of a call, one thread.  `resume`: a block is open, the clock and the bodies' ticks and levels go on.
__global__ void murb_block_begin_kernel(MurbBlockCtl* c, const MurbBlockArgs a, const float dt_max, const int kmax, const double eta, const unsigned int blocks,
                                        const unsigned long long max_steps, const int units, const int tiles,
                                        const unsigned int row_cap, const int resume, const float enc_thr)
{
    c->list = a.list;
    c->enc_hits = 0u;
    c->enc_thr = enc_thr;
    c->tick_sec = (double)dt_max * (double)murb_block_dt(1.f, kmax);
    c->eta = eta;
    c->ticks_done = 0;
    c->steps = 0;
    c->max_steps = max_steps;
    c->body_steps = 0;
    c->dt_max = dt_max;
    c->kmax = kmax;
    c->T = 1u << kmax;
    if (!resume) c->clock = 0u;
    c->blocks_left = blocks;
    c->t_next = ~0u;
    c->n_act = 0u;
    c->groups = 0; c->chunks = 1; c->stride = 0u;
    c->units = units;
    c->tiles = tiles;
    c->row_cap = row_cap;
    c->clamped = 0u;
    c->max_act = 0u;
    c->k_lo = ~0u;
    c->k_hi = 0u;
    c->done = 0;
    c->rec_act = a.rec_act;
    c->vel_act = a.vel_act;
    c->part_a = a.part_a;
    c->part_j = a.part_j;
}

// Starting levels from the remembered evaluation: the level of eta_start |a0| / |j0|; all bodies at tick 0.
__global__ __launch_bounds__(256) void murb_block_start_kernel(const MurbBlockArgs a, const MurbBlockCtl* ctl, const double eta_start)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.count) return;
    const unsigned int n = a.stride;
    const float req = murb_evolve_body_first_step(a.a0[s], a.a0[n + s], a.a0[2u * n + s], a.j0[s], a.j0[n + s], a.j0[2u * n + s], eta_start);
    bool clamped;
    a.levels[s] = murb_block_level_of(req, ctl->dt_max, ctl->kmax, clamped);
    a.ticks[s] = 0u;
}

// launch 1
__global__ __launch_bounds__(256) void murb_block_min_kernel(const MurbBlockArgs a, MurbBlockCtl* ctl)
{
    if (ctl->done) return;
    __shared__ unsigned int wave_min[4];
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int mine = ~0u;
    if (s < a.count) mine = a.ticks[s] + (ctl->T >> a.levels[s]);
    const unsigned int m = murb_wave_min_bits(__builtin_bit_cast(float, mine));   // an unsigned minimum of the bits, whatever they mean
    if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int lo = wave_min[0] < wave_min[1] ? wave_min[0] : wave_min[1];
        const unsigned int hi = wave_min[2] < wave_min[3] ? wave_min[2] : wave_min[3];
        atomicMin(&ctl->t_next, lo < hi ? lo : hi);
    }
}

// launch 2: one thread per pair of slots, like murb_hermite_predict_pair, but every body with its own dt = t_next - t_i
__global__ __launch_bounds__(256) void murb_block_predict_kernel(const MurbBlockArgs a, MurbBlockCtl* ctl)
{
#pragma clang fp contract(off)
    if (ctl->done) return;
    const int lp = blockIdx.x * blockDim.x + threadIdx.x;
    const int s0 = 2 * lp;
    const unsigned int n = a.stride;
    if (s0 >= (int)n) return;
    const unsigned long ra = murb_rec_a((unsigned long)lp);
    const float4 A = a.rec[ra], B = a.rec[ra + MURB_TILE_PAIRS];
    const float4 VA = a.vel[ra], VB = a.vel[ra + MURB_TILE_PAIRS];
    float q[2][3] = {{A.x, A.z, B.x}, {A.y, A.w, B.y}}, v[2][3] = {{VA.x, VA.z, VB.x}, {VA.y, VA.w, VB.y}};
    const unsigned int t_next = ctl->t_next, T = ctl->T;
    const double tick = ctl->tick_sec;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = s0 + h;
        if (s >= a.count) continue;
        const unsigned int t = a.ticks[s];
        const double dt = (double)(t_next - t) * tick, c2 = dt * dt * 0.5, c3 = dt * dt * dt / 6.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float ak = a.a0[(unsigned int)k * n + s], jk = a.j0[(unsigned int)k * n + s];
            const float qk = q[h][k], vk = v[h][k];
            q[h][k] = murb_hermite_predict_q(qk, vk, ak, jk, dt, c2, c3);
            v[h][k] = murb_hermite_predict_v(vk, ak, jk, dt, c2);
        }
        if (t + (T >> a.levels[s]) == t_next) {
            const unsigned int at = atomicAdd(&ctl->n_act, 1u);   // at < count <= slots
            a.list[at] = s;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                *murb_block_slot(a.rec_act, at, k) = q[h][k];
                *murb_block_slot(a.vel_act, at, k) = v[h][k];
            }
            if (a.contact) murb_block_slot(a.vel_act, at, 2)[2] = h ? VB.w : VB.z;   // the radius: the active sweep's i side reads it there
        }
    }
    a.rec_pred[ra] = make_float4(q[0][0], q[1][0], q[0][1], q[1][1]);
    a.rec_pred[ra + MURB_TILE_PAIRS] = make_float4(q[0][2], q[1][2], B.z, B.w);
    a.vel_pred[ra] = make_float4(v[0][0], v[1][0], v[0][1], v[1][1]);
    a.vel_pred[ra + MURB_TILE_PAIRS] = make_float4(v[0][2], v[1][2], VB.z, VB.w);
}

// launch 3, one thread: `units` (group, chunk) units at least, where the layout has the tiles for it
__global__ void murb_block_plan_kernel(MurbBlockCtl* c)
{
    if (c->done) return;
    const int groups = (int)((c->n_act + MURB_BLOCK_GROUP - 1) / MURB_BLOCK_GROUP);
    int chunks = groups > 0 ? (c->units + groups - 1) / groups : 1;
    chunks = chunks < 1 ? 1 : (chunks > c->tiles ? c->tiles : chunks);
    while (chunks > 1 && (unsigned long)groups * chunks * MURB_BLOCK_GROUP > c->row_cap) --chunks;   // never taken: the host sizes the rows
    c->groups = groups;
    c->chunks = chunks;
    c->stride = (unsigned int)groups * MURB_BLOCK_GROUP;
}

// The control block as the sweep reads it once per unit.  No launch writes it while the sweep runs, so the loads may go
// through the scalar cache (constant address space) like the `done` test of every launch here; the empty asm makes the
// pointer a new value to the compiler in every iteration, so that it does not move the loads in front of the loop and hold
// their results in scalar registers through the inner loop, where the i bodies need them.
typedef const __attribute__((address_space(4))) MurbBlockCtl* MurbBlockCtlK;
typedef const __attribute__((address_space(4))) float4* MurbF4K;
__device__ __forceinline__ MurbBlockCtlK murb_block_ctl_now(const MurbBlockCtl* ctl)
{
    unsigned long p = (unsigned long)ctl;
    asm volatile("" : "+s"(p));
    return (MurbBlockCtlK)p;
}

// launch 4.  murb_force_jerk_sweep's mapping and inner loop; the i bodies come from the compact buffer, and the workgroup
// walks units u = blockIdx.x, += gridDim.x with (group, chunk) = (u % groups, u / groups).  The entries behind the list's
// end in its last group are whatever the buffer held: their rows are never read.
// The body is a device function with the nearest-neighbour form behind a compile-time switch (NN, Args =
// MurbBlockNNSweepArgs; MODE 1), the contact form (MODE 2) and the potential form (MODE 3), like murb_force_jerk_sweep: the plain
// form's code does not change.
template <int R, int WAVES, int STAGE, int MODE = 0, typename Args = MurbBlockSweepArgs>
__device__ __forceinline__ void murb_force_jerk_block_sweep(const Args a, const MurbBlockCtl* ctl)  // NN: a is the kernel's first argument
{
    constexpr bool NN = MODE != 0, CT = MODE == 2, POT = MODE == 3;   // as in murb_force_jerk_sweep
    static_assert(R % 2 == 0 && WAVES * R == MURB_BLOCK_GROUP, "a workgroup takes one group of the list");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
#if defined(__HIP_DEVICE_COMPILE__)   // the host pass knows no constant address space to read through
    if (ctl->done) return;   // one wave-uniform load, before anything else
    __shared__ float4 lds[2 * STAGE * MURB_TILE_F4];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float soft2 = a.soft2;

    int stride_u = 0;
    for (int u = blockIdx.x;; u += NN ? stride_u : (int)gridDim.x) {
        if constexpr (NN) {   // the scalar registers are taken: the stride and the control block from the kernel arguments, per unit
            const auto* again = murb_kernarg_again<Args>();
            if constexpr (!CT) stride_u = again->grid;   // the contact form reads it at the unit's end: one scalar register less
            ctl = again->ctl;
        }
        const MurbBlockCtlK now = murb_block_ctl_now(ctl);
        const int groups = now->groups, chunks = now->chunks, tiles = now->tiles;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        int wave_now = wave;
        if constexpr (NN) {   // made in every unit, like the fold's lane below: the scalar registers are taken
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            wave_now = __builtin_amdgcn_readfirstlane(tid >> 6);
        }
        const int i_slot = (group * WAVES + wave_now) * R;   // list index, wave-uniform

        float xi[R], yi[R], zi[R], ui[R], vi[R], wi[R], ri[R];   // ri: the contact form's radii
        {
            const unsigned long ra = murb_rec_a((unsigned long)(i_slot >> 1));
            // written by the launch before this one and wave-uniform: scalar loads, straight into scalar registers
            const MurbF4K rec_act = (MurbF4K)(unsigned long)now->rec_act, vel_act = (MurbF4K)(unsigned long)now->vel_act;
#pragma unroll
            for (int h = 0; h < R / 2; ++h) {
                const float4 A = rec_act[ra + h], B = rec_act[ra + h + MURB_TILE_PAIRS];
                const float4 VA = vel_act[ra + h], VB = vel_act[ra + h + MURB_TILE_PAIRS];
                xi[2 * h] = A.x; xi[2 * h + 1] = A.y; yi[2 * h] = A.z; yi[2 * h + 1] = A.w; zi[2 * h] = B.x; zi[2 * h + 1] = B.y;
                ui[2 * h] = VA.x; ui[2 * h + 1] = VA.y; vi[2 * h] = VA.z; vi[2 * h + 1] = VA.w; wi[2 * h] = VB.x; wi[2 * h + 1] = VB.y;
                if constexpr (CT) {   // to vector registers: no scalar one is free
                    ri[2 * h] = VB.z; ri[2 * h + 1] = VB.w;
                    asm volatile("" : "+v"(ri[2 * h]), "+v"(ri[2 * h + 1]));
                }
            }
        }
        float mn[R];   // NN: the lane's smallest r2 per i body, and the lane step it fell at
        int st[R];
        // NN: the i bodies' slots in lanes 0 .. R - 1 of ONE vector register and the body count in lane R, read out lane by lane
        // where they are needed: the scalar registers are taken (an entry behind the list's end is a slot of an earlier step or 0,
        // its row is never read)
        int who = 0;
        if constexpr (NN) {
            int l = threadIdx.x & 63;
            asm volatile("" : "+v"(l));
            const int slot = ((const int*)now->list)[i_slot + (l & (R - 1))];
            who = l < R ? slot : murb_kernarg_again<Args>()->count;   // `a` is the kernel's first argument
#pragma unroll
            for (int r = 0; r < R; ++r) { mn[r] = __builtin_inff(); st[r] = 0; }
        }

        const int vt0 = (int)(((long)tiles * chunk) / chunks);
        const int vt1 = (int)(((long)tiles * (chunk + 1)) / chunks);

        murb_f2 ax[R], ay[R], az[R], jx[R], jy[R], jz[R], ph[R];   // ph: POT, the sums of GM_j * inv
        {
            float z = 0.f;   // made in every iteration, like the fold's below
            asm volatile("" : "+v"(z));
#pragma unroll
            for (int r = 0; r < R; ++r) {
                ax[r] = (murb_f2)(z); ay[r] = (murb_f2)(z); az[r] = (murb_f2)(z);
                jx[r] = (murb_f2)(z); jy[r] = (murb_f2)(z); jz[r] = (murb_f2)(z);
                if constexpr (POT) ph[r] = (murb_f2)(z);
            }
        }

        for (int vs = vt0; vs < vt1; vs += STAGE) {
            const int nt = (vt1 - vs) < STAGE ? (vt1 - vs) : STAGE;
            __syncthreads();   // previous stage (of this unit or the one before) fully consumed
            // The thread's index as a new value in every stage (the empty asm hides that it never changes): the copy's and the
            // reads' addresses are then made from it here instead of four of them being held through the inner loop from
            // in front of the unit loop, and the sweep fits the 96 vector registers of murb_force_jerk_sweep.
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const int lane = tid & 63;
            for (int t = 0; t < nt; ++t) {
                const float4* srcq = a.rec_pred + (unsigned long)(vs + t) * MURB_TILE_F4;
                const float4* srcv = a.vel_pred + (unsigned long)(vs + t) * MURB_TILE_F4;
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
                if constexpr (NN) {
                    int w = who, self_tile[R];
                    asm volatile("" : "+v"(w));   // read out here, in every tile
#pragma unroll
                    for (int r = 0; r < R; ++r) self_tile[r] = __builtin_amdgcn_readlane(w, r) / MURB_TILE_BODIES;
                    if constexpr (POT) {   // the wave's R bodies can lie in R different tiles
                        murb_pot_tile<R, R>(tq, tv, lane, vs + t, self_tile, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, ph);
                        continue;
                    }
                    const bool masked = murb_nn_tile_masked<R>(vs + t, self_tile, __builtin_amdgcn_readlane(w, R));   // wave-uniform
                    if constexpr (CT) murb_ct_tile<R>(tq, tv, lane, vs + t, masked, xi, yi, zi, ui, vi, wi, ri, soft2, ax, ay, az, jx, jy, jz, mn, st);
                    else murb_nn_tile<R>(tq, tv, lane, vs + t, masked, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, mn, st);
                    continue;
                }
#pragma unroll
                for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
                    const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
                    const float4 VA = tv[q + lane], VB = tv[q + lane + MURB_TILE_PAIRS];
                    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
                    const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y};
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        murb_interact_jerk_pk(xj, yj, zj, gj, uj, vj, wj, xi[r], yi[r], zi[r], ui[r], vi[r], wi[r], soft2,
                                              ax[r], ay[r], az[r], jx[r], jy[r], jz[r]);
                }
            }
        }

        // The fold's zero and lane tests are made here, in every iteration (the empty asm hides that they never change): moved
        // in front of the unit loop they would hold a vector register and ten scalar ones through the inner loop.
        float zero = 0.f;
        int fold_lane = threadIdx.x & 63;
        asm volatile("" : "+v"(zero), "+v"(fold_lane));
        float oa[3] = {zero, zero, zero}, oj[3] = {zero, zero, zero};
        float nn_a = zero, nn_j = zero;   // the rows' fourth floats
        if constexpr (NN) {
            int w = who, self[R], self_tile[R];
            const float4* rec_pred = a.rec_pred;
            asm volatile("" : "+v"(w), "+s"(rec_pred));   // no address made from the pointer in front of the unit loop
#pragma unroll
            for (int r = 0; r < R; ++r) { self[r] = __builtin_amdgcn_readlane(w, r); self_tile[r] = self[r] / MURB_TILE_BODIES; }
            const int count = __builtin_amdgcn_readlane(w, R);
            unsigned int nn_r2 = 0u, nn_idx = 0u;
            if constexpr (POT) {
                for (int tile = vt0; tile < vt1; ++tile)
                    if (murb_pot_tile_own<R>(tile, self_tile)) murb_pot_own_tile<R, true>(rec_pred, fold_lane, tile, xi, yi, zi, soft2, ph, self);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float sp = murb_wave_sum(ph[r].x + ph[r].y);
                    if (fold_lane == r) nn_r2 = __builtin_bit_cast(unsigned int, sp);   // part_j.w stays 0
                }
            } else if constexpr (CT) {
                const float4* vel_pred = a.vel_pred;
                asm volatile("" : "+s"(vel_pred));
                for (int tile = vt0; tile < vt1; ++tile)
                    if (murb_nn_tile_masked<R>(tile, self_tile, count))
                        murb_ct_masked_tile<R>(rec_pred, vel_pred, fold_lane, tile, xi, yi, zi, ri, soft2, mn, st, self, count);
                murb_ct_finish<R>(rec_pred, vel_pred, fold_lane, xi, yi, zi, ri, soft2, mn, st, self, count, nn_r2, nn_idx);
            } else {
                for (int tile = vt0; tile < vt1; ++tile)
                    if (murb_nn_tile_masked<R>(tile, self_tile, count))
                        murb_nn_masked_tile<R>(rec_pred, fold_lane, tile, xi, yi, zi, soft2, mn, st, self, count);
                murb_nn_finish<R>(rec_pred, fold_lane, xi, yi, zi, soft2, mn, st, self, count, nn_r2, nn_idx);
            }
            nn_a = __builtin_bit_cast(float, nn_r2);
            nn_j = __builtin_bit_cast(float, nn_idx);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float sx = murb_wave_sum(ax[r].x + ax[r].y), sy = murb_wave_sum(ay[r].x + ay[r].y), sz = murb_wave_sum(az[r].x + az[r].y);
            const float tx = murb_wave_sum(jx[r].x + jx[r].y), ty = murb_wave_sum(jy[r].x + jy[r].y), tz = murb_wave_sum(jz[r].x + jz[r].y);
            if (fold_lane == r) { oa[0] = sx; oa[1] = sy; oa[2] = sz; oj[0] = tx; oj[1] = ty; oj[2] = tz; }
        }
        if (fold_lane < R) {
            const MurbBlockCtlK end = murb_block_ctl_now(ctl);
            const unsigned long at = (unsigned long)chunk * end->stride + (unsigned long)i_slot + fold_lane;   // < groups * chunks * 16 <= row_cap
            end->part_a[at] = make_float4(oa[0], oa[1], oa[2], nn_a);
            end->part_j[at] = make_float4(oj[0], oj[1], oj[2], nn_j);
        }
        if constexpr (CT) stride_u = murb_kernarg_again<Args>()->grid;
    }
#else
    (void)a; (void)ctl; (void)NN; (void)CT; (void)POT;
#endif
}

template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(5))) void murb_force_jerk_block_kernel(const MurbBlockSweepArgs a, const MurbBlockCtl* ctl)
{
    murb_force_jerk_block_sweep<R, WAVES, STAGE>(a, ctl);
}

// The nearest-neighbour form.  104+ vector registers: 4 waves per SIMD, so the host launches 4 workgroups per CU.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_nn_active_sweep_kernel(const MurbBlockNNSweepArgs a, const MurbBlockCtl* ctl)
{
    murb_force_jerk_block_sweep<R, WAVES, STAGE, 1, MurbBlockNNSweepArgs>(a, ctl);
}

// The contact form: the i bodies' radii come from the compact velocity buffer, where the block predictor puts them.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_contact_active_sweep_kernel(const MurbBlockNNSweepArgs a, const MurbBlockCtl* ctl)
{
    murb_force_jerk_block_sweep<R, WAVES, STAGE, 2, MurbBlockNNSweepArgs>(a, ctl);
}

// The potential form: the i bodies' slots come from the list, like the nearest-neighbour form's.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_force_jerk_pot_block_kernel(const MurbBlockNNSweepArgs a, const MurbBlockCtl* ctl)
{
    murb_force_jerk_block_sweep<R, WAVES, STAGE, 3, MurbBlockNNSweepArgs>(a, ctl);
}

// launch 5: one thread per list entry.  The grid covers `count` entries; threads behind the list's end only take part in the
// wave folds.
__global__ __launch_bounds__(256) void murb_block_correct_kernel(const MurbBlockArgs a, MurbBlockCtl* ctl)
{
#pragma clang fp contract(off)
    if (ctl->done) return;
    const unsigned int at = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned int n_act = ctl->n_act;
    if ((at & ~63u) >= n_act) return;   // the whole wave is behind the list's end
    const bool live = at < n_act;
    unsigned int k_used = ~0u, k_used_inv = ~0u;
    bool clamped = false;
    if (live) {
        const unsigned int n = a.stride, stride = ctl->stride, t_next = ctl->t_next, T = ctl->T;
        const int chunks = ctl->chunks, kmax = ctl->kmax;
        const float dt_max = ctl->dt_max;
        const int s = a.list[at];
        const int k = a.levels[s];
        float a0[3], j0[3], a1[3] = {0.f, 0.f, 0.f}, j1[3] = {0.f, 0.f, 0.f};
        unsigned int nn_r2 = a.contact ? MURB_CT_NONE_KEY : MURB_F32_INF_BITS, nn_idx = MURB_NN_NONE;
        float ph = 0.f;
        for (int p = 0; p < chunks; ++p) {
            const float4 u = a.part_a[(unsigned long)p * stride + at];
            const float4 w = a.part_j[(unsigned long)p * stride + at];
            a1[0] += u.x; a1[1] += u.y; a1[2] += u.z;
            j1[0] += w.x; j1[1] += w.y; j1[2] += w.z;
            if (a.phi) ph += u.w;
            murb_nn_fold_row(nn_r2, nn_idx, u, w);
        }
        if (a.phi) a.phi[s] = ph;
        if (a.contact) {
            murb_ct_store(a.nn_idx, a.nn_r2, s, nn_r2, nn_idx);
            if (a.contact == 2) murb_ct_test(&ctl->enc_hits, a.enc, s, nn_r2, nn_idx);
        } else if (a.nn_idx) {
            murb_nn_store(a.nn_idx, a.nn_r2, s, nn_r2, nn_idx);
            murb_enc_test(&ctl->enc_hits, a.enc, ctl->enc_thr, s, nn_r2, nn_idx);
        }
        const float dt32 = murb_block_dt(dt_max, k);
        const double dt = (double)dt32, h2 = dt * 0.5, c12 = dt * dt / 12.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned int pl = (unsigned int)c * n + s;
            a0[c] = a.a0[pl]; j0[c] = a.j0[pl];
            a.a0[pl] = a1[c]; a.j0[pl] = j1[c]; a.acc_out[pl] = a1[c];
            float* const qp = murb_block_slot(a.rec, (unsigned int)s, c);
            float* const vp = murb_block_slot(a.vel, (unsigned int)s, c);
            const float v0 = *vp;
            const float v1 = murb_hermite_correct_v(v0, a0[c], a1[c], j0[c], j1[c], h2, c12);
            *qp = murb_hermite_correct_q(*qp, v0, v1, a0[c], a1[c], h2, c12);
            *vp = v1;
        }
        const float req = murb_evolve_body_step(a0, j0, a1, j1, dt, ctl->eta);
        const int k_req = murb_block_level_of(req, dt_max, kmax, clamped);
        a.levels[s] = murb_block_new_level(k, k_req, t_next, T);
        a.ticks[s] = t_next == T ? 0u : t_next;
        k_used = (unsigned int)k;
        k_used_inv = (unsigned int)(kmax - k);
    }
    const unsigned int lo = murb_wave_min_bits(__builtin_bit_cast(float, k_used));
    const unsigned int hi_inv = murb_wave_min_bits(__builtin_bit_cast(float, k_used_inv));
    const unsigned int nclamped = (unsigned int)__builtin_popcountll(__ballot(clamped));
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&ctl->k_lo, lo);
        atomicMax(&ctl->k_hi, (unsigned int)ctl->kmax - hi_inv);
        if (nclamped) atomicAdd(&ctl->clamped, nclamped);
    }
}

// murbhip_potential_energy: -1/2 m_i phi_i per real body in fp64, block sums in murb_metrics_kernel's fixed order (wave shuffle
// tree, then the 4 waves through LDS); the host adds the block rows in index order.  One block = 256 consecutive slots.
__global__ __launch_bounds__(256) void murb_potential_sum_kernel(const float* mass, const float* phi, double* out, const int count)
{
#pragma clang fp contract(off)
    __shared__ double red[3];
    const int s = blockIdx.x * 256 + threadIdx.x;
    double v = s < count ? -0.5 * (double)mass[s] * (double)phi[s] : 0.0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0 && wave > 0) red[wave - 1] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((v + red[0]) + red[1]) + red[2];
}

// The radii in the velocity records ("contact"): lanes z, w of a pair's B record = {R0, R1}; radius null: 0 in both (option
// off, or no radii set yet), as in the padding slots.  One thread per pair of slots.
__global__ __launch_bounds__(256) void murb_radii_lanes_kernel(float4* vel, const float* radius, const int count, const unsigned int slots)
{
    const unsigned int lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (2u * lp >= slots) return;
    const int s0 = (int)(2u * lp);
    float* const b = (float*)(vel + murb_rec_a((unsigned long)lp) + MURB_TILE_PAIRS);
    b[2] = radius && s0 < count ? radius[s0] : 0.f;
    b[3] = radius && s0 + 1 < count ? radius[s0 + 1] : 0.f;
}

// launch 6, one thread: the step in flight has been taken
__global__ void murb_block_book_kernel(MurbBlockCtl* c)
{
    if (c->done) return;
    const unsigned int t_next = c->t_next, n_act = c->n_act;
    c->ticks_done += (unsigned long long)(t_next - c->clock);
    c->steps += 1;
    c->body_steps += n_act;
    c->max_act = n_act > c->max_act ? n_act : c->max_act;
    if (t_next == c->T) {
        c->clock = 0u;
        c->blocks_left -= 1u;
    } else {
        c->clock = t_next;
    }
    c->t_next = ~0u;
    c->n_act = 0u;
    if (c->blocks_left == 0u || c->steps >= c->max_steps || c->enc_hits) c->done = 1;
}

// ---- field at arbitrary points (murbfield_at / murbfield_of; include/murbfield.h has the definition) --------------------
// The rectangular sweep as a read-out: `count` points with velocities of the caller's against ALL bodies at their current
// state; per point acceleration, jerk and potential, with one body slot per point left out (its "skip" entry, or none).
//     1  murb_field_pack_kernel    the uploaded SoA points, or the listed bodies' own q and v gathered from the records, into
//                                  one pair of records per point: {x, y, z, skip} {u, v, w, 0}; the last group of 16 is filled
//                                  up with copies of its first point (their rows are never read)
//     2  murb_force_field_kernel   workgroups walk (group of 16 points, j chunk) units over a fixed grid; rows part[chunk * stride + point]
//     3  murb_field_rows_kernel    one thread per point: the rows added in chunk order, SoA results in the caller's order
// The skipped slot must not enter an fp32 sum at all (DESIGN.md §4.11 gave the reason for phi; a point need not sit on the
// body it skips, so here it holds for a and j too).  Testing the slot per pair would cost every pair.  Instead the tile that
// holds a point's skipped slot runs the loop's arithmetic with G m_j times a multiplier that is 0 for THAT point alone
// (wave-uniform, per point: one packed multiply per pair of interactions, where the potential sweeps spend their fma with pm)
// and adds nothing, and behind the loop that tile's 512 slots are swept once more for that point from the records in memory
// with the skipped slot's G m replaced by 0 through a select.  So every point's sums receive "the chunk's other tiles in layout
// order, then the tile of its skipped slot", whoever shares its wave, its group, its launch or its call: the bits of a point's
// results depend on its own inputs, the bodies and the chunk count (murb_field.h) alone.
struct MurbFieldArgs {
    const float4* rec;      // current positions + GM, all slots
    const float4* vel;      // current velocities (with "contact" on their B records carry radii in lanes z, w: never read)
    const float4* pts;      // two records per point
    float4* part_a;         // part_a[chunk * stride + point] = {ax, ay, az, phi}
    float4* part_j;         // ... {jx, jy, jz, 0}
    int groups, chunks;     // the launch's units
    int tiles;              // layout tiles swept as j (those that hold real bodies)
    unsigned int stride;    // entries per partial row: 16 * groups
    float soft2;
};

struct MurbFieldPackArgs {
    const float* in;        // murbfield_at: px | py | pz | pvx | pvy | pvz, in_stride floats each; null: murbfield_of
    const int* idx;         // murbfield_at: the skip entries, or null (none); murbfield_of: the bodies
    const float4* rec;      // murbfield_of: where the bodies' q and v are read
    const float4* vel;
    float4* pts;
    int count;              // points of the launch
    int padded;             // ... rounded up to whole groups
    unsigned int in_stride;
    int has_vel;            // murbfield_at: 0 = points at rest
};

__global__ __launch_bounds__(256) void murb_field_pack_kernel(const MurbFieldPackArgs a)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= a.padded) return;
    const int src = p < a.count ? p : p / MURB_FIELD_GROUP * MURB_FIELD_GROUP;   // the group's first point: < count
    float x, y, z, u = 0.f, v = 0.f, w = 0.f;
    int skip = -1;
    if (a.in) {
        x = a.in[src]; y = a.in[a.in_stride + src]; z = a.in[2 * a.in_stride + src];
        if (a.has_vel) { u = a.in[3 * a.in_stride + src]; v = a.in[4 * a.in_stride + src]; w = a.in[5 * a.in_stride + src]; }
        if (a.idx) skip = a.idx[src];
    } else {
        skip = a.idx[src];
        const unsigned long ra = murb_rec_a((unsigned long)(skip >> 1));
        const float* const q = (const float*)(a.rec + ra) + (skip & 1);
        const float* const qv = (const float*)(a.vel + ra) + (skip & 1);
        x = q[0]; y = q[2]; z = q[4 * MURB_TILE_PAIRS];
        u = qv[0]; v = qv[2]; w = qv[4 * MURB_TILE_PAIRS];
    }
    a.pts[2 * p] = make_float4(x, y, z, __builtin_bit_cast(float, skip));
    a.pts[2 * p + 1] = make_float4(u, v, w, 0.f);
}

// One point against the tile of its skipped slot, from the records in memory: the loop's packed arithmetic, the slot's G m
// replaced by 0.  Lane steps rising, like the loop's.
__device__ __forceinline__ void murb_field_skip_tile(const float4* rec, const float4* vel, const int lane, const int skip,
                                                     const float xi, const float yi, const float zi,
                                                     const float ui, const float vi, const float wi, const float soft2,
                                                     murb_f2& ax, murb_f2& ay, murb_f2& az, murb_f2& jx, murb_f2& jy, murb_f2& jz, murb_f2& ph)
{
    const int tile = skip / MURB_TILE_BODIES;
#pragma unroll 1
    for (int qs = 0; qs < MURB_TILE_PAIRS / 64; ++qs) {
        const unsigned long ra = (unsigned long)tile * MURB_TILE_F4 + qs * 64 + lane;
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
        const float4 VA = vel[ra], VB = vel[ra + MURB_TILE_PAIRS];
        const int j0 = tile * MURB_TILE_BODIES + 2 * (qs * 64 + lane);
        const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y};
        const murb_f2 gj = {j0 == skip ? 0.f : B.z, j0 + 1 == skip ? 0.f : B.w};
        const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y};
        murb_f2 r2, gi;
        murb_interact_jerk_pk_gi(xj, yj, zj, gj, uj, vj, wj, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, r2, gi);
        ph += gi;
    }
}

// launch 2.  murb_force_jerk_block_sweep's mapping: a workgroup takes a group of 16 points, 4 per wave, their values
// wave-uniform, and walks units u = blockIdx.x, += gridDim.x with (group, chunk) = (u % groups, u / groups): neighbouring
// workgroups sweep the same j tiles.  128 vector registers at most: 4 waves per SIMD, the grid of the potential forms.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_force_field_kernel(const MurbFieldArgs a)
{
    static_assert(R % 2 == 0 && WAVES * R == MURB_FIELD_GROUP, "a workgroup takes one group of points");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
    __shared__ float4 lds[2 * STAGE * MURB_TILE_F4];
    const float soft2 = a.soft2;

    // Through the inner loop the scalar registers hold the points' 24 values, the four multipliers and the two record
    // pointers.  Everything else of the kernel's argument is read again where it is needed (murb_kernarg_again), and the
    // points' skip entries wait in lanes 0 .. R - 1 of one vector register (`who`), like the active sweep's slots.
    for (int u = blockIdx.x;; u += (int)gridDim.x) {
        const auto* now = murb_kernarg_again<MurbFieldArgs>();
        const int groups = now->groups, chunks = now->chunks, tiles = now->tiles;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63;
        const int i_first = (group * WAVES + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;   // point of the launch, wave-uniform

        float xi[R], yi[R], zi[R], ui[R], vi[R], wi[R];
        int who;   // lane r: the skip entry of point r (-1: none)
        {
            const float4* const pts = now->pts;
            who = __builtin_bit_cast(int, pts[2 * (i_first + (lane & (R - 1)))].w);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 P = pts[2 * (i_first + r)], V = pts[2 * (i_first + r) + 1];
                xi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.x)));
                yi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.y)));
                zi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.z)));
                ui[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, V.x)));
                vi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, V.y)));
                wi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, V.z)));
            }
        }

        const int vt0 = (int)(((long)tiles * chunk) / chunks);
        const int vt1 = (int)(((long)tiles * (chunk + 1)) / chunks);

        murb_f2 ax[R], ay[R], az[R], jx[R], jy[R], jz[R], ph[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ax[r] = (murb_f2)(0.f); ay[r] = (murb_f2)(0.f); az[r] = (murb_f2)(0.f);
            jx[r] = (murb_f2)(0.f); jy[r] = (murb_f2)(0.f); jz[r] = (murb_f2)(0.f);
            ph[r] = (murb_f2)(0.f);
        }

        for (int vs = vt0; vs < vt1; vs += STAGE) {
            const int nt = (vt1 - vs) < STAGE ? (vt1 - vs) : STAGE;
            __syncthreads();   // previous stage (of this unit or the one before) fully consumed
            for (int t = 0; t < nt; ++t) {
                const float4* srcq = a.rec + (unsigned long)(vs + t) * MURB_TILE_F4;
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
                float pm[R];   // wave-uniform, per point: 0 in the tile of the point's OWN skipped slot alone
                {
                    int w = who;
                    asm volatile("" : "+v"(w));   // read out here, in every tile
#pragma unroll
                    for (int r = 0; r < R; ++r) pm[r] = (__builtin_amdgcn_readlane(w, r) >> 9) == vs + t ? 0.f : 1.f;   // -1 >> 9 = -1: no tile
                    static_assert(MURB_TILE_BODIES == 1 << 9, "a slot's tile is slot >> 9");
                }
#pragma unroll
                for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
                    const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
                    const float4 VA = tv[q + lane], VB = tv[q + lane + MURB_TILE_PAIRS];
                    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
                    const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y};
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        murb_f2 r2, gi;
                        murb_interact_jerk_pk_gi(xj, yj, zj, gj * pm[r], uj, vj, wj, xi[r], yi[r], zi[r], ui[r], vi[r], wi[r], soft2,
                                                 ax[r], ay[r], az[r], jx[r], jy[r], jz[r], r2, gi);
                        ph[r] += gi;
                    }
                }
            }
        }

        // the tile of every point's skipped slot, for that point alone (wave-uniform branches)
        {
            const auto* again = murb_kernarg_again<MurbFieldArgs>();
            const float4* const rec = again->rec;
            const float4* const vel = again->vel;
            int w = who;
            asm volatile("" : "+v"(w));
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int skip = __builtin_amdgcn_readlane(w, r), skip_tile = skip >> 9;
                if (skip_tile >= vt0 && skip_tile < vt1)
                    murb_field_skip_tile(rec, vel, lane, skip, xi[r], yi[r], zi[r], ui[r], vi[r], wi[r], soft2,
                                         ax[r], ay[r], az[r], jx[r], jy[r], jz[r], ph[r]);
            }
        }

        // fold the 64 lanes x 2 halves of every accumulator; lane r keeps point r's totals
        float oa[4] = {0.f, 0.f, 0.f, 0.f}, oj[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float sx = murb_wave_sum(ax[r].x + ax[r].y), sy = murb_wave_sum(ay[r].x + ay[r].y), sz = murb_wave_sum(az[r].x + az[r].y);
            const float tx = murb_wave_sum(jx[r].x + jx[r].y), ty = murb_wave_sum(jy[r].x + jy[r].y), tz = murb_wave_sum(jz[r].x + jz[r].y);
            const float sp = murb_wave_sum(ph[r].x + ph[r].y);
            if (lane == r) { oa[0] = sx; oa[1] = sy; oa[2] = sz; oa[3] = sp; oj[0] = tx; oj[1] = ty; oj[2] = tz; }
        }
        if (lane < R) {
            const auto* end = murb_kernarg_again<MurbFieldArgs>();
            const unsigned long at = (unsigned long)chunk * end->stride + (unsigned long)i_first + lane;   // < chunks * 16 * groups
            end->part_a[at] = make_float4(oa[0], oa[1], oa[2], oa[3]);
            end->part_j[at] = make_float4(oj[0], oj[1], oj[2], 0.f);
        }
    }
}

// launch 3: one thread per point of the launch.  fp32, chunks in ascending order.  out: ax | ay | az | jx | jy | jz | phi,
// out_stride floats each; a null plane pointer is not possible here: the host copies out what the caller asked for.
__global__ __launch_bounds__(256) void murb_field_rows_kernel(const float4* part_a, const float4* part_j, float* out, const int count,
                                                              const int chunks, const unsigned int stride, const unsigned int out_stride)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= count) return;
    float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < chunks; ++c) {
        const float4 u = part_a[(unsigned long)c * stride + p];
        const float4 w = part_j[(unsigned long)c * stride + p];
        s[0] += u.x; s[1] += u.y; s[2] += u.z;
        s[3] += w.x; s[4] += w.y; s[5] += w.z;
        s[6] += u.w;
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) out[(unsigned long)k * out_stride + p] = s[k];
}

#endif
