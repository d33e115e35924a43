// gfx950 (CDNA4) kernels of the minimum-spanning-tree read-out (murbforeign_of / murbmst_of).  Device code only; included by
// murb_ctx.h.
#ifndef MURB_KERNELS_MST_H_
#define MURB_KERNELS_MST_H_

#include "murb_field.h"
#include "murb_kernels_side.h"

// ---- nearest body of another label (include/murbmst.h has the definition) ----------------------------------------------------
// The neighbour sweeps' walk (murb_kernels_nbr.h) with a label compared per pair and a lexicographic minimum in the place of
// the count: `count` listed bodies against ALL bodies at their current positions, per point the smallest (r2, index) over the
// bodies whose label is >= 0 and not the point's own.
//     0  murb_mst_label_kernel     a copy of the position + G m records in which the two G m lanes of each B record carry the
//                                  two bodies' label BITS, and every slot that must never win (a body with label < 0, a padding
//                                  slot) carries x = +inf: its r2 is fma(inf, inf, soft2) = +inf whatever the point, which is
//                                  never strictly below a running minimum that starts at +inf.  (+inf and not NaN: the sum stays
//                                  an ordered number through the three-operand minimum, and the step behind the loop may compare
//                                  it with ==.)  The sweep reads the copy, so `index < n`, the mask and the body itself cost
//                                  the loop nothing: the body drops out by its own label
//     1  murb_foreign_pack_kernel  the listed bodies' own q gathered from the records, with their label bits: {x, y, z, label},
//                                  the first of a point's two records; the last group of 16 is filled up with copies of its
//                                  first point (murb_field_pack_kernel's rule; their rows are never read)
//     2  murb_foreign_sweep_kernel the walk over (group of 16 points, j chunk) units on the fixed grid; per unit and point one
//                                  (r2 bits, index): part[chunk * stride + point]
//     3  murb_foreign_rows_kernel  one thread per point: the chunks' entries folded in chunk order
// The labels are integers in float lanes.  They move through memory, LDS and registers as bits and meet integer compares
// alone: no float operation touches them (small integers are denormals and would be flushed).
// The running minimum is kept the way murb_bind_step keeps it: every lane keeps, per point, the minimum of the r2 it has formed
// (one three-operand minimum per pair of interactions) and the lane step S = 4 * tile + q / 64 at which it last fell (a compare
// and a select).  Slots rise with S in a lane and the select takes a strictly smaller value only, so S is the EARLIEST step
// that holds the lane's minimum.  Behind the loop the lane forms that one step's two r2 again from the labelled copy in memory,
// through the same inline function, label select included: the lower slot of the pair may tie in r2 and carry the point's own
// label.  The first of the two that holds the minimum is the lowest slot.  The wave then folds (r2 bits, slot)
// lexicographically; r2 >= 0, so the bits order as unsigned integers.
#define MURB_FOREIGN_NONE 0x7fffffffu   // "no candidate" in the rows (the public index is -1)

// launch 0: one thread per record of the tiles that hold real bodies.
__global__ __launch_bounds__(256) void murb_mst_label_kernel(const float4* rec, const int* label, float4* out, const int count,
                                                             const unsigned int records)
{
    const unsigned int r = blockIdx.x * 256u + threadIdx.x;
    if (r >= records) return;
    float4 v = rec[r];
    const unsigned int tile = r / MURB_TILE_F4, within = r % MURB_TILE_F4;
    const bool b_rec = within >= MURB_TILE_PAIRS;
    const int j0 = (int)(2u * (tile * MURB_TILE_PAIRS + (b_rec ? within - MURB_TILE_PAIRS : within)));
    const int l0 = j0 < count ? label[j0] : -1;
    const int l1 = j0 + 1 < count ? label[j0 + 1] : -1;
    if (b_rec) {   // {z0, z1, G m0, G m1}: the labels' bits in the place of G m
        v.z = __builtin_bit_cast(float, l0);
        v.w = __builtin_bit_cast(float, l1);
    } else {       // {x0, x1, y0, y1}: a slot that must never win sits at x = +inf
        if (l0 < 0) v.x = __builtin_inff();
        if (l1 < 0) v.y = __builtin_inff();
    }
    out[r] = v;
}

// launch 1: one thread per point of the launch, whole groups.
__global__ __launch_bounds__(256) void murb_foreign_pack_kernel(const float4* rec, const int* label, const int* bodies, float4* pts,
                                                                const int count, const int padded)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= padded) return;
    const int src = p < count ? p : p / MURB_FIELD_GROUP * MURB_FIELD_GROUP;   // the group's first point: < count
    const int body = bodies[src];
    const unsigned long ra = murb_rec_a((unsigned long)(body >> 1));
    const float* const q = (const float*)(rec + ra) + (body & 1);
    pts[2 * p] = make_float4(q[0], q[2], q[4 * MURB_TILE_PAIRS], __builtin_bit_cast(float, label[body]));
    pts[2 * p + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

struct MurbForeignArgs {
    const float4* rec;      // the labelled copy of the records (murb_mst_label_kernel): the tiles that hold real bodies
    const float4* pts;      // two records per point (murb_foreign_pack_kernel); the first is read
    uint2* part;            // part[chunk * stride + point] = {r2 bits, index}
    int groups, chunks;     // the launch's units
    int tiles_each, tiles_more; // the j cut: every chunk takes tiles_each layout tiles, the first tiles_more chunks one more
    unsigned int stride;    // points per chunk row: 16 * groups
    float soft2;
};

// r2 of one point and two j bodies, packed, with the label select: 3 packed subtractions and 3 packed fmas, then per half one
// integer compare of the slot's label with the point's and a select of +inf.  The loop and the step behind it share this one
// function.
__device__ __forceinline__ murb_f2 murb_foreign_r2_pk(const float4 A, const float4 B, const float xi, const float yi, const float zi,
                                                      const int label, const float soft2)
{
    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y};
    const murb_f2 dx = xj - xi, dy = yj - yi, dz = zj - zi;
    murb_f2 r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
    r2 = __builtin_elementwise_fma(dy, dy, r2);
    r2 = __builtin_elementwise_fma(dz, dz, r2);
    r2.x = __builtin_bit_cast(int, B.z) == label ? __builtin_inff() : r2.x;
    r2.y = __builtin_bit_cast(int, B.w) == label ? __builtin_inff() : r2.y;
    return r2;
}

// launch 2.  murb_nbr_sweep's frame: a workgroup takes a group of 16 points, 4 per wave, each point's x, y, z and label
// wave-uniform in scalar registers, and walks units u = blockIdx.x, += gridDim.x with (group, chunk) = (u % groups, u / groups).
// STAGE tiles of 8 KiB each in LDS: positions + labels.  With STAGE = 2 a workgroup holds 16 KiB and 4 workgroups share a CU,
// the 4 waves per SIMD the attribute asks for.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_foreign_sweep_kernel(const MurbForeignArgs a)
{
    static_assert(R % 2 == 0 && WAVES * R == MURB_FIELD_GROUP, "a workgroup takes one group of points");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
    static_assert(STAGE * MURB_TILE_F4 * sizeof(float4) * 4 <= 160 * 1024, "4 workgroups per CU share its LDS");
    __shared__ float4 lds[STAGE * MURB_TILE_F4];
    const float soft2 = a.soft2;

    // Through the loop the scalar registers hold the points' coordinates (a packed instruction reads a scalar as a pair: 6
    // registers a point), their labels and the compares' masks.  Of the kernel's argument only rec and soft2 stay, the rest is
    // read again once per unit (murb_kernarg_again), as murb_nbr_sweep does.
    for (int u = blockIdx.x;; u += (int)gridDim.x) {
        const auto* now = murb_kernarg_again<MurbForeignArgs>();   // `a` is the kernel's first argument
        const int groups = now->groups, chunks = now->chunks;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));   // made here, per unit: nothing derived from it is held in scalar registers across units
        const int lane = tid & 63;
        const int i_first = (group * WAVES + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;   // point of the launch, wave-uniform

        float xi[R], yi[R], zi[R], mn[R];   // the point's x, y, z and label: wave-uniform, in scalar registers
        int lab[R], st[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 P = now->pts[2 * (i_first + r)];
            xi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.x)));
            yi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.y)));
            zi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.z)));
            lab[r] = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.w));
            mn[r] = __builtin_inff();
            st[r] = 0;
        }

        // tiles_each * chunks + tiles_more = tiles (a minimum does not depend on the cut, so it need not be the field sweep's)
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
#pragma unroll
                for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
                    const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
                    const int S = (vs + t) * (MURB_TILE_PAIRS / 64) + q / 64;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const murb_f2 r2 = murb_foreign_r2_pk(A, B, xi[r], yi[r], zi[r], lab[r], soft2);
                        const float m = __builtin_fminf(__builtin_fminf(mn[r], r2.x), r2.y);
                        st[r] = m < mn[r] ? S : st[r];
                        mn[r] = m;
                    }
                }
            }
        }

        // the slot behind every lane's minimum, then the fold over the wave: (r2 bits, slot) of every point, wave-uniform
        uint2 out[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int p = st[r] * 64 + lane;   // the pair of slots of lane step st[r] (0 where nothing fell): inside the labelled copy
            const unsigned long ra = murb_rec_a((unsigned long)p);
            const murb_f2 r2 = murb_foreign_r2_pk(a.rec[ra], a.rec[ra + MURB_TILE_PAIRS], xi[r], yi[r], zi[r], lab[r], soft2);
            const unsigned int idx = mn[r] < __builtin_inff() ? (unsigned int)(r2.x == mn[r] ? 2 * p : 2 * p + 1) : MURB_FOREIGN_NONE;
            const unsigned int key = __builtin_bit_cast(unsigned int, mn[r]);
            out[r].x = murb_wave_min_bits(__builtin_bit_cast(float, key));   // an unsigned minimum of the bits
            out[r].y = murb_wave_min_bits(__builtin_bit_cast(float, key == out[r].x ? idx : MURB_FOREIGN_NONE));
        }
        if (lane == 0) {
            const auto* end = murb_kernarg_again<MurbForeignArgs>();
            uint2* const row = end->part + ((unsigned long)chunk * end->stride + (unsigned long)i_first);   // < chunks * 16 * groups
#pragma unroll
            for (int r = 0; r < R; ++r) row[r] = out[r];
        }
    }
}

// launch 3: one thread per point of the launch.  The chunks' (r2 bits, index) folded lexicographically in chunk order; -1 and
// +inf where there is no candidate and for a point whose own label is < 0.
__global__ __launch_bounds__(256) void murb_foreign_rows_kernel(const uint2* part, const float4* pts, int* out_idx, float* out_r2,
                                                                const int count, const int chunks, const unsigned int stride)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= count) return;
    unsigned int key = __builtin_bit_cast(unsigned int, __builtin_inff()), idx = MURB_FOREIGN_NONE;
    for (int c = 0; c < chunks; ++c) {
        const uint2 e = part[(unsigned long)c * stride + p];
        if (e.x < key || (e.x == key && e.y < idx)) { key = e.x; idx = e.y; }
    }
    if (__builtin_bit_cast(int, pts[2 * p].w) < 0) idx = MURB_FOREIGN_NONE;
    out_idx[p] = idx == MURB_FOREIGN_NONE ? -1 : (int)idx;
    out_r2[p] = idx == MURB_FOREIGN_NONE ? __builtin_inff() : __builtin_bit_cast(float, key);
}

#endif
