// gfx950 (CDNA4) kernels of the listed-source read-out (murblist_of / murblist_at / murbsplit_of).  Device code only; included by
// murb_ctx.h.
#ifndef MURB_KERNELS_LIST_H_
#define MURB_KERNELS_LIST_H_

#include "murb_kernels_side.h"
#include "murb_list.h"

// ---- the field of listed bodies at arbitrary points (include/murblist.h has the definition) ---------------------------------
// Acceleration, jerk and potential at a point from an explicit list of source bodies: O(list length), not O(N).
//     1  murb_list_pack_kernel    a copy of the bodies for gathering, two records per body: {x, y, z, G m} {u, v, w, 0}, so that a
//                                 source costs two 16-byte loads from one 32-byte line (the layout records keep a body's seven
//                                 values in four places)
//     (murb_field_pack_kernel)    the points, as the field read-out packs them: {x, y, z, -} {u, v, w, 0}
//     2  murb_list_sweep_kernel   one wave per point; the lane of entry e is (e >> 1) & 63, its half e & 1, its lane step e >> 7
// No skip machinery, no chunks, no partial rows: a point's sums are formed by one wave from its own list in its own order.
struct MurbListPackArgs {
    const float4* rec;      // current positions + GM, all slots
    const float4* vel;      // current velocities
    float4* src;            // two records per body
    int count;              // real bodies
};

__global__ __launch_bounds__(256) void murb_list_pack_kernel(const MurbListPackArgs a)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= a.count) return;
    const unsigned long ra = murb_rec_a((unsigned long)(j >> 1));
    const float* const q = (const float*)(a.rec + ra) + (j & 1);
    const float* const qv = (const float*)(a.vel + ra) + (j & 1);
    a.src[2 * j] = make_float4(q[0], q[2], q[4 * MURB_TILE_PAIRS], q[4 * MURB_TILE_PAIRS + 2]);
    a.src[2 * j + 1] = make_float4(qv[0], qv[2], qv[4 * MURB_TILE_PAIRS], 0.f);
}

struct MurbListArgs {
    const float4* src;          // two records per body (murb_list_pack_kernel)
    const float4* pts;          // two records per point of the launch (murb_field_pack_kernel)
    const unsigned int* begin;  // per point: where its list starts in idx ...
    const unsigned int* len;    // ... and its length
    const int* idx;             // the staged entries: body indices in [0, n), checked or produced before the launch
    float* out;                 // ax | ay | az | jx | jy | jz | phi, out_stride floats each
    int count;                  // points of the launch
    unsigned int out_stride;
    float soft2;
};

// U lane steps of one point, from lane step `step` on: first all 2 U index loads, then all 4 U record gathers, then the
// arithmetic in ascending lane step.  A slot past the list's last entry re-reads the LAST entry (one address for all such lanes)
// with G m replaced by +0: its products are +-0 and leave every sum as it is.
template <int U>
__device__ __forceinline__ void murb_list_steps(const float4* __restrict__ src, const int* __restrict__ list, const int last, const int step,
                                                const int lane, const float xi, const float yi, const float zi, const float ui,
                                                const float vi, const float wi, const float soft2, murb_f2& ax, murb_f2& ay, murb_f2& az,
                                                murb_f2& jx, murb_f2& jy, murb_f2& jz, murb_f2& ph)
{
    int j0[U], j1[U];
    bool in0[U], in1[U];
#pragma unroll
    for (int s = 0; s < U; ++s) {
        const int e0 = (step + s) * MURB_LIST_STEP + 2 * lane, e1 = e0 + 1;
        in0[s] = e0 <= last;
        in1[s] = e1 <= last;
        j0[s] = list[in0[s] ? e0 : last];   // offsets may be odd: two dwords
        j1[s] = list[in1[s] ? e1 : last];
    }
    float4 P0[U], V0[U], P1[U], V1[U];
#pragma unroll
    for (int s = 0; s < U; ++s) {
        P0[s] = src[2 * (unsigned long)j0[s]]; V0[s] = src[2 * (unsigned long)j0[s] + 1];
        P1[s] = src[2 * (unsigned long)j1[s]]; V1[s] = src[2 * (unsigned long)j1[s] + 1];
    }
#pragma unroll
    for (int s = 0; s < U; ++s) {
        const murb_f2 xj = {P0[s].x, P1[s].x}, yj = {P0[s].y, P1[s].y}, zj = {P0[s].z, P1[s].z};
        const murb_f2 gj = {in0[s] ? P0[s].w : 0.f, in1[s] ? P1[s].w : 0.f};
        const murb_f2 uj = {V0[s].x, V1[s].x}, vj = {V0[s].y, V1[s].y}, wj = {V0[s].z, V1[s].z};
        murb_f2 r2, gi;
        murb_interact_jerk_pk_gi(xj, yj, zj, gj, uj, vj, wj, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, r2, gi);
        ph += gi;
    }
}

// launch 2.  A workgroup of WAVES waves takes WAVES consecutive points, a wave one point: its six values wave-uniform in scalar
// registers as in the field kernel, its list walked in lane steps of 128 entries, 4 lane steps of gathers in flight where the
// list is that long, then 2, then 1.  Lanes beyond a short list add +0.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void murb_list_sweep_kernel(const MurbListArgs a)
{
    int tid = threadIdx.x;
    const int lane = tid & 63;
    const int p = (int)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform
    if (p >= a.count) return;
    const int length = __builtin_amdgcn_readfirstlane((int)a.len[p]);
    if (length == 0) {   // an empty list: +0 seven times
        if (lane < 7) a.out[(unsigned long)lane * a.out_stride + p] = 0.f;
        return;
    }
    const int* const list = a.idx + __builtin_amdgcn_readfirstlane((int)a.begin[p]);
    const float4 P = a.pts[2 * p], V = a.pts[2 * p + 1];
    const float xi = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.x)));
    const float yi = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.y)));
    const float zi = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.z)));
    const float ui = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, V.x)));
    const float vi = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, V.y)));
    const float wi = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, V.z)));
    const float soft2 = a.soft2;
    const int last = length - 1, steps = murb_list_lane_steps((unsigned int)length);

    murb_f2 ax = (murb_f2)(0.f), ay = (murb_f2)(0.f), az = (murb_f2)(0.f);
    murb_f2 jx = (murb_f2)(0.f), jy = (murb_f2)(0.f), jz = (murb_f2)(0.f), ph = (murb_f2)(0.f);
    int step = 0;
#pragma unroll 1
    for (; step + 4 <= steps; step += 4)
        murb_list_steps<4>(a.src, list, last, step, lane, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, ph);
    if (step + 2 <= steps) {
        murb_list_steps<2>(a.src, list, last, step, lane, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, ph);
        step += 2;
    }
    if (step < steps)
        murb_list_steps<1>(a.src, list, last, step, lane, xi, yi, zi, ui, vi, wi, soft2, ax, ay, az, jx, jy, jz, ph);

    const float sx = murb_wave_sum(ax.x + ax.y), sy = murb_wave_sum(ay.x + ay.y), sz = murb_wave_sum(az.x + az.y);
    const float tx = murb_wave_sum(jx.x + jx.y), ty = murb_wave_sum(jy.x + jy.y), tz = murb_wave_sum(jz.x + jz.y);
    const float sp = murb_wave_sum(ph.x + ph.y);
    if (lane == 0) {
        float* const o = a.out + p;
        const unsigned long st = a.out_stride;
        o[0] = sx; o[st] = sy; o[2 * st] = sz; o[3 * st] = tx; o[4 * st] = ty; o[5 * st] = tz; o[6 * st] = sp;
    }
}

#endif
