// gfx950 (CDNA4) kernels of the field read-out (murbfield_at / murbfield_of).  Device code only; included by murb_ctx.h.
#ifndef MURB_KERNELS_FIELD_H_
#define MURB_KERNELS_FIELD_H_

#include "murb_field.h"
#include "murb_kernels_side.h"

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
