// gfx950 (CDNA4) kernels of the tidal read-out (murbtidal_at / murbtidal_of).  Device code only; included by murb_ctx.h.
#ifndef MURB_KERNELS_TIDAL_H_
#define MURB_KERNELS_TIDAL_H_

#include "murb_field.h"
#include "murb_kernels_side.h"

// ---- tidal tensor at arbitrary points (murbtidal_at / murbtidal_of; include/murbtidal.h has the definition) -------------
// The field read-out's rectangular sweep (murb_kernels_field.h) with the gradient of the acceleration in the place of the
// field: `count` points against ALL bodies at their current positions, six sums per point, one body slot per point left out.
//     1  murb_field_pack_kernel    the field read-out's, as it is: {x, y, z, skip} is the first of a point's two records (the
//                                  second, the velocity, is packed and never read here)
//     2  murb_tidal_sweep_kernel   the field sweep's walk over (group of 16 points, j chunk) units on the same fixed grid; rows
//                                  part_a[chunk * stride + point] = {xx, yy, zz, xy}, part_b[...] = {xz, yz, 0, 0}
//     3  murb_tidal_rows_kernel    one thread per point: the rows added in chunk order, SoA results in the caller's order
// No velocities: a tile's position + GM records alone are staged in LDS, 8 KiB a tile where the field sweep stages 16.
// The skipped slot is the field sweep's: in the tile of a point's skipped slot G m_j is multiplied by 0 for THAT point alone,
// and behind the loop that tile is swept once more for that point from memory with the slot's G m replaced by 0.
struct MurbTidalArgs {
    const float4* rec;      // current positions + GM, all slots
    const float4* pts;      // two records per point (murb_field_pack_kernel); the first is read
    float4* part_a;         // part_a[chunk * stride + point] = {xx, yy, zz, xy}
    float4* part_b;         // ... {xz, yz, 0, 0}
    int groups, chunks;     // the launch's units
    int tiles;              // layout tiles swept as j (those that hold real bodies)
    unsigned int stride;    // entries per partial row: 16 * groups
    float soft2;
};

// One point against two j bodies (packed): the pair's term of T, formed per pair and then added (include/murbtidal.h has the
// sequence and the reason: the diagonal never meets a separate sum of s).
// 3 pk_add + 3 pk_fma (|d|^2 + soft^2) + 2 rsq + 10 pk_mul + 3 pk_fma + 3 (pk_fma + pk_add): 25 packed, 26 with the caller's mask
__device__ __forceinline__ void murb_tidal_pair_pk(const murb_f2 xj, const murb_f2 yj, const murb_f2 zj, const murb_f2 gj,
                                                   const float xi, const float yi, const float zi, const float soft2,
                                                   murb_f2& xx, murb_f2& yy, murb_f2& zz, murb_f2& xy, murb_f2& xz, murb_f2& yz)
{
    const murb_f2 dx = xj - xi, dy = yj - yi, dz = zj - zi;
    murb_f2 r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
    r2 = __builtin_elementwise_fma(dy, dy, r2);
    r2 = __builtin_elementwise_fma(dz, dz, r2);
    murb_f2 inv;
    inv.x = __builtin_amdgcn_rsqf(r2.x);
    inv.y = __builtin_amdgcn_rsqf(r2.y);
    const murb_f2 inv2 = inv * inv;
    const murb_f2 gi = gj * inv;
    const murb_f2 s = gi * inv2;             // GM_j * inv^3, never G*inv^3 alone (fp32 range)
    const murb_f2 s3 = s * 3.0f;
    const murb_f2 nx = dx * inv, ny = dy * inv, nz = dz * inv;   // |n| <= 1
    const murb_f2 tx = s3 * nx, ty = s3 * ny, tz = s3 * nz;
    xx += __builtin_elementwise_fma(tx, nx, -s);
    yy += __builtin_elementwise_fma(ty, ny, -s);
    zz += __builtin_elementwise_fma(tz, nz, -s);
    xy = __builtin_elementwise_fma(tx, ny, xy);
    xz = __builtin_elementwise_fma(tx, nz, xz);
    yz = __builtin_elementwise_fma(ty, nz, yz);
}

// One point against the tile of its skipped slot, from the records in memory: the loop's packed arithmetic, the slot's G m
// replaced by 0.  Lane steps rising, like the loop's.
__device__ __forceinline__ void murb_tidal_skip_tile(const float4* rec, const int lane, const int skip,
                                                     const float xi, const float yi, const float zi, const float soft2,
                                                     murb_f2& xx, murb_f2& yy, murb_f2& zz, murb_f2& xy, murb_f2& xz, murb_f2& yz)
{
    const int tile = skip / MURB_TILE_BODIES;
#pragma unroll 1
    for (int qs = 0; qs < MURB_TILE_PAIRS / 64; ++qs) {
        const unsigned long ra = (unsigned long)tile * MURB_TILE_F4 + qs * 64 + lane;
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
        const int j0 = tile * MURB_TILE_BODIES + 2 * (qs * 64 + lane);
        const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y};
        const murb_f2 gj = {j0 == skip ? 0.f : B.z, j0 + 1 == skip ? 0.f : B.w};
        murb_tidal_pair_pk(xj, yj, zj, gj, xi, yi, zi, soft2, xx, yy, zz, xy, xz, yz);
    }
}

// launch 2.  murb_force_field_kernel's mapping: a workgroup takes a group of 16 points, 4 per wave, their values
// wave-uniform, and walks units u = blockIdx.x, += gridDim.x with (group, chunk) = (u % groups, u / groups).  128 vector
// registers at most: 4 waves per SIMD, 4 workgroups per CU, the field sweep's grid; STAGE tiles of 8 KiB each in LDS.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_tidal_sweep_kernel(const MurbTidalArgs a)
{
    static_assert(R % 2 == 0 && WAVES * R == MURB_FIELD_GROUP, "a workgroup takes one group of points");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
    static_assert(STAGE * MURB_TILE_F4 * sizeof(float4) * 4 <= 160 * 1024, "4 workgroups per CU share its LDS");
    __shared__ float4 lds[STAGE * MURB_TILE_F4];
    const float soft2 = a.soft2;

    // Through the inner loop the scalar registers hold the points' 12 values, the four multipliers and the record pointer.
    // Everything else of the kernel's argument is read again where it is needed (murb_kernarg_again), and the points' skip
    // entries wait in lanes 0 .. R - 1 of one vector register (`who`), like the field sweep's.
    for (int u = blockIdx.x;; u += (int)gridDim.x) {
        const auto* now = murb_kernarg_again<MurbTidalArgs>();
        const int groups = now->groups, chunks = now->chunks, tiles = now->tiles;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63;
        const int i_first = (group * WAVES + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;   // point of the launch, wave-uniform

        float xi[R], yi[R], zi[R];
        int who;   // lane r: the skip entry of point r (-1: none)
        {
            const float4* const pts = now->pts;
            who = __builtin_bit_cast(int, pts[2 * (i_first + (lane & (R - 1)))].w);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 P = pts[2 * (i_first + r)];
                xi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.x)));
                yi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.y)));
                zi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.z)));
            }
        }

        const int vt0 = (int)(((long)tiles * chunk) / chunks);
        const int vt1 = (int)(((long)tiles * (chunk + 1)) / chunks);

        murb_f2 xx[R], yy[R], zz[R], xy[R], xz[R], yz[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            xx[r] = (murb_f2)(0.f); yy[r] = (murb_f2)(0.f); zz[r] = (murb_f2)(0.f);
            xy[r] = (murb_f2)(0.f); xz[r] = (murb_f2)(0.f); yz[r] = (murb_f2)(0.f);
        }

        for (int vs = vt0; vs < vt1; vs += STAGE) {
            const int nt = (vt1 - vs) < STAGE ? (vt1 - vs) : STAGE;
            __syncthreads();   // previous stage (of this unit or the one before) fully consumed
            for (int t = 0; t < nt; ++t) {
                const float4* srcq = a.rec + (unsigned long)(vs + t) * MURB_TILE_F4;   // vs + t < vt1 <= tiles
#pragma unroll
                for (int c = 0; c < MURB_TILE_F4 / (WAVES * 64); ++c) {
                    const int k = tid + c * WAVES * 64;
                    lds[t * MURB_TILE_F4 + k] = srcq[k];
                }
            }
            __syncthreads();
            for (int t = 0; t < nt; ++t) {
                const float4* tq = lds + t * MURB_TILE_F4;
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
                    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        murb_tidal_pair_pk(xj, yj, zj, gj * pm[r], xi[r], yi[r], zi[r], soft2, xx[r], yy[r], zz[r], xy[r], xz[r], yz[r]);
                }
            }
        }

        // the tile of every point's skipped slot, for that point alone (wave-uniform branches)
        {
            const auto* again = murb_kernarg_again<MurbTidalArgs>();
            const float4* const rec = again->rec;
            int w = who;
            asm volatile("" : "+v"(w));
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int skip = __builtin_amdgcn_readlane(w, r), skip_tile = skip >> 9;
                if (skip_tile >= vt0 && skip_tile < vt1)   // inside the layout: vt1 <= tiles
                    murb_tidal_skip_tile(rec, lane, skip, xi[r], yi[r], zi[r], soft2, xx[r], yy[r], zz[r], xy[r], xz[r], yz[r]);
            }
        }

        // fold the 64 lanes x 2 halves of every accumulator; lane r keeps point r's totals
        float oa[4] = {0.f, 0.f, 0.f, 0.f}, ob[2] = {0.f, 0.f};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float sxx = murb_wave_sum(xx[r].x + xx[r].y), syy = murb_wave_sum(yy[r].x + yy[r].y), szz = murb_wave_sum(zz[r].x + zz[r].y);
            const float sxy = murb_wave_sum(xy[r].x + xy[r].y), sxz = murb_wave_sum(xz[r].x + xz[r].y), syz = murb_wave_sum(yz[r].x + yz[r].y);
            if (lane == r) { oa[0] = sxx; oa[1] = syy; oa[2] = szz; oa[3] = sxy; ob[0] = sxz; ob[1] = syz; }
        }
        if (lane < R) {
            const auto* end = murb_kernarg_again<MurbTidalArgs>();
            const unsigned long at = (unsigned long)chunk * end->stride + (unsigned long)i_first + lane;   // < chunks * 16 * groups
            end->part_a[at] = make_float4(oa[0], oa[1], oa[2], oa[3]);
            end->part_b[at] = make_float4(ob[0], ob[1], 0.f, 0.f);
        }
    }
}

// launch 3: one thread per point of the launch.  fp32, chunks in ascending order.  out: txx | tyy | tzz | txy | txz | tyz,
// out_stride floats each.
__global__ __launch_bounds__(256) void murb_tidal_rows_kernel(const float4* part_a, const float4* part_b, float* out, const int count,
                                                              const int chunks, const unsigned int stride, const unsigned int out_stride)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= count) return;
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < chunks; ++c) {
        const float4 u = part_a[(unsigned long)c * stride + p];
        const float4 w = part_b[(unsigned long)c * stride + p];
        s[0] += u.x; s[1] += u.y; s[2] += u.z; s[3] += u.w;
        s[4] += w.x; s[5] += w.y;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) out[(unsigned long)k * out_stride + p] = s[k];
}

#endif
