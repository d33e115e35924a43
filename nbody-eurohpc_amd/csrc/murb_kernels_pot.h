// gfx950 (CDNA4) kernels of the potential read-out and of the bound members (murbpot_of / murbpot_at / murbbound_members).
// Device code only; included by murb_ctx.h.
#ifndef MURB_KERNELS_POT_H_
#define MURB_KERNELS_POT_H_

#include "murb_bound.h"
#include "murb_field.h"
#include "murb_kernels_field.h"
#include "murb_kernels_side.h"

// ---- potential of a subset of the bodies at arbitrary points (include/murbbound.h has the definition) ------------------------
// The field read-out's rectangular sweep (murb_kernels_field.h) with phi alone: `count` points against the bodies of a subset
// S at their current positions, per point the sum of G m_j inv with one body slot left out.
//     0  murb_pot_mask_kernel      with a mask alone: a copy of the position + G m records in which the bodies outside S
//                                  carry G m = +0; the sweep reads the copy, so the mask costs the loop nothing
//     1  murb_field_pack_kernel    the field read-out's, as it is: {x, y, z, skip} is the first of a point's two records
//     2  murb_pot_sweep_kernel     the field sweep's walk over (group of 16 points, j chunk) units on the same fixed grid; one
//                                  float per unit and point: part[chunk * stride + point]
//     3  murb_pot_rows_kernel      one thread per point: the rows added in chunk order
// The arithmetic is the field sweep's phi, operation for operation, so that the bits are (tests/test_bound_gpu.py compares
// them): r2 from three packed subtractions and three packed fmas, v_rsq_f32, then phi = fma(G m_j * pm, inv, phi) with pm the
// wave-uniform multiplier that is 0 for a point in the tile of its OWN skipped slot alone and 1 otherwise (G m_j * 1 is exact).
// Behind the loop that tile is swept once more for that point from the records in memory with the slot's G m replaced by 0
// through a select: "the chunk's tiles in layout order, then the tile of the skipped slot", the field sweep's order.
// Per pair of interactions and point: 3 v_pk_add_f32, 4 v_pk_fma_f32, 1 v_pk_mul_f32 and 2 v_rsq_f32, no velocity tiles.
struct MurbPotArgs {
    const float4* rec;      // positions + GM, all slots that hold real bodies: the records, or the masked copy
    const float4* pts;      // two records per point (murb_field_pack_kernel); the first is read
    float* part;            // part[chunk * stride + point]
    int groups, chunks;     // the launch's units
    int tiles;              // layout tiles swept as j (those that hold real bodies)
    unsigned int stride;    // points per chunk row: 16 * groups
    float soft2;
};

// launch 0: one thread per record of the tiles that hold real bodies.  A records (x, y) are copied; in B records (z, G m) the
// G m of a real body outside the set becomes +0.  Padding slots keep what they carry (G m = 0).
__global__ __launch_bounds__(256) void murb_pot_mask_kernel(const float4* rec, const unsigned char* member, float4* out, const int count,
                                                            const unsigned int records)
{
    const unsigned int r = blockIdx.x * 256u + threadIdx.x;
    if (r >= records) return;
    float4 v = rec[r];
    const unsigned int tile = r / MURB_TILE_F4, within = r % MURB_TILE_F4;
    if (within >= MURB_TILE_PAIRS) {
        const int j0 = (int)(2u * (tile * MURB_TILE_PAIRS + (within - MURB_TILE_PAIRS)));
        if (j0 < count && !member[j0]) v.z = 0.f;
        if (j0 + 1 < count && !member[j0 + 1]) v.w = 0.f;
    }
    out[r] = v;
}

// One point against the tile of its skipped slot, from the records in memory: the loop's packed arithmetic, the slot's G m
// replaced by 0 (murb_field_skip_tile's phi).  Lane steps rising, like the loop's.
__device__ __forceinline__ void murb_pot_skip_tile(const float4* rec, const int lane, const int skip, const float xi, const float yi,
                                                   const float zi, const float soft2, murb_f2& ph)
{
    const int tile = skip / MURB_TILE_BODIES;
#pragma unroll 1
    for (int qs = 0; qs < MURB_TILE_PAIRS / 64; ++qs) {
        const unsigned long ra = (unsigned long)tile * MURB_TILE_F4 + qs * 64 + lane;
        const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
        const int j0 = tile * MURB_TILE_BODIES + 2 * (qs * 64 + lane);
        const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y};
        const murb_f2 gj = {j0 == skip ? 0.f : B.z, j0 + 1 == skip ? 0.f : B.w};
        const murb_f2 dx = xj - xi, dy = yj - yi, dz = zj - zi;
        murb_f2 r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
        r2 = __builtin_elementwise_fma(dy, dy, r2);
        r2 = __builtin_elementwise_fma(dz, dz, r2);
        murb_f2 inv;
        inv.x = __builtin_amdgcn_rsqf(r2.x);
        inv.y = __builtin_amdgcn_rsqf(r2.y);
        ph = __builtin_elementwise_fma(gj, inv, ph);
    }
}

// launch 2.  murb_knn_sweep_kernel's frame: a workgroup takes a group of 16 points, 4 per wave, their values wave-uniform in
// scalar registers, and walks units u = blockIdx.x, += gridDim.x with (group, chunk) = (u % groups, u / groups).  STAGE tiles of
// 8 KiB each in LDS: positions + G m alone.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_pot_sweep_kernel(const MurbPotArgs a)
{
    static_assert(R % 2 == 0 && WAVES * R == MURB_FIELD_GROUP, "a workgroup takes one group of points");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
    static_assert(STAGE * MURB_TILE_F4 * sizeof(float4) * 4 <= 160 * 1024, "4 workgroups per CU share its LDS");
    static_assert(MURB_TILE_BODIES == 1 << 9, "a slot's tile is slot >> 9");
    __shared__ float4 lds[STAGE * MURB_TILE_F4];
    const float soft2 = a.soft2;

    for (int u = blockIdx.x;; u += (int)gridDim.x) {
        const int groups = a.groups, chunks = a.chunks, tiles = a.tiles;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        const int i_first = (group * WAVES + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;   // point of the launch, wave-uniform

        float xi[R], yi[R], zi[R];
        int skip[R];
        murb_f2 ph[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 P = a.pts[2 * (i_first + r)];
            xi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.x)));
            yi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.y)));
            zi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.z)));
            skip[r] = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.w));
            ph[r] = (murb_f2)(0.f);
        }

        const int vt0 = (int)(((long)tiles * chunk) / chunks);
        const int vt1 = (int)(((long)tiles * (chunk + 1)) / chunks);

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
                float pm[R];   // wave-uniform, per point: 0 in the tile of the point's OWN skipped slot alone
#pragma unroll
                for (int r = 0; r < R; ++r) pm[r] = (skip[r] >> 9) == vs + t ? 0.f : 1.f;   // -1 >> 9 = -1: no tile
#pragma unroll
                for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
                    const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
                    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const murb_f2 dx = xj - xi[r], dy = yj - yi[r], dz = zj - zi[r];
                        murb_f2 r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
                        r2 = __builtin_elementwise_fma(dy, dy, r2);
                        r2 = __builtin_elementwise_fma(dz, dz, r2);
                        murb_f2 inv;
                        inv.x = __builtin_amdgcn_rsqf(r2.x);
                        inv.y = __builtin_amdgcn_rsqf(r2.y);
                        const murb_f2 gp = gj * pm[r];
                        ph[r] = __builtin_elementwise_fma(gp, inv, ph[r]);
                    }
                }
            }
        }

        // the tile of every point's skipped slot, for that point alone (wave-uniform branches)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int skip_tile = skip[r] >> 9;
            if (skip_tile >= vt0 && skip_tile < vt1) murb_pot_skip_tile(a.rec, lane, skip[r], xi[r], yi[r], zi[r], soft2, ph[r]);
        }

        // fold the 64 lanes x 2 halves; lane r keeps point r's total
        float o = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float sp = murb_wave_sum(ph[r].x + ph[r].y);
            if (lane == r) o = sp;
        }
        if (lane < R) a.part[(unsigned long)chunk * a.stride + (unsigned long)i_first + lane] = o;   // < chunks * 16 * groups
    }
}

// launch 3: one thread per point of the launch.  fp32, chunks in ascending order (murb_field_rows_kernel's phi).
__global__ __launch_bounds__(256) void murb_pot_rows_kernel(const float* part, float* out, const int count, const int chunks,
                                                            const unsigned int stride)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= count) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(unsigned long)c * stride + p];
    out[p] = s;
}

// ---- bound members (murbbound_members) ---------------------------------------------------------------------------------------
// One thread per body, 256 bodies per block, fp64 without contraction (csrc/murb_bound.h holds the arithmetic).

// a body's velocity from the records
__device__ __forceinline__ void murb_bound_velocity(const float4* vel, const int s, float& vx, float& vy, float& vz)
{
    const unsigned long ra = murb_rec_a((unsigned long)(s >> 1));
    const float* const pv = (const float*)(vel + ra) + (s & 1);
    vx = pv[0]; vy = pv[2]; vz = pv[4 * MURB_TILE_PAIRS];   // lanes z, w of the B record may carry radii ("contact"): never read
}

// 256-body block sums in murb_metrics_kernel's fixed order (wave shuffle tree, then the 4 waves through LDS); thread 0 writes
// the block's row.  The host adds the block rows in index order.
template <int VALUES>
__device__ __forceinline__ void murb_bound_block_sums(double (&v)[VALUES], double (&red)[3][VALUES], double* out)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < VALUES; ++e)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[e] += __shfl_down(v[e], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0 && wave > 0) {
#pragma unroll
        for (int e = 0; e < VALUES; ++e) red[wave - 1][e] = v[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < VALUES; ++e) out[(unsigned long)blockIdx.x * VALUES + e] = ((v[e] + red[0][e]) + red[1][e]) + red[2][e];
    }
}

// A round's evaluation: e of every real body against the sweep's phi and the frame V.  update != 0: the members whose e is not
// negative leave (NaN leaves), and the block rows count them; update == 0 (the final pass): the set stays as it is.
__global__ __launch_bounds__(256) void murb_bound_energy_kernel(const float4* vel, const float* phi, unsigned char* member, double* e,
                                                                double* removed, const int count, const int update, const double Vx,
                                                                const double Vy, const double Vz)
{
    __shared__ double red[3][1];
    const int s = blockIdx.x * 256 + threadIdx.x;
    double v[1] = {0.0};
    if (s < count) {
        const double V[3] = {Vx, Vy, Vz};
        float vx, vy, vz;
        murb_bound_velocity(vel, s, vx, vy, vz);
        const double es = murb_bound_energy(vx, vy, vz, V, phi[s]);
        e[s] = es;
        if (update && member[s] && !murb_bound_stays(es)) {
            member[s] = 0;
            v[0] = 1.0;
        }
    }
    murb_bound_block_sums<1>(v, red, removed);
}

// The sums of a set, per block a row of MURB_BOUND_SUMS values (csrc/murb_bound.h): members, m, m v, m q over the set; with
// energy != 0 also K = sum of (0.5 m) |v - V|^2 and sum of m phi over the set, and the real bodies with e >= 0.  mass: the masses as
// uploaded, by body index.
__global__ __launch_bounds__(256) void murb_bound_sums_kernel(const float4* rec, const float4* vel, const float* mass,
                                                              const unsigned char* member, const float* phi, const double* e, double* out,
                                                              const int count, const int energy, const double Vx, const double Vy,
                                                              const double Vz)
{
#pragma clang fp contract(off)
    __shared__ double red[3][MURB_BOUND_SUMS];
    const int s = blockIdx.x * 256 + threadIdx.x;
    double v[MURB_BOUND_SUMS];
#pragma unroll
    for (int k = 0; k < MURB_BOUND_SUMS; ++k) v[k] = 0.0;
    if (s < count) {
        if (energy && e[s] >= 0.0) v[10] = 1.0;
        if (member[s]) {
            const unsigned long ra = murb_rec_a((unsigned long)(s >> 1));
            const float* const pq = (const float*)(rec + ra) + (s & 1);
            float vx, vy, vz;
            murb_bound_velocity(vel, s, vx, vy, vz);
            const double m = mass[s];
            v[0] = 1.0;
            v[1] = m;
            v[2] = m * (double)vx;
            v[3] = m * (double)vy;
            v[4] = m * (double)vz;
            v[5] = m * (double)pq[0];
            v[6] = m * (double)pq[2];
            v[7] = m * (double)pq[4 * MURB_TILE_PAIRS];
            if (energy) {
                const double V[3] = {Vx, Vy, Vz};
                const double hm = 0.5 * m;
                v[8] = hm * murb_bound_w2(vx, vy, vz, V);
                v[9] = m * (double)phi[s];
            }
        }
    }
    murb_bound_block_sums<MURB_BOUND_SUMS>(v, red, out);
}

#endif
