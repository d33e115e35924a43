// gfx950 (CDNA4) kernels of the pair-separation read-out (murbsep_of / murbsep_at).  Device code only; included by murb_ctx.h.
#ifndef MURB_KERNELS_SEP_H_
#define MURB_KERNELS_SEP_H_

#include "murb_field.h"
#include "murb_kernels_field.h"
#include "murb_sep.h"

// ---- pair separations of points against a subset of the bodies (include/murbsep.h has the definition) ------------------------
// The potential read-out's rectangular sweep (murb_kernels_pot.h) with the separation itself in the place of G m / r: `count`
// points against the bodies of a subset S, per point the sum of r over S, and over the whole call the pairs counted by the bits
// of their d2.
//     0  murb_sep_mask_kernel      always: a copy of the position records in which every slot that must not count (a body outside
//                                  S, padding) sits at (+inf, 0, 0) with a cap of +0 in the G m lane, and every slot that counts
//                                  carries a cap of +inf.  The loop pays no index, mask or own-body test per pair.
//     1  murb_field_pack_kernel    the field read-out's, as it is: {x, y, z, skip} is the first of a point's two records
//     2  murb_sep_sweep_kernel     the field sweep's walk over (group of 16 points, j chunk) units on the same fixed grid; one
//                                  float per unit and point: part[chunk * stride + point]; with HIST the workgroup's table of
//                                  32-bit counters, kept in LDS across its units and stored once: rows[workgroup][slot]
//     3  murb_sep_rows_kernel      one thread per point: the rows added in chunk order in fp64; one thread per slot: the
//                                  workgroups' rows added into the call's 64-bit totals in row order
// A slot that must not count has d2 = +inf (or NaN against a filler point at +inf): v_sqrt_f32 gives +inf or NaN, and
// v_min_f32 with its cap of +0 gives +0 for either, so it adds +0; its pair lands in the table's last slot ("above"; the table
// always has MURB_SEP_TABLE slots so that the clamp's bounds are constants, and every slot past the last bin is "above"), from
// which the host takes the exactly known number of such entries.  The points that fill the last group of 16 are moved to x = +inf in
// the sweep: every slot's d2 is then +inf or NaN, "above" as well, and their sums are never read.
// Per pair of interactions and point: 3 v_pk_add_f32 (subtractions), 3 v_pk_fma_f32, 2 v_sqrt_f32, 2 v_min_f32, 1 v_pk_add_f32;
// with HIST 2 v_lshrrev_b32, 2 v_lshl_add_u32, 2 v_med3_i32 and 2 ds_add_u32.  Per lane step 2 v_max_f32 quiet the caps.
struct MurbSepArgs {
    const float4* rec;      // the masked copy of the records, all slots of the tiles that hold real bodies
    const float4* pts;      // two records per point (murb_field_pack_kernel); the first is read
    float* part;            // part[chunk * stride + point]
    unsigned int* rows;     // HIST: rows[workgroup * MURB_SEP_TABLE + slot]
    int groups, chunks;     // the launch's units
    int tiles;              // layout tiles swept as j (those that hold real bodies)
    int count;              // points of the launch; those from count up to 16 * groups are fillers
    unsigned int stride;    // points per chunk row: 16 * groups
    int sh, minus4;         // HIST: murb_sep_slot_bytes' shift and -4 * (lowest key - 1)
};

// launch 0: one thread per pair of slots of the tiles that hold real bodies; both records of the pair are written.
__global__ __launch_bounds__(256) void murb_sep_mask_kernel(const float4* rec, const unsigned char* member, float4* out, const int count,
                                                            const unsigned int pairs)
{
    const unsigned int p = blockIdx.x * 256u + threadIdx.x;
    if (p >= pairs) return;
    const unsigned long ra = murb_rec_a(p);
    float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
    const int j0 = (int)(2u * p);
    const bool in0 = j0 < count && (!member || member[j0]);
    const bool in1 = j0 + 1 < count && (!member || member[j0 + 1]);
    const float inf = __builtin_inff();
    if (!in0) { A.x = inf; A.z = 0.f; B.x = 0.f; }
    if (!in1) { A.y = inf; A.w = 0.f; B.y = 0.f; }
    B.z = in0 ? inf : 0.f;
    B.w = in1 ? inf : 0.f;
    out[ra] = A;                       // ra + MURB_TILE_PAIRS < tiles * MURB_TILE_F4: p < tiles * MURB_TILE_PAIRS
    out[ra + MURB_TILE_PAIRS] = B;
}

// launch 2.  murb_pot_sweep_kernel's frame: a workgroup takes a group of 16 points, 4 per wave, their values wave-uniform in
// scalar registers, and walks units u = blockIdx.x, += gridDim.x with (group, chunk) = (u % groups, u / groups).  STAGE tiles of
// 8 KiB each in LDS: positions + caps alone.  HIST: 4 KiB of counters beside them.
template <int R, int WAVES, int STAGE, bool HIST>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_sep_sweep_kernel(const MurbSepArgs a)
{
    static_assert(R % 2 == 0 && WAVES * R == MURB_FIELD_GROUP, "a workgroup takes one group of points");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
    static_assert((STAGE * MURB_TILE_F4 * sizeof(float4) + MURB_SEP_TABLE * sizeof(unsigned int)) * 4 <= 160 * 1024,
                  "4 workgroups per CU share its LDS");
    __shared__ float4 lds[STAGE * MURB_TILE_F4];
    __shared__ unsigned int table[HIST ? MURB_SEP_TABLE : 1];
    const int sh = a.sh, minus4 = a.minus4;
    if (HIST) {
        for (int e = threadIdx.x; e < MURB_SEP_TABLE; e += WAVES * 64) table[e] = 0u;   // the loop's first barrier comes before any add
    }

    for (int u = blockIdx.x;; u += (int)gridDim.x) {
        const int groups = a.groups, chunks = a.chunks, tiles = a.tiles;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        const int i_first = (group * WAVES + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;   // point of the launch, wave-uniform

        float xi[R], yi[R], zi[R];
        murb_f2 s[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 P = a.pts[2 * (i_first + r)];
            xi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.x)));
            yi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.y)));
            zi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.z)));
            if (i_first + r >= a.count) xi[r] = __builtin_inff();   // a filler: every pair of it lands above
            s[r] = (murb_f2)(0.f);
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
#pragma unroll
                for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
                    const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
                    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y};
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const murb_f2 dx = xj - xi[r], dy = yj - yi[r], dz = zj - zi[r];
                        murb_f2 d2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(0.f));
                        d2 = __builtin_elementwise_fma(dy, dy, d2);
                        d2 = __builtin_elementwise_fma(dz, dz, d2);
                        murb_f2 m;
                        m.x = __builtin_fminf(__builtin_amdgcn_sqrtf(d2.x), B.z);
                        m.y = __builtin_fminf(__builtin_amdgcn_sqrtf(d2.y), B.w);
                        s[r] = s[r] + m;
                        if (HIST) {
                            const float even = d2.x, odd = d2.y;   // scalars: a bit cast of a vector's element reads element 0
                            // byte offsets in [0, 4 * (MURB_SEP_TABLE - 1)], multiples of 4: inside the table
                            atomicAdd((unsigned int*)((char*)table + murb_sep_slot_bytes(__builtin_bit_cast(unsigned int, even), sh, minus4)), 1u);
                            atomicAdd((unsigned int*)((char*)table + murb_sep_slot_bytes(__builtin_bit_cast(unsigned int, odd), sh, minus4)), 1u);
                        }
                    }
                }
            }
        }

        // fold the 64 lanes x 2 halves; lane r keeps point r's total
        float o = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float sp = murb_wave_sum(s[r].x + s[r].y);
            if (lane == r) o = sp;
        }
        if (lane < R) a.part[(unsigned long)chunk * a.stride + (unsigned long)i_first + lane] = o;   // < chunks * 16 * groups
    }

    if (HIST) {
        __syncthreads();   // every wave's adds have landed
        unsigned int* const row = a.rows + (unsigned long)blockIdx.x * MURB_SEP_TABLE;
        for (int e = threadIdx.x; e < MURB_SEP_TABLE; e += WAVES * 64) row[e] = table[e];
    }
}

// launch 3.  Thread p < count: point p's chunk rows in ascending order, in fp64.  Thread p < width (HIST alone: width =
// MURB_SEP_TABLE, else 0): slot p of the launch's `grid` workgroup rows added to the call's 64-bit total in row order.
__global__ __launch_bounds__(256) void murb_sep_rows_kernel(const float* part, double* sum, const int count, const int chunks,
                                                            const unsigned int stride, const unsigned int* rows,
                                                            unsigned long long* total, const int width, const int grid)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p < count) {
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += (double)part[(unsigned long)c * stride + p];
        sum[p] = s;
    }
    if (p < width) {
        unsigned long long t = total[p];
        for (int g = 0; g < grid; ++g) t += rows[(unsigned long)g * width + p];
        total[p] = t;
    }
}

#endif
