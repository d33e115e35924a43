// gfx950 (CDNA4) kernels of the k-nearest-neighbour read-out (murbknn_of / murbknn_at / murbdensity_of / murbdensity_centre).
// Device code only; included by murb_ctx.h.
#ifndef MURB_KERNELS_KNN_H_
#define MURB_KERNELS_KNN_H_

#include "murb_field.h"
#include "murb_kernels_side.h"
#include "murb_knn.h"

// ---- k nearest neighbours of arbitrary points (include/murbknn.h has the definition) ----------------------------------------
// The field read-out's rectangular sweep (murb_kernels_field.h) with a sorted list in the place of the sums: `count` points
// against ALL bodies at their current positions, per point the k smallest (r2, index) with one body slot left out.
//     1  murb_field_pack_kernel    the field read-out's, as it is: {x, y, z, skip} is the first of a point's two records
//     2  murb_knn_sweep_kernel     the field sweep's walk over (group of 16 points, j chunk) units on the same fixed grid; per unit
//                                  and point one sorted list of k entries: part[(chunk * stride + point) * k + l]
//     3  murb_knn_rows_kernel      one thread per point: the chunks' lists merged in chunk order (murb_knn_merge)
//     4  murb_knn_density_kernel   one thread per point: murb_knn_density of its list
//     5  murb_knn_centre_kernel    256-body block sums in fp64 (murb_metrics_kernel's order), twice: the first moments, then
//                                  the second moment about the centre the first pass gave
// A point's list lies ACROSS THE LANES of two vector registers: lane l holds entry l's r2 and index, sorted ascending, empty
// places +inf / MURB_KNN_NONE.  The r2 and the index of its k-th entry (the threshold) are wave-uniform and sit in scalar
// registers; until the list is full the threshold is (+inf, none) and everything passes it.
// The loop forms r2 alone (3 packed subtractions, 3 packed fmas per pair of interactions), takes the minimum of the two
// halves, compares it with the threshold and branches on the ballot: 8 vector instructions per pair of interactions and
// point.  A lane step in which some lane holds an r2 <= threshold goes the slow way (murb_knn_lane_step): each flagged
// candidate is tested exactly, (r2, index) against the threshold entry, with index < n and index != skip tested there and
// only there (the body itself and the padding at the origin pass the loop's compare and are turned away here), and the
// survivors are inserted one at a time.  The k smallest of a set under a total order do not depend on the order in which the
// set is presented, so neither lanes, halves, tiles nor chunks leave a trace in the list.
#define MURB_KNN_NONE 0x7fffffff   // "no candidate" in the lists on the device (the public index is -1)

struct MurbKnnArgs {
    const float4* rec;      // current positions + GM, all slots
    const float4* pts;      // two records per point (murb_field_pack_kernel); the first is read
    float* part_r2;         // part_r2[(chunk * stride + point) * k + l]
    int* part_idx;          // ... the indices, MURB_KNN_NONE where there is none
    int groups, chunks;     // the launch's units
    int tiles;              // layout tiles swept as j (those that hold real bodies)
    int count;              // real bodies: slots >= count are padding and never candidates
    int k;                  // 1 .. MURB_KNN_KMAX
    unsigned int stride;    // points per chunk row: 16 * groups
    float soft2;
};

// One candidate (wave-uniform) that comes before the threshold entry into a point's list.  Lane l < k keeps its entry where
// that comes before the candidate, takes the candidate at the first place behind those, and its left neighbour's entry
// further up; the former k-th entry falls off the end.
__device__ __forceinline__ void murb_knn_insert(float& lr2, int& lidx, float& thr, int& thr_idx, const float cr2, const int cidx,
                                                const int k, const int lane)
{
    const bool live = lane < k;
    const bool keep = live && murb_knn_before(lr2, lidx, cr2, cidx);   // a prefix of the lanes: the list is sorted
    const int pos = __builtin_popcountll(__builtin_amdgcn_ballot_w64(keep));
    // the left neighbour's entry: wave_shr:1 (lane 0 keeps its own, and never takes it: pos >= 0)
    const float up_r2 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, lr2), __builtin_bit_cast(int, lr2), 0x138, 0xF, 0xF, false));
    const int up_idx = __builtin_amdgcn_update_dpp(lidx, lidx, 0x138, 0xF, 0xF, false);
    lr2 = !live ? __builtin_inff() : lane < pos ? lr2 : lane == pos ? cr2 : up_r2;
    lidx = !live ? MURB_KNN_NONE : lane < pos ? lidx : lane == pos ? cidx : up_idx;
    thr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lr2), k - 1));
    thr_idx = __builtin_amdgcn_readlane(lidx, k - 1);
}

// The slow way of one lane step for one point: the lanes' two candidates (slots j0, j0 + 1 of lane 0's j_first + 2 * lane, with
// r2.x, r2.y) tested exactly and inserted.  Wave-uniform throughout: the lanes flagged under the threshold entry of the
// moment are taken one at a time off a ballot, and each is tested again, in scalar registers, against the threshold entry as
// the insertions before it have left it: of the 128 candidates of a first trip all are looked at (two lane reads and a
// compare each) and few are inserted.  (Flagging anew after every insertion was measured a tenth slower)
__device__ __forceinline__ void murb_knn_lane_step(float& lr2, int& lidx, float& thr, int& thr_idx, const murb_f2 r2, const int j_first,
                                                   const int skip, const int count, const int k, const int lane)
{
    const int j0 = j_first + 2 * lane;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float c = h ? r2.y : r2.x;
        const int j = j0 + h;
        unsigned long todo = __builtin_amdgcn_ballot_w64(j < count && j != skip && murb_knn_before(c, j, thr, thr_idx));
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float cr2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c), src));
            const int cidx = j_first + 2 * src + h;
            if (murb_knn_before(cr2, cidx, thr, thr_idx)) murb_knn_insert(lr2, lidx, thr, thr_idx, cr2, cidx, k, lane);   // scalar
        }
    }
}

// launch 2.  murb_force_field_kernel's mapping: a workgroup takes a group of 16 points, 4 per wave, their values
// wave-uniform, and walks units u = blockIdx.x, += gridDim.x with (group, chunk) = (u % groups, u / groups).  STAGE tiles of
// 8 KiB each in LDS: positions alone, like the tidal sweep.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_knn_sweep_kernel(const MurbKnnArgs a)
{
    static_assert(R % 2 == 0 && WAVES * R == MURB_FIELD_GROUP, "a workgroup takes one group of points");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
    static_assert(STAGE * MURB_TILE_F4 * sizeof(float4) * 4 <= 160 * 1024, "4 workgroups per CU share its LDS");
    static_assert(MURB_KNN_KMAX <= 64, "a list lies across the lanes of one wave");
    __shared__ float4 lds[STAGE * MURB_TILE_F4];
    const float soft2 = a.soft2;
    const int k = a.k, count = a.count;

    for (int u = blockIdx.x;; u += (int)gridDim.x) {
        const int groups = a.groups, chunks = a.chunks, tiles = a.tiles;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        const int tid = threadIdx.x;
        const int lane = tid & 63;
        const int i_first = (group * WAVES + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;   // point of the launch, wave-uniform

        float xi[R], yi[R], zi[R];
        int skip[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 P = a.pts[2 * (i_first + r)];
            xi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.x)));
            yi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.y)));
            zi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.z)));
            skip[r] = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, P.w));
        }

        const int vt0 = (int)(((long)tiles * chunk) / chunks);
        const int vt1 = (int)(((long)tiles * (chunk + 1)) / chunks);

        float lr2[R], thr[R];
        int lidx[R], thr_idx[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            lr2[r] = __builtin_inff(); lidx[r] = MURB_KNN_NONE;
            thr[r] = __builtin_inff(); thr_idx[r] = MURB_KNN_NONE;
        }

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
#pragma unroll 2
                for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
                    const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
                    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y};
                    const int j_first = (vs + t) * MURB_TILE_BODIES + 2 * q;   // lane 0's first slot
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const murb_f2 dx = xj - xi[r], dy = yj - yi[r], dz = zj - zi[r];
                        murb_f2 r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
                        r2 = __builtin_elementwise_fma(dy, dy, r2);
                        r2 = __builtin_elementwise_fma(dz, dz, r2);
                        const float m = __builtin_fminf(r2.x, r2.y);
                        if (__builtin_amdgcn_ballot_w64(m <= thr[r]) != 0)   // wave-uniform
                            murb_knn_lane_step(lr2[r], lidx[r], thr[r], thr_idx[r], r2, j_first, skip[r], count, k, lane);
                    }
                }
            }
        }

        if (lane < k) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const unsigned long at = ((unsigned long)chunk * a.stride + (unsigned long)(i_first + r)) * (unsigned long)k + lane;   // < chunks * 16 * groups * k
                a.part_r2[at] = lr2[r];
                a.part_idx[at] = lidx[r];
            }
        }
    }
}

// launch 3: one thread per point of the launch.  The chunks' lists folded in chunk order with murb_knn_merge; out_idx / out_r2
// [p * k + l] in the caller's order, -1 and +inf where there is no candidate.
__global__ __launch_bounds__(256) void murb_knn_rows_kernel(const float* part_r2, const int* part_idx, int* out_idx, float* out_r2,
                                                            const int count, const int chunks, const unsigned int stride, const int k)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= count) return;
    int ia[MURB_KNN_KMAX], ib[MURB_KNN_KMAX], ic[MURB_KNN_KMAX];
    float ra[MURB_KNN_KMAX], rb[MURB_KNN_KMAX], rc[MURB_KNN_KMAX];
    for (int l = 0; l < k; ++l) { ia[l] = -1; ra[l] = __builtin_inff(); }
    for (int c = 0; c < chunks; ++c) {
        const unsigned long at = ((unsigned long)c * stride + (unsigned long)p) * (unsigned long)k;
        for (int l = 0; l < k; ++l) {
            const int j = part_idx[at + l];
            ib[l] = j == MURB_KNN_NONE ? -1 : j;
            rb[l] = part_r2[at + l];
        }
        murb_knn_merge(k, ia, ra, ib, rb, ic, rc);
        for (int l = 0; l < k; ++l) { ia[l] = ic[l]; ra[l] = rc[l]; }
    }
    for (int l = 0; l < k; ++l) {
        out_idx[(unsigned long)p * k + l] = ia[l];
        out_r2[(unsigned long)p * k + l] = ra[l];
    }
}

// launch 4: one thread per point of the launch: the density of its list.  mass: the masses as uploaded, by body index.
__global__ __launch_bounds__(256) void murb_knn_density_kernel(const int* idx, const float* r2, const float* mass, float* rho,
                                                               const int count, const int k, const float soft2)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= count) return;
    rho[p] = murb_knn_density(k, idx + (unsigned long)p * k, r2 + (unsigned long)p * k, mass, soft2);
}

// launch 5, run twice: per block of 256 consecutive bodies the fp64 sums of the bodies with a finite rho, in
// murb_metrics_kernel's fixed order (wave shuffle tree, then the 4 waves through LDS); the host adds the block rows in index
// order.  second == 0: {rho, rho^2, rho x, rho y, rho z, 1, 0, 0}; second != 0: {rho^2 |q - X|^2, 0 ...} about X = (cx, cy, cz).
#define MURB_KNN_CENTRE_VALUES 8
__global__ __launch_bounds__(256) void murb_knn_centre_kernel(const float4* rec, const float* rho, double* out, const int count,
                                                              const int second, const double cx, const double cy, const double cz)
{
#pragma clang fp contract(off)
    __shared__ double red[3][MURB_KNN_CENTRE_VALUES];
    const int s = blockIdx.x * 256 + threadIdx.x;
    double v[MURB_KNN_CENTRE_VALUES];
#pragma unroll
    for (int e = 0; e < MURB_KNN_CENTRE_VALUES; ++e) v[e] = 0.0;
    if (s < count) {
        const float rf = rho[s];
        if (rf < __builtin_inff()) {   // finite: rho is never negative or NaN
            const unsigned long ra = murb_rec_a((unsigned long)(s >> 1));
            const int h = s & 1;
            const float4 A = rec[ra], B = rec[ra + MURB_TILE_PAIRS];
            const double x = h ? A.y : A.x, y = h ? A.w : A.z, z = h ? B.y : B.x, w = rf;
            if (second) {
                const double ex = x - cx, ey = y - cy, ez = z - cz;
                v[0] = (w * w) * ((ex * ex + ey * ey) + ez * ez);
            } else {
                v[0] = w; v[1] = w * w; v[2] = w * x; v[3] = w * y; v[4] = w * z; v[5] = 1.0;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < MURB_KNN_CENTRE_VALUES; ++e)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[e] += __shfl_down(v[e], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0 && wave > 0) {
#pragma unroll
        for (int e = 0; e < MURB_KNN_CENTRE_VALUES; ++e) red[wave - 1][e] = v[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < MURB_KNN_CENTRE_VALUES; ++e)
            out[(unsigned long)blockIdx.x * MURB_KNN_CENTRE_VALUES + e] = ((v[e] + red[0][e]) + red[1][e]) + red[2][e];
    }
}

#endif
