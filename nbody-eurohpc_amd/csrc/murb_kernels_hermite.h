// gfx950 (CDNA4) kernels of the 4th-order Hermite predictor-corrector (Makino & Aarseth 1992), option "integrator" 2.
// Device code only; included through murb_ctx.h.  Replaces the reference's first-order update (Bodies.cpp:260-278).
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
// live in a control block in device memory and the device chooses every step's size (murbhip_evolve;
// murb_kernels_adaptive.h).  Sweep, predictor and corrector are device functions that both sets of kernels call.
#ifndef MURB_KERNELS_HERMITE_H_
#define MURB_KERNELS_HERMITE_H_

#include "murb_kernels_side.h"

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

struct MurbNNJerkArgs : MurbJerkArgs {
    int count;   // real bodies: slots >= count are padding
};

// ---- the sweep -------------------------------------------------------------------------------------------------------
// grid.x = i groups of WAVES*R bodies, grid.y = j chunks.  LDS: STAGE position tiles + STAGE velocity tiles (16 KiB a stage).
// The body is a device function so that the adaptive launch (murb_force_jerk_adaptive_kernel, murb_kernels_adaptive.h) runs the same code.
// SIDE: the side product kept beside the sums (Args = MurbNNJerkArgs where there is one); the plain form's code does not
// change with the others.  NN names what the three share (the copy in whole rounds, the kernel arguments read again behind
// the loop); the potential form (POT) keeps R packed sums in the place of the minima and steps.
template <int R, int WAVES, int STAGE, MurbSide SIDE = MurbSide::None, typename Args = MurbJerkArgs>
__device__ __forceinline__ void murb_force_jerk_sweep(const Args a)
{
    constexpr bool NN = SIDE != MurbSide::None, CT = SIDE == MurbSide::Contact, POT = SIDE == MurbSide::Potential;
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
            murb_sweep_tile<R, SIDE, 1>(tq, tv, lane, vs + t, self_tile, count, xi, yi, zi, ui, vi, wi, ri, soft2, ax, ay, az, jx, jy, jz, mn, st, ph);
        }
    }

    float nn_a = 0.f, nn_j = 0.f;   // the rows' fourth floats
    if constexpr (NN) {
        const auto* again = murb_kernarg_again<Args>();   // `a` is the kernel's first argument
        const float4* const rec = again->rec;
        int cnt = 0;
        if constexpr (!POT) cnt = again->count;
        int self[R], first = i_slot;
        asm volatile("" : "+s"(first));   // the bodies' slots are made here, not held through the loop
#pragma unroll
        for (int r = 0; r < R; ++r) self[r] = first + r;
        const int tiles = again->tiles, nchunks = again->nchunks;
        const int t0 = (int)(((long)tiles * chunk) / nchunks), t1 = (int)(((long)tiles * (chunk + 1)) / nchunks);   // vt0, vt1 again
        const int own[1] = {first / MURB_TILE_BODIES};
        if constexpr (POT) {
            if (own[0] >= t0 && own[0] < t1) murb_pot_own_tile<R>(rec, lane, own[0], xi, yi, zi, soft2, ph, self);   // wave-uniform
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float sp = murb_wave_sum(ph[r].x + ph[r].y);
                if (lane == r) nn_a = sp;   // part_j.w stays 0
            }
        } else {
            unsigned int nn_r2, nn_idx;
            using M = std::conditional_t<CT, MurbContactMetric, MurbNearestMetric>;
            const float4* vel = nullptr;   // the j radii
            if constexpr (CT) vel = again->vel;
            for (int tile = t0; tile < t1; ++tile)
                if (murb_nn_tile_masked<1>(tile, own, cnt)) murb_side_masked_tile<R, M>(rec, vel, lane, tile, xi, yi, zi, ri, soft2, mn, st, self, cnt);
            murb_side_finish<R, M>(rec, vel, lane, xi, yi, zi, ri, soft2, mn, st, self, cnt, nn_r2, nn_idx);
            nn_a = __builtin_bit_cast(float, nn_r2);
            nn_j = __builtin_bit_cast(float, nn_idx);
        }
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
// ones (dt read from the control block, murb_kernels_adaptive.h) run the same code.
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
    f.nn_r2[0] = f.nn_r2[1] = a.contact ? MurbContactMetric::key(__builtin_inff()) : MurbNearestMetric::key(__builtin_inff());
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
            if (a.contact) murb_side_store<MurbContactMetric>(a.nn_idx, a.nn_r2, s0 + h, f.nn_r2[h], f.nn_idx[h]);
            else murb_side_store<MurbNearestMetric>(a.nn_idx, a.nn_r2, s0 + h, f.nn_r2[h], f.nn_idx[h]);
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

#endif
