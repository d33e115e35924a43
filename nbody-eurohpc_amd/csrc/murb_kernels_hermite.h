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
__device__ __forceinline__ void murb_interact_jerk_pk(const murb_f2 xj, const murb_f2 yj, const murb_f2 zj, const murb_f2 gj,
                                                      const murb_f2 uj, const murb_f2 vj, const murb_f2 wj,
                                                      const float xi, const float yi, const float zi,
                                                      const float ui, const float vi, const float wi, const float soft2,
                                                      murb_f2& ax, murb_f2& ay, murb_f2& az,
                                                      murb_f2& jx, murb_f2& jy, murb_f2& jz)
{
    const murb_f2 dx = xj - xi, dy = yj - yi, dz = zj - zi;
    const murb_f2 wx = uj - ui, wy = vj - vi, wz = wj - wi;
    murb_f2 r2 = __builtin_elementwise_fma(dx, dx, (murb_f2)(soft2));
    r2 = __builtin_elementwise_fma(dy, dy, r2);
    r2 = __builtin_elementwise_fma(dz, dz, r2);
    murb_f2 dw = dx * wx;
    dw = __builtin_elementwise_fma(dy, wy, dw);
    dw = __builtin_elementwise_fma(dz, wz, dw);
    murb_f2 inv;
    inv.x = __builtin_amdgcn_rsqf(r2.x);
    inv.y = __builtin_amdgcn_rsqf(r2.y);
    const murb_f2 inv2 = inv * inv;
    const murb_f2 gi = gj * inv;
    const murb_f2 s = gi * inv2;            // GM_j * inv^3, never G*inv^3 alone (fp32 range)
    const murb_f2 c = (dw * inv2) * -3.0f;  // -3 (d.w) / (|d|^2 + soft^2)
    ax = __builtin_elementwise_fma(s, dx, ax);
    ay = __builtin_elementwise_fma(s, dy, ay);
    az = __builtin_elementwise_fma(s, dz, az);
    jx = __builtin_elementwise_fma(s, __builtin_elementwise_fma(c, dx, wx), jx);
    jy = __builtin_elementwise_fma(s, __builtin_elementwise_fma(c, dy, wy), jy);
    jz = __builtin_elementwise_fma(s, __builtin_elementwise_fma(c, dz, wz), jz);
}

// ---- the sweep -------------------------------------------------------------------------------------------------------
// grid.x = i groups of WAVES*R bodies, grid.y = j chunks.  LDS: STAGE position tiles + STAGE velocity tiles (16 KiB a stage).
// The body is a device function so that the adaptive launch (murb_force_jerk_adaptive_kernel, below) runs the same code.
template <int R, int WAVES, int STAGE>
__device__ __forceinline__ void murb_force_jerk_sweep(const MurbJerkArgs a)
{
    static_assert(R % 2 == 0 && MURB_TILE_BODIES % (WAVES * R) == 0, "i groups must tile the layout");
    __shared__ float4 lds[2 * STAGE * MURB_TILE_F4];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i_slot = (blockIdx.x * WAVES + wave) * R;   // wave-uniform; the host keeps the grid inside the slots

    // the wave's R i bodies -> scalar registers
    float xi[R], yi[R], zi[R], ui[R], vi[R], wi[R];
    {
        const unsigned long ra = murb_rec_a((unsigned long)(i_slot >> 1));
#pragma unroll
        for (int h = 0; h < R / 2; ++h) {
            const float4 A = a.rec[ra + h], B = a.rec[ra + h + MURB_TILE_PAIRS];
            const float4 VA = a.vel[ra + h], VB = a.vel[ra + h + MURB_TILE_PAIRS];
            xi[2 * h] = A.x; xi[2 * h + 1] = A.y; yi[2 * h] = A.z; yi[2 * h + 1] = A.w; zi[2 * h] = B.x; zi[2 * h + 1] = B.y;
            ui[2 * h] = VA.x; ui[2 * h + 1] = VA.y; vi[2 * h] = VA.z; vi[2 * h + 1] = VA.w; wi[2 * h] = VB.x; wi[2 * h + 1] = VB.y;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            xi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, xi[r])));
            yi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, yi[r])));
            zi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, zi[r])));
            ui[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ui[r])));
            vi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, vi[r])));
            wi[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wi[r])));
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

    for (int vs = vt0; vs < vt1; vs += STAGE) {
        const int nt = (vt1 - vs) < STAGE ? (vt1 - vs) : STAGE;
        __syncthreads();   // previous stage fully consumed
        for (int t = 0; t < nt; ++t) {
            const float4* srcq = a.rec + (unsigned long)(vs + t) * MURB_TILE_F4;
            const float4* srcv = a.vel + (unsigned long)(vs + t) * MURB_TILE_F4;
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

    // fold the 64 lanes x 2 halves of every accumulator; lane r keeps body r's totals
    float oa[3] = {0.f, 0.f, 0.f}, oj[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float sx = murb_wave_sum(ax[r].x + ax[r].y), sy = murb_wave_sum(ay[r].x + ay[r].y), sz = murb_wave_sum(az[r].x + az[r].y);
        const float tx = murb_wave_sum(jx[r].x + jx[r].y), ty = murb_wave_sum(jy[r].x + jy[r].y), tz = murb_wave_sum(jz[r].x + jz[r].y);
        if (lane == r) { oa[0] = sx; oa[1] = sy; oa[2] = sz; oj[0] = tx; oj[1] = ty; oj[2] = tz; }
    }
    if (lane < R) {
        const unsigned long at = (unsigned long)chunk * a.stride + (unsigned long)i_slot + lane;
        a.part_a[at] = make_float4(oa[0], oa[1], oa[2], 0.f);
        a.part_j[at] = make_float4(oj[0], oj[1], oj[2], 0.f);
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
    for (int p = 0; p < a.nparts; ++p) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 u = a.part_a[(unsigned long)p * n + s0 + h];
            const float4 w = a.part_j[(unsigned long)p * n + s0 + h];
            f.a1[h][0] += u.x; f.a1[h][1] += u.y; f.a1[h][2] += u.z;
            f.j1[h][0] += w.x; f.j1[h][1] += w.y; f.j1[h][2] += w.z;
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
#define MURB_F32_INF_BITS 0x7f800000u

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
                                         const float dt_hi, const unsigned long long max_steps, const int fresh)
{
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
    if (was_last || c->steps >= c->max_steps) c->done = 1;
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
    }
    murb_evolve_fold_min(ctl, mine);
}

#endif
