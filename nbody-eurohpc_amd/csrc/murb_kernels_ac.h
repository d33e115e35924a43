// gfx950 (CDNA4) kernels of the Ahmad-Cohen neighbour scheme (murbac_begin / murbac_steps; include/murbac.h has the definition).
// Device code only; included by murb_ctx.h.
#ifndef MURB_KERNELS_AC_H_
#define MURB_KERNELS_AC_H_

#include "murb_ac.h"
#include "murb_kernels_hermite.h"
#include "murb_kernels_list.h"

// ---- a Hermite step whose full sweep happens only on every n_irr-th step ---------------------------------------------------
// An irregular step is three launches, none of them O(N^2):
//     1  murb_ac_predict_kernel   the Hermite predictor, written straight into the gather form {x, y, z, G m} {u, v, w, 0} that
//                                 murb_list_pack_kernel produces (a regular step runs the existing predictor and that pack)
//     2  murb_ac_sweep_kernel     one wave per body over its resident list: murb_list_sweep_kernel's walk, the body's own point
//                                 read from gather records 2 i and 2 i + 1, begin and length from resident device arrays
//     3  murb_ac_correct_kernel   a1 = aI1 + the regular polynomial at tau, then the Hermite corrector
// A regular step ends in murb_ac_regular_kernel in the corrector's place: the rows of the full sweep, the derivative update on
// the old list, the new split, the Hermite corrector with the total.  No atomic operation anywhere.
struct MurbAcPredictArgs {
    const float4* rec;      // current positions + GM, all slots
    const float4* vel;      // current velocities
    const float* a0;        // ax | ay | az (stride each) of the remembered evaluation
    const float* j0;
    float4* src;            // two records per body
    int count;              // real bodies
    unsigned int stride;    // slots
    float dt;
};

__global__ __launch_bounds__(256) void murb_ac_predict_kernel(const MurbAcPredictArgs a)
{
#pragma clang fp contract(off)
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= a.count) return;
    const unsigned long ra = murb_rec_a((unsigned long)(j >> 1));
    const float* const q = (const float*)(a.rec + ra) + (j & 1);
    const float* const qv = (const float*)(a.vel + ra) + (j & 1);
    const double dt = (double)a.dt, c2 = dt * dt * 0.5, c3 = dt * dt * dt / 6.0;
    const unsigned int n = a.stride;
    const float ax = a.a0[j], ay = a.a0[n + j], az = a.a0[2u * n + j];
    const float jx = a.j0[j], jy = a.j0[n + j], jz = a.j0[2u * n + j];
    const float x = q[0], y = q[2], z = q[4 * MURB_TILE_PAIRS], u = qv[0], v = qv[2], w = qv[4 * MURB_TILE_PAIRS];
    a.src[2 * j] = make_float4(murb_hermite_predict_q(x, u, ax, jx, dt, c2, c3), murb_hermite_predict_q(y, v, ay, jy, dt, c2, c3),
                               murb_hermite_predict_q(z, w, az, jz, dt, c2, c3), q[4 * MURB_TILE_PAIRS + 2]);
    a.src[2 * j + 1] = make_float4(murb_hermite_predict_v(u, ax, jx, dt, c2), murb_hermite_predict_v(v, ay, jy, dt, c2),
                                   murb_hermite_predict_v(w, az, jz, dt, c2), 0.f);
}

struct MurbAcSweepArgs {
    const float4* src;          // two records per body: the sources AND the points
    const unsigned int* begin;  // per body: where its list starts in idx ...
    const unsigned int* len;    // ... and its length
    const int* idx;             // the resident entries: body indices in [0, n), produced by the fill sweep
    float* out;                 // ax | ay | az | jx | jy | jz | phi, out_stride floats each
    int count;                  // bodies
    unsigned int out_stride;
    float soft2;
};

// murb_list_sweep_kernel's walk and sums, lane step for lane step (murb_list_steps unchanged): 4 lane steps of gathers in flight
// where the list is that long, then 2, then 1.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void murb_ac_sweep_kernel(const MurbAcSweepArgs a)
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
    const float4 P = a.src[2 * (unsigned long)p], V = a.src[2 * (unsigned long)p + 1];
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

// What both correctors take: the Hermite corrector's arguments and the scheme's own planes, all of stride n.
struct MurbAcArgs {
    MurbHermiteArgs h;      // rec_in, rec_out, vel, a0, j0, acc_out, count, stride, dt; the regular kernel also part_a, part_j, nparts
    const float* f_cur;     // the sweep over the resident lists at the predicted state, seven planes: (aI1, jI1), or (aIo, jIo)
    const float* f_new;     // regular: the sweep over the new lists, (aIn, jIn)
    float* irr;             // aI (3 planes) | jI (3)
    float* reg;             // aR (3) | jR (3) | a2R (3) | a3R (3)
    unsigned int n;         // floats per plane of the four above
    int elapsed;            // irregular: m + 1; regular: n_irr
    int begin;              // regular: 1 = murbac_begin's form (the remembered evaluation in the rows' place, no update, no step)
};

// launch 3 of an irregular step.  One thread per pair of slots, like the Hermite corrector.
__global__ __launch_bounds__(256) void murb_ac_correct_kernel(const MurbAcArgs a)
{
#pragma clang fp contract(off)
    const int lp = blockIdx.x * blockDim.x + threadIdx.x;
    const int s0 = 2 * lp;
    if (s0 >= (int)a.h.stride) return;
    const double tau = murb_ac_elapsed(a.elapsed, a.h.dt);
    const unsigned int n = a.n, stride = a.h.stride;
    MurbHermiteForces f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const unsigned int s = (unsigned int)(s0 + h);
        const bool real = (int)s < a.h.count;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            f.a0[h][k] = f.j0[h][k] = f.a1[h][k] = f.j1[h][k] = 0.f;
            if (!real) continue;
            const unsigned int e = (unsigned int)k * n + s, at = (unsigned int)k * stride + s;
            const float aI1 = a.f_cur[e], jI1 = a.f_cur[3u * n + e];
            const float aR = a.reg[e], jR = a.reg[3u * n + e], a2R = a.reg[6u * n + e], a3R = a.reg[9u * n + e];
            const float a1 = aI1 + murb_ac_poly_a(aR, jR, a2R, a3R, tau);
            const float j1 = jI1 + murb_ac_poly_j(jR, a2R, a3R, tau);
            f.a0[h][k] = a.h.a0[at]; f.j0[h][k] = a.h.j0[at];
            f.a1[h][k] = a1; f.j1[h][k] = j1;
            a.h.a0[at] = a1; a.h.j0[at] = j1;
            a.h.acc_out[at] = a1;
            a.irr[e] = aI1; a.irr[3u * n + e] = jI1;
        }
    }
    murb_hermite_correct_pair(a.h, lp, f, a.h.dt);
}

// The last launch of a regular step (and, with `begin`, of murbac_begin).
__global__ __launch_bounds__(256) void murb_ac_regular_kernel(const MurbAcArgs a)
{
#pragma clang fp contract(off)
    const int lp = blockIdx.x * blockDim.x + threadIdx.x;
    const int s0 = 2 * lp;
    if (s0 >= (int)a.h.stride) return;
    const unsigned int n = a.n, stride = a.h.stride;
    const bool begin = a.begin != 0;
    MurbHermiteForces f = {};
    if (!begin) murb_hermite_sum_rows(a.h, s0, f);   // (a1, j1): the full sweep's rows in the Hermite step's order; (a0, j0) <- (a1, j1)
    const double T = murb_ac_elapsed(a.elapsed, a.h.dt);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const unsigned int s = (unsigned int)(s0 + h);
        if ((int)s >= a.h.count) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned int e = (unsigned int)k * n + s;
            float a1 = f.a1[h][k], j1 = f.j1[h][k], a2R = 0.f, a3R = 0.f;
            if (begin) {
                a1 = a.h.a0[(unsigned int)k * stride + s];
                j1 = a.h.j0[(unsigned int)k * stride + s];
            } else {
                const float A1 = a1 - a.f_cur[e], J1 = j1 - a.f_cur[3u * n + e];   // on the OLD list, like (aR, jR)
                murb_ac_derivatives(a.reg[e], a.reg[3u * n + e], A1, J1, T, a2R, a3R);
            }
            const float aIn = a.f_new[e], jIn = a.f_new[3u * n + e];
            a.reg[e] = a1 - aIn; a.reg[3u * n + e] = j1 - jIn;
            a.reg[6u * n + e] = a2R; a.reg[9u * n + e] = a3R;
            a.irr[e] = aIn; a.irr[3u * n + e] = jIn;
        }
    }
    if (!begin) murb_hermite_correct_pair(a.h, lp, f, a.h.dt);
}

#endif
