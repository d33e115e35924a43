// gfx950 (CDNA4) kernels of the Hermite integrator's shared adaptive step (murbhip_evolve): murb_kernels_hermite.h's sweep,
// predictor and corrector driven from a control block in device memory.  Device code only; included by murb_kernels_block.h.
#ifndef MURB_KERNELS_ADAPTIVE_H_
#define MURB_KERNELS_ADAPTIVE_H_

#include "murb_kernels_hermite.h"

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
    unsigned int enc_hits;          // bodies of the step just taken with r2 <= enc_thr ("nearest"): non-zero ends the run
    float enc_thr;                  // radius^2 + soft^2, or -1: no encounter stop
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
                                         const float dt_hi, const unsigned long long max_steps, const int fresh,
                                         const float enc_thr)
{
    c->enc_hits = 0u;
    c->enc_thr = enc_thr;
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
    if (was_last || c->steps >= c->max_steps || c->enc_hits) c->done = 1;
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

// The nearest-neighbour form of both launches (ctl null: the fixed-step one).  104+ vector registers: 4 waves per SIMD.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_nn_sweep_kernel(const MurbNNJerkArgs a, const MurbEvolveCtl* ctl)
{
    if (ctl && ctl->done) return;   // wave-uniform
    murb_force_jerk_sweep<R, WAVES, STAGE, MurbSide::Nearest, MurbNNJerkArgs>(a);
}

// The contact form of both launches (ctl null: the fixed-step one); 4 waves per SIMD like the nearest-neighbour form.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_contact_sweep_kernel(const MurbNNJerkArgs a, const MurbEvolveCtl* ctl)
{
    if (ctl && ctl->done) return;   // wave-uniform
    murb_force_jerk_sweep<R, WAVES, STAGE, MurbSide::Contact, MurbNNJerkArgs>(a);
}

// The potential form of both launches (ctl null: the fixed-step one).  R more packed accumulators: 4 waves per SIMD.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_force_jerk_pot_kernel(const MurbNNJerkArgs a, const MurbEvolveCtl* ctl)
{
    if (ctl && ctl->done) return;   // wave-uniform
    murb_force_jerk_sweep<R, WAVES, STAGE, MurbSide::Potential, MurbNNJerkArgs>(a);
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
        if (a.contact == 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (s0 + h < a.count) murb_side_test<MurbContactMetric>(&ctl->enc_hits, a.enc, 0.f, s0 + h, f.nn_r2[h], f.nn_idx[h]);
        } else if (a.nn_idx && !a.contact) {
            const float thr = ctl->enc_thr;
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (s0 + h < a.count) murb_side_test<MurbNearestMetric>(&ctl->enc_hits, a.enc, thr, s0 + h, f.nn_r2[h], f.nn_idx[h]);
        }
    }
    murb_evolve_fold_min(ctl, mine);
}

#endif
