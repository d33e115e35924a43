// gfx950 (CDNA4) kernels of the massless tracers (include/murbtracer.h has the definition).  Device code only; included by
// murb_ctx.h.
#ifndef MURB_KERNELS_TRACER_H_
#define MURB_KERNELS_TRACER_H_

#include "murb_kernels_adaptive.h"
#include "murb_kernels_field.h"
#include "murb_tracer.h"

// ---- massless tracers carried through Hermite steps --------------------------------------------------------------------
// A second, massless population resident beside the bodies: SoA planes q, v, (a0, j0), (a1, j1) of `stride` floats per
// component.  A step of the bodies carries them along, enqueue-only:
//     1  murb_tracer_predict_kernel   the predictor (murb_hermite_predict_q / _v), or a plain copy for an evaluation at the
//                                     current state, into one pair of records per tracer {x, y, z, 0} {u, v, w, 0}; the last
//                                     group of 16 is filled up with copies of its first tracer (murb_field_pack_kernel's rule)
//     2  murb_tracer_sweep_kernel     per launch of at most "tracer_batch" tracers: the field sweep without its extras
//     3  murb_tracer_rows_kernel      ... and its rows added in chunk order into (a1, j1), or (a0, j0) for an evaluation
//     4  murb_tracer_correct_kernel   the corrector (murb_hermite_correct_v / _q); (a0, j0) <- (a1, j1)
// dt is a launch argument (murbhip_step) or read from the control block of murbhip_evolve, whose `done` makes every one of the
// four a no-op.  The sweep reads the bodies' PREDICTED records and velocities, the ones the bodies' own sweep reads.
struct MurbTracerArgs {
    float* q;               // x | y | z, stride floats each
    float* v;
    float* a0;              // the remembered evaluation
    float* j0;
    float* a1;              // the sweep's evaluation of the step in flight
    float* j1;
    float4* pts;            // two records per tracer, whole groups
    int count;              // tracers
    int padded;             // ... rounded up to whole groups
    unsigned int stride;
    float dt;               // the fixed step (ctl null)
    int predict;            // predictor: 0 = the current state as it is
    int fold_dt;            // corrector under a control block: "tracer_dt" 1
};

struct MurbTracerSweepArgs {
    const float4* rec;      // the bodies' positions + GM the sweep is made at, all slots
    const float4* vel;      // ... and velocities (with "contact" on their B records carry radii in lanes z, w: never read)
    const float4* pts;      // two records per tracer of the launch
    float4* part_a;         // part_a[chunk * stride + tracer] = {ax, ay, az, 0}
    float4* part_j;         // ... {jx, jy, jz, 0}
    int groups, chunks;     // the launch's units
    int tiles;              // layout tiles swept as j (those that hold real bodies)
    unsigned int stride;    // entries per partial row: 16 * groups
    float soft2;
};

__global__ __launch_bounds__(256) void murb_tracer_predict_kernel(const MurbTracerArgs a, const MurbEvolveCtl* ctl)
{
#pragma clang fp contract(off)
    if (ctl && ctl->done) return;   // wave-uniform
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= a.padded) return;
    const int src = p < a.count ? p : p / MURB_FIELD_GROUP * MURB_FIELD_GROUP;   // the group's first tracer: < count
    const unsigned int n = a.stride;
    float x = a.q[src], y = a.q[n + src], z = a.q[2u * n + src];
    float u = a.v[src], v = a.v[n + src], w = a.v[2u * n + src];
    if (a.predict) {
        const double dt = (double)(ctl ? ctl->dt : a.dt), c2 = dt * dt * 0.5, c3 = dt * dt * dt / 6.0;
        const float ax = a.a0[src], ay = a.a0[n + src], az = a.a0[2u * n + src];
        const float jx = a.j0[src], jy = a.j0[n + src], jz = a.j0[2u * n + src];
        x = murb_hermite_predict_q(x, u, ax, jx, dt, c2, c3);
        y = murb_hermite_predict_q(y, v, ay, jy, dt, c2, c3);
        z = murb_hermite_predict_q(z, w, az, jz, dt, c2, c3);
        u = murb_hermite_predict_v(u, ax, jx, dt, c2);
        v = murb_hermite_predict_v(v, ay, jy, dt, c2);
        w = murb_hermite_predict_v(w, az, jz, dt, c2);
    }
    a.pts[2 * p] = make_float4(x, y, z, 0.f);
    a.pts[2 * p + 1] = make_float4(u, v, w, 0.f);
}

// launch 2.  murb_force_field_kernel's mapping and loop nest without the skip machinery and without phi: a workgroup takes a
// group of 16 tracers, 4 per wave, their 24 values wave-uniform in scalar registers, and walks units u = blockIdx.x,
// += gridDim.x with (group, chunk) = (u % groups, u / groups).  Per pair of interactions the plain Hermite sweep's 26 packed
// instructions and 2 v_rsq_f32; the fp32 sequence is the field kernel's with its multiplier 1 (G m_j * 1.0f is exact), so a
// tracer's (a, j) have the bits murbfield_at gives for the same point, velocity and no skipped body at the same chunk count.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_tracer_sweep_kernel(const MurbTracerSweepArgs a, const MurbEvolveCtl* ctl)
{
    static_assert(R % 2 == 0 && WAVES * R == MURB_FIELD_GROUP, "a workgroup takes one group of tracers");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
    __shared__ float4 lds[2 * STAGE * MURB_TILE_F4];
    if (ctl && ctl->done) return;   // wave-uniform, before anything else
    const float soft2 = a.soft2;

    // Through the inner loop the scalar registers hold the tracers' 24 values and the two record pointers.  Everything else of
    // the kernel's argument is read again where it is needed (murb_kernarg_again).
    for (int u = blockIdx.x;; u += (int)gridDim.x) {
        const auto* now = murb_kernarg_again<MurbTracerSweepArgs>();
        const int groups = now->groups, chunks = now->chunks, tiles = now->tiles;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63;
        const int i_first = (group * WAVES + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;   // tracer of the launch, wave-uniform

        float xi[R], yi[R], zi[R], ui[R], vi[R], wi[R];
        {
            const float4* const pts = now->pts;
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

        murb_f2 ax[R], ay[R], az[R], jx[R], jy[R], jz[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ax[r] = (murb_f2)(0.f); ay[r] = (murb_f2)(0.f); az[r] = (murb_f2)(0.f);
            jx[r] = (murb_f2)(0.f); jy[r] = (murb_f2)(0.f); jz[r] = (murb_f2)(0.f);
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
#pragma unroll
                for (int q = 0; q < MURB_TILE_PAIRS; q += 64) {
                    const float4 A = tq[q + lane], B = tq[q + lane + MURB_TILE_PAIRS];
                    const float4 VA = tv[q + lane], VB = tv[q + lane + MURB_TILE_PAIRS];
                    const murb_f2 xj = {A.x, A.y}, yj = {A.z, A.w}, zj = {B.x, B.y}, gj = {B.z, B.w};
                    const murb_f2 uj = {VA.x, VA.y}, vj = {VA.z, VA.w}, wj = {VB.x, VB.y};
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        murb_f2 r2, gi;
                        murb_interact_jerk_pk_gi(xj, yj, zj, gj, uj, vj, wj, xi[r], yi[r], zi[r], ui[r], vi[r], wi[r], soft2,
                                                 ax[r], ay[r], az[r], jx[r], jy[r], jz[r], r2, gi);
                    }
                }
            }
        }

        // fold the 64 lanes x 2 halves of every accumulator; lane r keeps tracer r's totals
        float oa[3] = {0.f, 0.f, 0.f}, oj[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float sx = murb_wave_sum(ax[r].x + ax[r].y), sy = murb_wave_sum(ay[r].x + ay[r].y), sz = murb_wave_sum(az[r].x + az[r].y);
            const float tx = murb_wave_sum(jx[r].x + jx[r].y), ty = murb_wave_sum(jy[r].x + jy[r].y), tz = murb_wave_sum(jz[r].x + jz[r].y);
            if (lane == r) { oa[0] = sx; oa[1] = sy; oa[2] = sz; oj[0] = tx; oj[1] = ty; oj[2] = tz; }
        }
        if (lane < R) {
            const auto* end = murb_kernarg_again<MurbTracerSweepArgs>();
            const unsigned long at = (unsigned long)chunk * end->stride + (unsigned long)i_first + lane;   // < chunks * 16 * groups
            end->part_a[at] = make_float4(oa[0], oa[1], oa[2], 0.f);
            end->part_j[at] = make_float4(oj[0], oj[1], oj[2], 0.f);
        }
    }
}

// launch 3: one thread per tracer of the launch (never one of the last group's copies).  fp32, chunks in ascending order.
// out_a / out_j: the planes of (a1, j1), or of (a0, j0) for an evaluation at the current state, already offset to the launch's
// first tracer.
__global__ __launch_bounds__(256) void murb_tracer_rows_kernel(const float4* part_a, const float4* part_j, float* out_a, float* out_j,
                                                               const int count, const int chunks, const unsigned int stride,
                                                               const unsigned int out_stride, const MurbEvolveCtl* ctl)
{
    if (ctl && ctl->done) return;   // wave-uniform
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= count) return;
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < chunks; ++c) {
        const float4 u = part_a[(unsigned long)c * stride + p];
        const float4 w = part_j[(unsigned long)c * stride + p];
        s[0] += u.x; s[1] += u.y; s[2] += u.z;
        s[3] += w.x; s[4] += w.y; s[5] += w.z;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_a[(unsigned long)k * out_stride + p] = s[k];
        out_j[(unsigned long)k * out_stride + p] = s[3 + k];
    }
}

// launch 4: one thread per tracer; the grid covers the tracers in whole workgroups of 256 (threads past `count` only take part
// in the fold).  Under a control block with "tracer_dt" 1 every tracer's Aarseth step enters the step-size minimum.
__global__ __launch_bounds__(256) void murb_tracer_correct_kernel(const MurbTracerArgs a, MurbEvolveCtl* ctl)
{
#pragma clang fp contract(off)
    if (ctl && ctl->done) return;   // wave-uniform: the tracers stay where the run ended
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    float mine = __builtin_inff();
    if (p < a.count) {
        const unsigned int n = a.stride;
        const float dt32 = ctl ? ctl->dt : a.dt;
        const double dt = (double)dt32, h2 = dt * 0.5, c12 = dt * dt / 12.0;
        float a0[3], j0[3], a1[3], j1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned int at = (unsigned int)k * n + p;
            a0[k] = a.a0[at]; j0[k] = a.j0[at]; a1[k] = a.a1[at]; j1[k] = a.j1[at];
            const float q = a.q[at], v = a.v[at];
            const float v1 = murb_hermite_correct_v(v, a0[k], a1[k], j0[k], j1[k], h2, c12);
            a.q[at] = murb_hermite_correct_q(q, v, v1, a0[k], a1[k], h2, c12);
            a.v[at] = v1;
            a.a0[at] = a1[k]; a.j0[at] = j1[k];
        }
        if (ctl && a.fold_dt) mine = murb_evolve_body_step(a0, j0, a1, j1, dt, ctl->eta);
    }
    if (ctl && a.fold_dt) murb_evolve_fold_min(ctl, mine);   // kernel-uniform
}

// "tracer_dt" 1, head of a murbhip_evolve call without a proposal: the tracers' eta_start |a0| / |j0| beside the bodies'
// (murb_evolve_first_kernel), between it and murb_evolve_start_kernel.
__global__ __launch_bounds__(256) void murb_tracer_first_kernel(const MurbTracerArgs a, MurbEvolveCtl* ctl, const double eta_start)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const unsigned int n = a.stride;
    float mine = __builtin_inff();
    if (p < a.count)
        mine = murb_evolve_body_first_step(a.a0[p], a.a0[n + p], a.a0[2u * n + p], a.j0[p], a.j0[n + p], a.j0[2u * n + p], eta_start);
    murb_evolve_fold_min(ctl, mine);
}

#endif
