// gfx950 (CDNA4) kernels of the Hermite integrator's individual block time steps (murbhip_evolve_block), and the two small
// kernels of the options "potential" and "contact".  Device code only; included by murb_ctx.h.
#ifndef MURB_KERNELS_BLOCK_H_
#define MURB_KERNELS_BLOCK_H_

#include "murb_kernels_adaptive.h"

// ---- individual block time steps (murbhip_evolve_block) --------------------------------------------------------------------
// Every body has its own step dt_max 2^-k (its level k in [0, kmax]) and its own time, counted in ticks of dt_max 2^-kmax
// inside the block of dt_max in flight (T = 2^kmax ticks; include/murbhip.h spells the scheme out).  A block step advances
// only the bodies whose next time is the earliest one — the active set — and sweeps those few i bodies against ALL bodies
// predicted to that time.  The host never learns how many they are: the set's size, the shape of the sweep made from it and
// the end of the run live in a control block, like murbhip_evolve's, and every launch has a size fixed by the host.
//     1  murb_block_min_kernel       t_next = min_i (t_i + (T >> k_i))                      (one atomicMin per workgroup)
//     2  murb_block_predict_kernel   every body -> herm_rec / herm_vel at t_next; the active ones also get a place in the
//                                    list (atomicAdd) and their predicted q, v in a compact buffer of the same pair layout
//     3  murb_block_plan_kernel      one thread: groups of 16 list entries, j chunks, row stride
//     4  murb_force_jerk_block_kernel  workgroups walk (group, chunk) units; rows part[chunk * stride + list index]
//     5  murb_block_correct_kernel   one thread per list entry: row sum in chunk order, corrector in place, criterion, level
//     6  murb_block_book_kernel      one thread: clock, counters, done, reset of t_next and the list length
// All on one stream.  Concurrent writers meet only in integer atomics (a minimum, a maximum, a count, a list position): a
// body's place in the list varies from run to run, its numbers do not — its sums depend on the j order and the chunk cut
// alone, and the cut on the SIZE of the list.
#define MURB_BLOCK_GROUP 16   // list entries per workgroup of the sweep (4 waves x 4 i bodies)

struct MurbBlockCtl {
    double tick_sec;                 // (double)dt_max * 2^-kmax: seconds = (double)ticks * tick_sec, exact for kmax <= 20
    double eta;
    unsigned long long ticks_done;   // model time advanced in this call, in ticks
    unsigned long long steps, max_steps, body_steps;
    float dt_max;
    int kmax;
    unsigned int T;                  // ticks per block, 2^kmax
    unsigned int clock;              // time of the last block step inside the block in flight, [0, T); 0 = synchronised
    unsigned int blocks_left;
    unsigned int t_next;             // step in flight: its time (running minimum of launch 1; ~0u between steps)
    unsigned int n_act;              // ... length of the active list
    int groups, chunks;              // ... the sweep's units
    unsigned int stride;             // ... entries per partial row, 16 * groups
    int units, tiles;                // "block_units", layout tiles swept as j
    unsigned int row_cap;            // entries a partial-row buffer holds
    unsigned int clamped;            // steps whose criterion asked for less than dt_max 2^-kmax
    unsigned int max_act;
    unsigned int k_lo, k_hi;         // smallest and largest level a step of this call was taken at
    int done;
    // the i side and the rows of the active sweep, which reads them here once per unit instead of holding four more pointers
    // in scalar registers through its inner loop
    const float4* rec_act;
    const float4* vel_act;
    float4* part_a;
    float4* part_j;
    // "nearest"
    const int* list;                 // the active list, where the nearest-neighbour sweep finds its i bodies' slots
    unsigned int enc_hits;           // active bodies of the step just taken with r2 <= enc_thr: non-zero ends the run
    float enc_thr;                   // radius^2 + soft^2, or -1: no encounter stop
};

struct MurbBlockArgs {
    float4* rec;           // current positions + GM: the corrector updates active bodies in place
    float4* vel;
    float4* rec_pred;      // every body predicted to t_next (herm_rec / herm_vel): the j side of the sweep
    float4* vel_pred;
    float4* rec_act;       // predicted q, v of the active bodies by list index, pair layout: the i side
    float4* vel_act;
    float* a0;             // remembered evaluation of every body at its own time
    float* j0;
    float* acc_out;
    float4* part_a;        // partial rows
    float4* part_j;
    unsigned int* ticks;   // t_i
    int* levels;           // k_i
    int* list;             // active bodies, unordered
    int* nn_idx;           // "nearest": every body's nearest neighbour and its r2 at its own time; null = off
    float* nn_r2;
    MurbEncList* enc;
    int count;
    unsigned int stride;   // slots
    float soft2;
    int contact;           // "contact": see MurbHermiteArgs
    float* phi;            // "potential": every body's potential at its own time; null = off
};

// what the active sweep holds of it through its inner loop
struct MurbBlockSweepArgs {
    const float4* rec_pred;
    const float4* vel_pred;
    float soft2;
};

struct MurbBlockNNSweepArgs : MurbBlockSweepArgs {
    int count;                  // real bodies: slots >= count are padding
    int grid;                   // workgroups of the launch
    const MurbBlockCtl* ctl;    // the control block once more: the sweep reads both here, once per unit (murb_kernarg_again)
};

// dt_max 2^-k: exact while the result is a normal number
__device__ __forceinline__ float murb_block_dt(const float dt_max, const int k)
{
    return dt_max * __builtin_bit_cast(float, (unsigned int)(127 - k) << 23);
}

// smallest k in [0, kmax] with dt_max 2^-k <= req (+inf: 0); none: kmax, and the step counts as clamped
__device__ __forceinline__ int murb_block_level_of(const float req, const float dt_max, const int kmax, bool& clamped)
{
    clamped = false;
    for (int k = 0; k <= kmax; ++k)
        if (murb_block_dt(dt_max, k) <= req) return k;
    clamped = true;
    return kmax;
}

// the level after a step that ended at t_next: any number of halvings, one doubling where the coarser grid has a point
__device__ __forceinline__ int murb_block_new_level(const int k, const int k_req, const unsigned int t_next, const unsigned int T)
{
    if (k_req > k) return k_req;
    if (k_req < k && t_next % (2u * (T >> k)) == 0u) return k - 1;
    return k;
}

// one float of a body's place in the pair layout: c = 0, 1, 2 for x, y, z
__device__ __forceinline__ float* murb_block_slot(float4* recs, const unsigned int slot, const int c)
{
    float* const base = (float*)(recs + murb_rec_a((unsigned long)(slot >> 1)) + (c == 2 ? MURB_TILE_PAIRS : 0));
    return base + (c == 1 ? 2 : 0) + (slot & 1u);
}

// Head of a call, one thread.  `resume`: a block is open, the clock and the bodies' ticks and levels go on.
__global__ void murb_block_begin_kernel(MurbBlockCtl* c, const MurbBlockArgs a, const float dt_max, const int kmax, const double eta, const unsigned int blocks,
                                        const unsigned long long max_steps, const int units, const int tiles,
                                        const unsigned int row_cap, const int resume, const float enc_thr)
{
    c->list = a.list;
    c->enc_hits = 0u;
    c->enc_thr = enc_thr;
    c->tick_sec = (double)dt_max * (double)murb_block_dt(1.f, kmax);
    c->eta = eta;
    c->ticks_done = 0;
    c->steps = 0;
    c->max_steps = max_steps;
    c->body_steps = 0;
    c->dt_max = dt_max;
    c->kmax = kmax;
    c->T = 1u << kmax;
    if (!resume) c->clock = 0u;
    c->blocks_left = blocks;
    c->t_next = ~0u;
    c->n_act = 0u;
    c->groups = 0; c->chunks = 1; c->stride = 0u;
    c->units = units;
    c->tiles = tiles;
    c->row_cap = row_cap;
    c->clamped = 0u;
    c->max_act = 0u;
    c->k_lo = ~0u;
    c->k_hi = 0u;
    c->done = 0;
    c->rec_act = a.rec_act;
    c->vel_act = a.vel_act;
    c->part_a = a.part_a;
    c->part_j = a.part_j;
}

// Starting levels from the remembered evaluation: the level of eta_start |a0| / |j0|; all bodies at tick 0.
__global__ __launch_bounds__(256) void murb_block_start_kernel(const MurbBlockArgs a, const MurbBlockCtl* ctl, const double eta_start)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.count) return;
    const unsigned int n = a.stride;
    const float req = murb_evolve_body_first_step(a.a0[s], a.a0[n + s], a.a0[2u * n + s], a.j0[s], a.j0[n + s], a.j0[2u * n + s], eta_start);
    bool clamped;
    a.levels[s] = murb_block_level_of(req, ctl->dt_max, ctl->kmax, clamped);
    a.ticks[s] = 0u;
}

// launch 1
__global__ __launch_bounds__(256) void murb_block_min_kernel(const MurbBlockArgs a, MurbBlockCtl* ctl)
{
    if (ctl->done) return;
    __shared__ unsigned int wave_min[4];
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int mine = ~0u;
    if (s < a.count) mine = a.ticks[s] + (ctl->T >> a.levels[s]);
    const unsigned int m = murb_wave_min_bits(__builtin_bit_cast(float, mine));   // an unsigned minimum of the bits, whatever they mean
    if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int lo = wave_min[0] < wave_min[1] ? wave_min[0] : wave_min[1];
        const unsigned int hi = wave_min[2] < wave_min[3] ? wave_min[2] : wave_min[3];
        atomicMin(&ctl->t_next, lo < hi ? lo : hi);
    }
}

// launch 2: one thread per pair of slots, like murb_hermite_predict_pair, but every body with its own dt = t_next - t_i
__global__ __launch_bounds__(256) void murb_block_predict_kernel(const MurbBlockArgs a, MurbBlockCtl* ctl)
{
#pragma clang fp contract(off)
    if (ctl->done) return;
    const int lp = blockIdx.x * blockDim.x + threadIdx.x;
    const int s0 = 2 * lp;
    const unsigned int n = a.stride;
    if (s0 >= (int)n) return;
    const unsigned long ra = murb_rec_a((unsigned long)lp);
    const float4 A = a.rec[ra], B = a.rec[ra + MURB_TILE_PAIRS];
    const float4 VA = a.vel[ra], VB = a.vel[ra + MURB_TILE_PAIRS];
    float q[2][3] = {{A.x, A.z, B.x}, {A.y, A.w, B.y}}, v[2][3] = {{VA.x, VA.z, VB.x}, {VA.y, VA.w, VB.y}};
    const unsigned int t_next = ctl->t_next, T = ctl->T;
    const double tick = ctl->tick_sec;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = s0 + h;
        if (s >= a.count) continue;
        const unsigned int t = a.ticks[s];
        const double dt = (double)(t_next - t) * tick, c2 = dt * dt * 0.5, c3 = dt * dt * dt / 6.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float ak = a.a0[(unsigned int)k * n + s], jk = a.j0[(unsigned int)k * n + s];
            const float qk = q[h][k], vk = v[h][k];
            q[h][k] = murb_hermite_predict_q(qk, vk, ak, jk, dt, c2, c3);
            v[h][k] = murb_hermite_predict_v(vk, ak, jk, dt, c2);
        }
        if (t + (T >> a.levels[s]) == t_next) {
            const unsigned int at = atomicAdd(&ctl->n_act, 1u);   // at < count <= slots
            a.list[at] = s;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                *murb_block_slot(a.rec_act, at, k) = q[h][k];
                *murb_block_slot(a.vel_act, at, k) = v[h][k];
            }
            if (a.contact) murb_block_slot(a.vel_act, at, 2)[2] = h ? VB.w : VB.z;   // the radius: the active sweep's i side reads it there
        }
    }
    a.rec_pred[ra] = make_float4(q[0][0], q[1][0], q[0][1], q[1][1]);
    a.rec_pred[ra + MURB_TILE_PAIRS] = make_float4(q[0][2], q[1][2], B.z, B.w);
    a.vel_pred[ra] = make_float4(v[0][0], v[1][0], v[0][1], v[1][1]);
    a.vel_pred[ra + MURB_TILE_PAIRS] = make_float4(v[0][2], v[1][2], VB.z, VB.w);
}

// launch 3, one thread: `units` (group, chunk) units at least, where the layout has the tiles for it
__global__ void murb_block_plan_kernel(MurbBlockCtl* c)
{
    if (c->done) return;
    const int groups = (int)((c->n_act + MURB_BLOCK_GROUP - 1) / MURB_BLOCK_GROUP);
    int chunks = groups > 0 ? (c->units + groups - 1) / groups : 1;
    chunks = chunks < 1 ? 1 : (chunks > c->tiles ? c->tiles : chunks);
    while (chunks > 1 && (unsigned long)groups * chunks * MURB_BLOCK_GROUP > c->row_cap) --chunks;   // never taken: the host sizes the rows
    c->groups = groups;
    c->chunks = chunks;
    c->stride = (unsigned int)groups * MURB_BLOCK_GROUP;
}

// The control block as the sweep reads it once per unit.  No launch writes it while the sweep runs, so the loads may go
// through the scalar cache (constant address space) like the `done` test of every launch here; the empty asm makes the
// pointer a new value to the compiler in every iteration, so that it does not move the loads in front of the loop and hold
// their results in scalar registers through the inner loop, where the i bodies need them.
typedef const __attribute__((address_space(4))) MurbBlockCtl* MurbBlockCtlK;
typedef const __attribute__((address_space(4))) float4* MurbF4K;
__device__ __forceinline__ MurbBlockCtlK murb_block_ctl_now(const MurbBlockCtl* ctl)
{
    unsigned long p = (unsigned long)ctl;
    asm volatile("" : "+s"(p));
    return (MurbBlockCtlK)p;
}

// launch 4.  murb_force_jerk_sweep's mapping and inner loop; the i bodies come from the compact buffer, and the workgroup
// walks units u = blockIdx.x, += gridDim.x with (group, chunk) = (u % groups, u / groups).  The entries behind the list's
// end in its last group are whatever the buffer held: their rows are never read.
// The body is a device function with the side-product forms behind a compile-time switch (SIDE; NN, Args =
// MurbBlockNNSweepArgs), like murb_force_jerk_sweep: the plain form's code does not change.
template <int R, int WAVES, int STAGE, MurbSide SIDE = MurbSide::None, typename Args = MurbBlockSweepArgs>
__device__ __forceinline__ void murb_force_jerk_block_sweep(const Args a, const MurbBlockCtl* ctl)  // NN: a is the kernel's first argument
{
    constexpr bool NN = SIDE != MurbSide::None, CT = SIDE == MurbSide::Contact, POT = SIDE == MurbSide::Potential;   // as in murb_force_jerk_sweep
    static_assert(R % 2 == 0 && WAVES * R == MURB_BLOCK_GROUP, "a workgroup takes one group of the list");
    static_assert(MURB_TILE_F4 % (WAVES * 64) == 0, "the workgroup copies a tile in whole rounds");
#if defined(__HIP_DEVICE_COMPILE__)   // the host pass knows no constant address space to read through
    if (ctl->done) return;   // one wave-uniform load, before anything else
    __shared__ float4 lds[2 * STAGE * MURB_TILE_F4];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float soft2 = a.soft2;

    int stride_u = 0;
    for (int u = blockIdx.x;; u += NN ? stride_u : (int)gridDim.x) {
        if constexpr (NN) {   // the scalar registers are taken: the stride and the control block from the kernel arguments, per unit
            const auto* again = murb_kernarg_again<Args>();
            if constexpr (!CT) stride_u = again->grid;   // the contact form reads it at the unit's end: one scalar register less
            ctl = again->ctl;
        }
        const MurbBlockCtlK now = murb_block_ctl_now(ctl);
        const int groups = now->groups, chunks = now->chunks, tiles = now->tiles;
        if (u >= groups * chunks) break;   // workgroup-uniform
        const int chunk = u / groups, group = u - chunk * groups;
        int wave_now = wave;
        if constexpr (NN) {   // made in every unit, like the fold's lane below: the scalar registers are taken
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            wave_now = __builtin_amdgcn_readfirstlane(tid >> 6);
        }
        const int i_slot = (group * WAVES + wave_now) * R;   // list index, wave-uniform

        float xi[R], yi[R], zi[R], ui[R], vi[R], wi[R], ri[R];   // ri: the contact form's radii
        {
            const unsigned long ra = murb_rec_a((unsigned long)(i_slot >> 1));
            // written by the launch before this one and wave-uniform: scalar loads, straight into scalar registers
            const MurbF4K rec_act = (MurbF4K)(unsigned long)now->rec_act, vel_act = (MurbF4K)(unsigned long)now->vel_act;
#pragma unroll
            for (int h = 0; h < R / 2; ++h) {
                const float4 A = rec_act[ra + h], B = rec_act[ra + h + MURB_TILE_PAIRS];
                const float4 VA = vel_act[ra + h], VB = vel_act[ra + h + MURB_TILE_PAIRS];
                xi[2 * h] = A.x; xi[2 * h + 1] = A.y; yi[2 * h] = A.z; yi[2 * h + 1] = A.w; zi[2 * h] = B.x; zi[2 * h + 1] = B.y;
                ui[2 * h] = VA.x; ui[2 * h + 1] = VA.y; vi[2 * h] = VA.z; vi[2 * h + 1] = VA.w; wi[2 * h] = VB.x; wi[2 * h + 1] = VB.y;
                if constexpr (CT) {   // to vector registers: no scalar one is free
                    ri[2 * h] = VB.z; ri[2 * h + 1] = VB.w;
                    asm volatile("" : "+v"(ri[2 * h]), "+v"(ri[2 * h + 1]));
                }
            }
        }
        float mn[R];   // NN: the lane's smallest r2 per i body, and the lane step it fell at
        int st[R];
        // NN: the i bodies' slots in lanes 0 .. R - 1 of ONE vector register and the body count in lane R, read out lane by lane
        // where they are needed: the scalar registers are taken (an entry behind the list's end is a slot of an earlier step or 0,
        // its row is never read)
        int who = 0;
        if constexpr (NN) {
            int l = threadIdx.x & 63;
            asm volatile("" : "+v"(l));
            const int slot = ((const int*)now->list)[i_slot + (l & (R - 1))];
            who = l < R ? slot : murb_kernarg_again<Args>()->count;   // `a` is the kernel's first argument
#pragma unroll
            for (int r = 0; r < R; ++r) { mn[r] = __builtin_inff(); st[r] = 0; }
        }

        const int vt0 = (int)(((long)tiles * chunk) / chunks);
        const int vt1 = (int)(((long)tiles * (chunk + 1)) / chunks);

        murb_f2 ax[R], ay[R], az[R], jx[R], jy[R], jz[R], ph[R];   // ph: POT, the sums of GM_j * inv
        {
            float z = 0.f;   // made in every iteration, like the fold's below
            asm volatile("" : "+v"(z));
#pragma unroll
            for (int r = 0; r < R; ++r) {
                ax[r] = (murb_f2)(z); ay[r] = (murb_f2)(z); az[r] = (murb_f2)(z);
                jx[r] = (murb_f2)(z); jy[r] = (murb_f2)(z); jz[r] = (murb_f2)(z);
                if constexpr (POT) ph[r] = (murb_f2)(z);
            }
        }

        for (int vs = vt0; vs < vt1; vs += STAGE) {
            const int nt = (vt1 - vs) < STAGE ? (vt1 - vs) : STAGE;
            __syncthreads();   // previous stage (of this unit or the one before) fully consumed
            // The thread's index as a new value in every stage (the empty asm hides that it never changes): the copy's and the
            // reads' addresses are then made from it here instead of four of them being held through the inner loop from
            // in front of the unit loop, and the sweep fits the 96 vector registers of murb_force_jerk_sweep.
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const int lane = tid & 63;
            for (int t = 0; t < nt; ++t) {
                const float4* srcq = a.rec_pred + (unsigned long)(vs + t) * MURB_TILE_F4;
                const float4* srcv = a.vel_pred + (unsigned long)(vs + t) * MURB_TILE_F4;
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
                int w = who, self_tile[R], count = 0;   // NN: the bodies' tiles (they can lie in R different ones) and the body count
                if constexpr (NN) {
                    asm volatile("" : "+v"(w));   // read out here, in every tile
#pragma unroll
                    for (int r = 0; r < R; ++r) self_tile[r] = __builtin_amdgcn_readlane(w, r) / MURB_TILE_BODIES;
                }
                const int tile = vs + t;
                if constexpr (NN && !POT) count = __builtin_amdgcn_readlane(w, R);
                murb_sweep_tile<R, SIDE, R>(tq, tv, lane, tile, self_tile, count, xi, yi, zi, ui, vi, wi, ri, soft2, ax, ay, az, jx, jy, jz, mn, st, ph);
            }
        }

        // The fold's zero and lane tests are made here, in every iteration (the empty asm hides that they never change): moved
        // in front of the unit loop they would hold a vector register and ten scalar ones through the inner loop.
        float zero = 0.f;
        int fold_lane = threadIdx.x & 63;
        asm volatile("" : "+v"(zero), "+v"(fold_lane));
        float oa[3] = {zero, zero, zero}, oj[3] = {zero, zero, zero};
        float nn_a = zero, nn_j = zero;   // the rows' fourth floats
        if constexpr (NN) {
            int w = who, self[R], self_tile[R];
            const float4* rec_pred = a.rec_pred;
            asm volatile("" : "+v"(w), "+s"(rec_pred));   // no address made from the pointer in front of the unit loop
#pragma unroll
            for (int r = 0; r < R; ++r) { self[r] = __builtin_amdgcn_readlane(w, r); self_tile[r] = self[r] / MURB_TILE_BODIES; }
            const int count = __builtin_amdgcn_readlane(w, R);
            unsigned int nn_r2 = 0u, nn_idx = 0u;
            if constexpr (POT) {
                for (int tile = vt0; tile < vt1; ++tile)
                    if (murb_pot_tile_own<R>(tile, self_tile)) murb_pot_own_tile<R, true>(rec_pred, fold_lane, tile, xi, yi, zi, soft2, ph, self);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float sp = murb_wave_sum(ph[r].x + ph[r].y);
                    if (fold_lane == r) nn_r2 = __builtin_bit_cast(unsigned int, sp);   // part_j.w stays 0
                }
            } else if constexpr (CT) {
                const float4* vel_pred = a.vel_pred;
                asm volatile("" : "+s"(vel_pred));
                for (int tile = vt0; tile < vt1; ++tile)
                    if (murb_nn_tile_masked<R>(tile, self_tile, count))
                        murb_side_masked_tile<R, MurbContactMetric>(rec_pred, vel_pred, fold_lane, tile, xi, yi, zi, ri, soft2, mn, st, self, count);
                murb_side_finish<R, MurbContactMetric>(rec_pred, vel_pred, fold_lane, xi, yi, zi, ri, soft2, mn, st, self, count, nn_r2, nn_idx);
            } else {   // an arm of its own: written as one call over the metric, like murb_force_jerk_sweep's, this form's register allocation moves
                for (int tile = vt0; tile < vt1; ++tile)
                    if (murb_nn_tile_masked<R>(tile, self_tile, count))
                        murb_side_masked_tile<R, MurbNearestMetric>(rec_pred, nullptr, fold_lane, tile, xi, yi, zi, ri, soft2, mn, st, self, count);
                murb_side_finish<R, MurbNearestMetric>(rec_pred, nullptr, fold_lane, xi, yi, zi, ri, soft2, mn, st, self, count, nn_r2, nn_idx);
            }
            nn_a = __builtin_bit_cast(float, nn_r2);
            nn_j = __builtin_bit_cast(float, nn_idx);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float sx = murb_wave_sum(ax[r].x + ax[r].y), sy = murb_wave_sum(ay[r].x + ay[r].y), sz = murb_wave_sum(az[r].x + az[r].y);
            const float tx = murb_wave_sum(jx[r].x + jx[r].y), ty = murb_wave_sum(jy[r].x + jy[r].y), tz = murb_wave_sum(jz[r].x + jz[r].y);
            if (fold_lane == r) { oa[0] = sx; oa[1] = sy; oa[2] = sz; oj[0] = tx; oj[1] = ty; oj[2] = tz; }
        }
        if (fold_lane < R) {
            const MurbBlockCtlK end = murb_block_ctl_now(ctl);
            const unsigned long at = (unsigned long)chunk * end->stride + (unsigned long)i_slot + fold_lane;   // < groups * chunks * 16 <= row_cap
            end->part_a[at] = make_float4(oa[0], oa[1], oa[2], nn_a);
            end->part_j[at] = make_float4(oj[0], oj[1], oj[2], nn_j);
        }
        if constexpr (CT) stride_u = murb_kernarg_again<Args>()->grid;
    }
#else
    (void)a; (void)ctl; (void)NN; (void)CT; (void)POT;
#endif
}

template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(5))) void murb_force_jerk_block_kernel(const MurbBlockSweepArgs a, const MurbBlockCtl* ctl)
{
    murb_force_jerk_block_sweep<R, WAVES, STAGE>(a, ctl);
}

// The nearest-neighbour form.  104+ vector registers: 4 waves per SIMD, so the host launches 4 workgroups per CU.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_nn_active_sweep_kernel(const MurbBlockNNSweepArgs a, const MurbBlockCtl* ctl)
{
    murb_force_jerk_block_sweep<R, WAVES, STAGE, MurbSide::Nearest, MurbBlockNNSweepArgs>(a, ctl);
}

// The contact form: the i bodies' radii come from the compact velocity buffer, where the block predictor puts them.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_contact_active_sweep_kernel(const MurbBlockNNSweepArgs a, const MurbBlockCtl* ctl)
{
    murb_force_jerk_block_sweep<R, WAVES, STAGE, MurbSide::Contact, MurbBlockNNSweepArgs>(a, ctl);
}

// The potential form: the i bodies' slots come from the list, like the nearest-neighbour form's.
template <int R, int WAVES, int STAGE>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void murb_force_jerk_pot_block_kernel(const MurbBlockNNSweepArgs a, const MurbBlockCtl* ctl)
{
    murb_force_jerk_block_sweep<R, WAVES, STAGE, MurbSide::Potential, MurbBlockNNSweepArgs>(a, ctl);
}

// launch 5: one thread per list entry.  The grid covers `count` entries; threads behind the list's end only take part in the
// wave folds.
__global__ __launch_bounds__(256) void murb_block_correct_kernel(const MurbBlockArgs a, MurbBlockCtl* ctl)
{
#pragma clang fp contract(off)
    if (ctl->done) return;
    const unsigned int at = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned int n_act = ctl->n_act;
    if ((at & ~63u) >= n_act) return;   // the whole wave is behind the list's end
    const bool live = at < n_act;
    unsigned int k_used = ~0u, k_used_inv = ~0u;
    bool clamped = false;
    if (live) {
        const unsigned int n = a.stride, stride = ctl->stride, t_next = ctl->t_next, T = ctl->T;
        const int chunks = ctl->chunks, kmax = ctl->kmax;
        const float dt_max = ctl->dt_max;
        const int s = a.list[at];
        const int k = a.levels[s];
        float a0[3], j0[3], a1[3] = {0.f, 0.f, 0.f}, j1[3] = {0.f, 0.f, 0.f};
        unsigned int nn_r2 = a.contact ? MurbContactMetric::key(__builtin_inff()) : MurbNearestMetric::key(__builtin_inff()), nn_idx = MURB_NN_NONE;
        float ph = 0.f;
        for (int p = 0; p < chunks; ++p) {
            const float4 u = a.part_a[(unsigned long)p * stride + at];
            const float4 w = a.part_j[(unsigned long)p * stride + at];
            a1[0] += u.x; a1[1] += u.y; a1[2] += u.z;
            j1[0] += w.x; j1[1] += w.y; j1[2] += w.z;
            if (a.phi) ph += u.w;
            murb_nn_fold_row(nn_r2, nn_idx, u, w);
        }
        if (a.phi) a.phi[s] = ph;
        if (a.contact) {
            murb_side_store<MurbContactMetric>(a.nn_idx, a.nn_r2, s, nn_r2, nn_idx);
            if (a.contact == 2) murb_side_test<MurbContactMetric>(&ctl->enc_hits, a.enc, 0.f, s, nn_r2, nn_idx);
        } else if (a.nn_idx) {
            murb_side_store<MurbNearestMetric>(a.nn_idx, a.nn_r2, s, nn_r2, nn_idx);
            murb_side_test<MurbNearestMetric>(&ctl->enc_hits, a.enc, ctl->enc_thr, s, nn_r2, nn_idx);
        }
        const float dt32 = murb_block_dt(dt_max, k);
        const double dt = (double)dt32, h2 = dt * 0.5, c12 = dt * dt / 12.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned int pl = (unsigned int)c * n + s;
            a0[c] = a.a0[pl]; j0[c] = a.j0[pl];
            a.a0[pl] = a1[c]; a.j0[pl] = j1[c]; a.acc_out[pl] = a1[c];
            float* const qp = murb_block_slot(a.rec, (unsigned int)s, c);
            float* const vp = murb_block_slot(a.vel, (unsigned int)s, c);
            const float v0 = *vp;
            const float v1 = murb_hermite_correct_v(v0, a0[c], a1[c], j0[c], j1[c], h2, c12);
            *qp = murb_hermite_correct_q(*qp, v0, v1, a0[c], a1[c], h2, c12);
            *vp = v1;
        }
        const float req = murb_evolve_body_step(a0, j0, a1, j1, dt, ctl->eta);
        const int k_req = murb_block_level_of(req, dt_max, kmax, clamped);
        a.levels[s] = murb_block_new_level(k, k_req, t_next, T);
        a.ticks[s] = t_next == T ? 0u : t_next;
        k_used = (unsigned int)k;
        k_used_inv = (unsigned int)(kmax - k);
    }
    const unsigned int lo = murb_wave_min_bits(__builtin_bit_cast(float, k_used));
    const unsigned int hi_inv = murb_wave_min_bits(__builtin_bit_cast(float, k_used_inv));
    const unsigned int nclamped = (unsigned int)__builtin_popcountll(__ballot(clamped));
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&ctl->k_lo, lo);
        atomicMax(&ctl->k_hi, (unsigned int)ctl->kmax - hi_inv);
        if (nclamped) atomicAdd(&ctl->clamped, nclamped);
    }
}

// murbhip_potential_energy: -1/2 m_i phi_i per real body in fp64, block sums in murb_metrics_kernel's fixed order (wave shuffle
// tree, then the 4 waves through LDS); the host adds the block rows in index order.  One block = 256 consecutive slots.
__global__ __launch_bounds__(256) void murb_potential_sum_kernel(const float* mass, const float* phi, double* out, const int count)
{
#pragma clang fp contract(off)
    __shared__ double red[3];
    const int s = blockIdx.x * 256 + threadIdx.x;
    double v = s < count ? -0.5 * (double)mass[s] * (double)phi[s] : 0.0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0 && wave > 0) red[wave - 1] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((v + red[0]) + red[1]) + red[2];
}

// The radii in the velocity records ("contact"): lanes z, w of a pair's B record = {R0, R1}; radius null: 0 in both (option
// off, or no radii set yet), as in the padding slots.  One thread per pair of slots.
__global__ __launch_bounds__(256) void murb_radii_lanes_kernel(float4* vel, const float* radius, const int count, const unsigned int slots)
{
    const unsigned int lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (2u * lp >= slots) return;
    const int s0 = (int)(2u * lp);
    float* const b = (float*)(vel + murb_rec_a((unsigned long)lp) + MURB_TILE_PAIRS);
    b[2] = radius && s0 < count ? radius[s0] : 0.f;
    b[3] = radius && s0 + 1 < count ? radius[s0 + 1] : 0.f;
}

// launch 6, one thread: the step in flight has been taken
__global__ void murb_block_book_kernel(MurbBlockCtl* c)
{
    if (c->done) return;
    const unsigned int t_next = c->t_next, n_act = c->n_act;
    c->ticks_done += (unsigned long long)(t_next - c->clock);
    c->steps += 1;
    c->body_steps += n_act;
    c->max_act = n_act > c->max_act ? n_act : c->max_act;
    if (t_next == c->T) {
        c->clock = 0u;
        c->blocks_left -= 1u;
    } else {
        c->clock = t_next;
    }
    c->t_next = ~0u;
    c->n_act = 0u;
    if (c->blocks_left == 0u || c->steps >= c->max_steps || c->enc_hits) c->done = 1;
}

#endif
