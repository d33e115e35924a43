// libmurbhip.so — the C ABI of include/murbhip.h: residency, launches, exchange.
// The only translation unit of the product that needs hipcc.  Its host code that needs no device lives in headers a plain
// C++ compiler can check: the plan choice (murb_choose.h), the tables of the pair-symmetric launches (murb_plan.h,
// murb_schedule.h), the shards' threads (murb_crew.h); the context and the counted allocations are in murb_ctx.h.
//
// Design notes (full text in DESIGN.md):
//   * body state stays resident in HBM for the whole simulation (reference twin:
//     CUDABodies, src/common/core/CUDABodies.cu:12-49); the only per-iteration host work is
//     enqueueing 2-3 kernels;
//   * positions are double-buffered: a step reads rec[cur] and the integrate kernel writes
//     rec[cur^1], so no kernel ever reads a buffer another kernel (or a peer GPU) is writing;
//   * force kernels: the pair-symmetric kernel (murb_kernels_sym.h; every body pair once, both
//     directions) wherever a GPU gets enough block pairs, the one-sided kernel (murb_kernels.h)
//     otherwise; make_plan() (murb_choose.h) decides, "variant"/"jsplit" override;
//   * multi-GPU: bodies are block-partitioned (murbhip_partition) into equal block-aligned slot
//     ranges of one replicated record buffer.  Half-ring schedule (sym_schedule_items): every pair is
//     evaluated by exactly one rank, ONE reduce-scatter returns each rank the accelerations of its own
//     bodies, ONE in-place all-gather publishes the integrated slice; both run on a second,
//     high-priority stream (RCCL, bound lazily with dlopen, or peer copies/peer reads inside one
//     process) under the two halves of the own-slice triangle (shard_iteration_sym_multi);
//   * one process driving several GPUs (murbhip_create_sharded, `--im hip+tile+multi`): the caller stays single-threaded
//     (reference contract, main.cpp:348-354), but every shard has a host thread of its own inside this library
//     (ShardCrew) that enqueues its device's share of a step — 100-140 us of HIP calls per shard and step, which one
//     thread would serialise to more than the 0.9 ms a rank of 8 computes at N = 200 000
//     (profiles/r03_host_enqueue.txt).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/murbhip.h"
#include "../../include/murbfield.h"
#include "../../include/murbtidal.h"
#include "../../include/murbbind.h"
#include "../../include/murbbound.h"
#include "../../include/murbknn.h"
#include "../../include/murbmst.h"
#include "../../include/murbnbr.h"
#include "../../include/murblist.h"
#include "../../include/murbac.h"
#include "../../include/murbsep.h"
#include "../../include/murbtracer.h"
#include "murb_init.h"
#include "murb_ctx.h"
#include "murb_mst.h"

namespace {

constexpr int kPotentialKernel = 100;   // not a selectable variant: murbhip_energy's potential sweep

// "solo_shard" timing aid: every shard but one stays completely idle
inline bool is_idle(const murbhip_ctx* c, const Shard& sh) { return c->solo_shard >= 0 && sh.rank != c->solo_shard; }

template <int MODE, int R, int WAVES, int STAGE>
int launch_force_t(const MurbForceArgs& a, int i_slots, hipStream_t s)
{
    const dim3 grid((unsigned)((i_slots + WAVES * R - 1) / (WAVES * R)), (unsigned)a.nchunks, 1);
    hipLaunchKernelGGL((murb_force_kernel<MODE, R, WAVES, STAGE>), grid, dim3(WAVES * 64), 0, s, a);
    return hip_rc(hipGetLastError());
}

// variant table: id -> (mode, R).  Keep in sync with DESIGN.md 4.1 (tools/ab.py and tools/sweep.py select them by id).
int launch_force(int variant, const MurbForceArgs& a, int i_slots, hipStream_t s)
{
    switch (variant) {
        case 1: return launch_force_t<MURB_MODE_PK_LDS, 8, 4, 4>(a, i_slots, s);
        case 2: return launch_force_t<MURB_MODE_PK_LDS, 4, 4, 4>(a, i_slots, s);
        case 3: return launch_force_t<MURB_MODE_PK_DIRECT, 8, 4, 1>(a, i_slots, s);
        case 4: return launch_force_t<MURB_MODE_SC_LDS, 8, 4, 4>(a, i_slots, s);
        case 5: return launch_force_t<MURB_MODE_PK_LDS, 16, 4, 4>(a, i_slots, s);
        case 6: return launch_force_t<MURB_MODE_PK_DIRECT, 4, 4, 1>(a, i_slots, s);
        case kPotentialKernel:   // few bodies: 2 per wave and 8 waves per workgroup, like murb_force_integrate_kernel (same sums per body)
            return i_slots <= 8192 ? launch_force_t<MURB_MODE_PHI, 2, 8, 4>(a, i_slots, s) : launch_force_t<MURB_MODE_PHI, 8, 4, 4>(a, i_slots, s);
        default: return MURBHIP_E_INVALID;
    }
}
// variant 1 with the state update in its tail (murb_force_integrate_kernel).  Few bodies: fewer i bodies per wave, i.e. more
// and shorter workgroups (N = 2 048 at 8 per wave is 64 workgroups on 256 CUs, each wave walking all j for 8 bodies); the
// sums of a body do not depend on how many others share its wave, so the results stay those of variant 1, bit for bit.
template <int R, int WAVES = 4>
int launch_force_integrate_t(const MurbForceArgs& a, const MurbIntegrateArgs& ia, int i_slots, hipStream_t s)
{
    const dim3 grid((unsigned)((i_slots + WAVES * R - 1) / (WAVES * R)), 1, 1);
    hipLaunchKernelGGL((murb_force_integrate_kernel<R, WAVES, 4>), grid, dim3(64 * WAVES), 0, s, a, ia);
    return hip_rc(hipGetLastError());
}
int launch_force_integrate(const MurbForceArgs& a, const MurbIntegrateArgs& ia, int i_slots, hipStream_t s)
{
    // 8 waves share a workgroup's staged j tiles up to 4 blocks (N = 2 048: 6.9 vs 7.3 us per step, 3 000: 8.6 vs 9.4,
    // 4 096: 10.2 vs 11.4; 5 000: 15.5 vs 14.9, 6 000: 18.2 vs 16.2 — profiles/r03_fused_small_steps.txt)
    if (i_slots <= 4096) return launch_force_integrate_t<2, 8>(a, ia, i_slots, s);
    if (i_slots <= 6144) return launch_force_integrate_t<2>(a, ia, i_slots, s);   // tools/rate_curve.py: 2 per wave wins up to 6 000,
    if (i_slots <= 8192) return launch_force_integrate_t<4>(a, ia, i_slots, s);   // 4 at 7 000 (21.9 vs 22.4 us), all equal from 8 193
    return launch_force_integrate_t<8>(a, ia, i_slots, s);
}
int launch_persistent(const MurbForceArgs& a, const MurbSchedule& sc, hipStream_t s)
{
    hipLaunchKernelGGL((murb_force_persistent<8, 4, 4>), dim3((unsigned)sc.nblocks), dim3(256), 0, s, a, sc);
    return hip_rc(hipGetLastError());
}

// The plan of the context as it stands (murb_choose.h).  A persistent plan needs the workgroups of its kernel that fit on a
// CU: asked of the runtime the first time such a plan is wanted, not before (the query loads the kernel).
Plan current_plan(murbhip_ctx* c)
{
    if (c->in.variant == kPersistentVariant && c->in.resident_per_cu == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, murb_force_persistent<8, 4, 4>, 256, 0) != hipSuccess || n < 1)
            n = 4;
        c->in.resident_per_cu = n;
    }
    return make_plan(c->in);
}

// ---- the shards' host threads: ShardCrew (murb_crew.h), one member per shard, bound to its device for life ---------------
// run() hands every member the same job for ITS shard and returns when all have finished enqueueing (never waits for the GPU);
// with one shard there is no thread: the caller runs the job.
int crew_run(murbhip_ctx* c, const std::function<int(Shard&)>& job)
{
    return c->crew->run([&](int i) -> int {
        Shard& sh = c->shards[(size_t)i];
        if (c->crew->threads() == 0) RC_TRY(hip_rc(hipSetDevice(sh.device)));   // a member thread set its device when it started
        return job(sh);
    });
}

// ---- timing spans ("profile") --------------------------------------------------------------------------------------------
// A span = two events recorded on `stream` around something; -1 = not recording (profiling off, level too low, pool empty:
// sampling just stops).  Each shard's spans are recorded by that shard's thread only.
int span_begin(murbhip_ctx* c, Shard& sh, int kind, hipStream_t stream, int* rc)
{
    const int level = (kind <= kProfTri2) ? 1 : 2;
    if (c->profile < level || sh.prof_used + 2 > sh.prof.size()) return -1;
    const int k = (int)(sh.prof_used / 2);
    sh.prof_used += 2;
    sh.prof_kind[(size_t)k] = kind;
    const int r = hip_rc(hipEventRecord(sh.prof[(size_t)2 * k], stream));
    if (r && !*rc) *rc = r;
    return k;
}
int span_end(Shard& sh, int span, hipStream_t stream)
{
    if (span < 0) return 0;
    return hip_rc(hipEventRecord(sh.prof[(size_t)2 * span + 1], stream));
}
// hipStreamWaitEvent as a span: the time the stream actually sat waiting (the exposed part of what it waits for)
int timed_wait(murbhip_ctx* c, Shard& sh, int kind, hipStream_t stream, hipEvent_t ev)
{
    int rc = 0;
    const int sp = span_begin(c, sh, kind, stream, &rc);
    RC_TRY(rc);
    HIP_TRY(hipStreamWaitEvent(stream, ev, 0));
    return span_end(sh, sp, stream);
}
// One launch on the compute stream as a span of its own kind ("profile" 2: the launch alone), then the launch's error.  `launch`
// enqueues and returns nothing; timed false: no span (the control-block forms of an adaptive step record none).
template <typename Enqueue>
int timed_launch(murbhip_ctx* c, Shard& sh, int kind, Enqueue&& launch, bool timed = true)
{
    int rc = 0;
    const int sp = timed ? span_begin(c, sh, kind, sh.compute, &rc) : -1;
    RC_TRY(rc);
    launch();
    RC_TRY(span_end(sh, sp, sh.compute));
    return hip_rc(hipGetLastError());
}

int build_sym_schedule(murbhip_ctx* c, Shard& sh, const Plan& p);
// The one-sided kernels' partial-sum rows: kMaxParts rows of float4 per local slot, zeroed once (rows a launch does
// not write must read as 0).  Not needed by the pair-symmetric plan, so only allocated when a one-sided launch, the
// one-sided potential sweep or murbhip_integrate_host_acc asks for it.
int ensure_accp(murbhip_ctx* c, Shard& sh) { return shard_alloc(sh, sh.accp, (size_t)kMaxParts * c->in.slice * sizeof(float4), sh.compute); }
// What a shard's read-out buffer (Shard::metrics) holds, in doubles: the block rows of murb_metrics_kernel, then the pair
// potentials of murbhip_energy — the partial sums of the two sets' groups (murb_sym_pe_sum_kernel) and the own slice's
// diagonal blocks (murb_sym_pe_diag_kernel).  One buffer so that one copy brings a tracked iteration's numbers to the host.
struct MetricsLayout {
    size_t blocks, pe_main, pe_tri, pe_diag, own_blocks, total;
};
MetricsLayout metrics_layout(const murbhip_ctx* c)
{
    MetricsLayout l{};
    l.blocks = (c->in.slice + 255) / 256;
    l.pe_main = l.blocks * MURB_METRIC_VALUES;
    l.pe_tri = l.pe_main + kPeSumBlocks;
    l.pe_diag = l.pe_tri + kPeSumBlocks;
    l.own_blocks = c->in.slice / MURB_SYM_BLOCK;
    l.total = l.pe_diag + l.own_blocks * MURB_PE_DIAG_SPLIT;
    return l;
}

int enqueue_sym_passes(murbhip_ctx* c, Shard& sh, bool potential);
int enqueue_sym_launch(murbhip_ctx* c, Shard& sh, int first, int count, bool own_triangle_rows = false,
                       hipStream_t stream = nullptr, bool potential = false, size_t comp_stride = 0, int kind = kProfForce);

// a fact for murbhip_get_info, noted by the first shard's thread only
inline void note_interactions(murbhip_ctx* c, const Shard& sh, double v) { if (&sh == &c->shards[0]) c->interactions_per_launch = v; }

// Force over the tiles of `which` (0 = own slice / everything when world == 1, 1 = all but own slice).
// `then`: the step's state update, to run in the tail of this launch (the one-sided kernel's default variant only;
// *fused says whether it did — otherwise the caller launches the integrate kernel as usual).
int enqueue_force(murbhip_ctx* c, Shard& sh, const Plan& p, int which, const MurbIntegrateArgs* then = nullptr, bool* fused = nullptr)
{
    MurbForceArgs a{};
    if (!p.symmetric) RC_TRY(ensure_accp(c, sh));
    a.rec = sh.rec[c->cur];
    a.accp = sh.accp;
    a.i_first_slot = (int)((unsigned long)sh.rank * c->in.slice);
    a.acc_stride = (unsigned int)c->in.slice;
    a.soft2 = c->soft2;
    const int tiles_local = (int)(c->in.slice / MURB_TILE_BODIES);
    const int tiles_all = (int)(c->in.slots / MURB_TILE_BODIES);
    if (which == 0) {
        a.tiles = MurbTileRange{sh.rank * tiles_local, tiles_local, tiles_local, 0};
        a.chunk_first = 0;
        a.nchunks = p.parts_local;
    } else {
        a.tiles = MurbTileRange{0, tiles_all - tiles_local, sh.rank * tiles_local, tiles_local};
        a.chunk_first = p.parts_local;
        a.nchunks = p.parts_remote;
    }
    const int i_slots = (int)sh.count;   // the grid rounds up to whole i groups; the extra slots hold mass 0
    if (p.symmetric) {   // one shard, no exchange: the whole triangle in one launch
        if (which != 0) return 0;
        RC_TRY(build_sym_schedule(c, sh, p));
        if (sh.sym_main.passes.size() > 1) {
            RC_TRY(enqueue_sym_passes(c, sh, false));
            note_interactions(c, sh, (double)c->in.n * (double)c->in.n / (double)sh.sym_main.passes.size());
            return 0;
        }
        RC_TRY(enqueue_sym_launch(c, sh, 0, sh.sym_items_total));   // its row sum is fused into the integrate launch
        note_interactions(c, sh, (double)c->in.n * (double)c->in.n);
        return 0;
    }
    if (p.persistent) {
        const MurbSchedule& sc = p.sched[which];
        if (sc.nblocks <= 0 || a.tiles.count <= 0) return 0;
        int rc = 0;
        const int sp = span_begin(c, sh, kProfForce, sh.compute, &rc);
        RC_TRY(rc);
        RC_TRY(launch_persistent(a, sc, sh.compute));
        RC_TRY(span_end(sh, sp, sh.compute));
    } else {
        if (a.nchunks <= 0 || a.tiles.count <= 0) return 0;
        int rc = 0;
        const int sp = span_begin(c, sh, kProfForce, sh.compute, &rc);
        RC_TRY(rc);
        if (then && fused && p.variant == kOneSidedVariant && a.nchunks == 1 && then->nparts == 1) {
            RC_TRY(launch_force_integrate(a, *then, i_slots, sh.compute));
            *fused = true;
        } else {
            RC_TRY(launch_force(p.variant, a, i_slots, sh.compute));
        }
        RC_TRY(span_end(sh, sp, sh.compute));
    }
    note_interactions(c, sh, (double)i_slots * (double)a.tiles.count * MURB_TILE_BODIES);
    return 0;
}

// Leapfrog kick length for a step of `dt`: half of it on the first step after an upload, otherwise
// the second half of the previous step's kick plus the first half of this one's.
inline float leapfrog_kick(const murbhip_ctx* c, float dt) { return c->lf_half ? 0.5f * (c->lf_last_dt + dt) : 0.5f * dt; }

// What the state update of a step works on (everything but the source of the accelerations, which the launch sites add).
MurbIntegrateArgs integrate_args(const murbhip_ctx* c, const Shard& sh, int nparts, float dt, int update_state, int scheme = -1,
                                 float* acc_out = nullptr)
{
    MurbIntegrateArgs a{};
    a.scheme = scheme >= 0 ? scheme : c->integrator;
    a.kick_dt = leapfrog_kick(c, dt);
    a.rec_in = sh.rec[c->cur];
    a.rec_out = sh.rec[c->cur ^ 1];
    a.vel = sh.vel;
    a.accp = sh.accp;
    a.acc_out = acc_out ? acc_out : sh.acc_out;
    a.i_first_slot = (int)((unsigned long)sh.rank * c->in.slice);
    a.count = (int)sh.count;
    a.nparts = nparts;
    a.acc_stride = (unsigned int)c->in.slice;
    a.dt = dt;
    a.update_state = update_state;
    return a;
}

int enqueue_integrate(murbhip_ctx* c, Shard& sh, int nparts, float dt, int update_state, const Plan* plan = nullptr,
                      int scheme = -1, float* acc_out = nullptr, bool acc_from_out = false)
{
    MurbIntegrateArgs a = integrate_args(c, sh, nparts, dt, update_state, scheme, acc_out);
    if (plan && plan->persistent) {
        a.group_bodies = 32;
        a.sched[0] = plan->sched[0];
        a.nsched = 1;
        if (c->in.world > 1 && plan->sched[1].nblocks > 0) { a.sched[1] = plan->sched[1]; a.nsched = 2; }
    }
    if (acc_from_out) a.acc_planes = sh.acc_out;   // remembered forces: nothing to sum
    if (plan && plan->symmetric && sh.sym_main.passes.size() > 1) {   // several passes: the sums are in the fp64 accumulator
        a.acc64 = sh.sym_acc64;
        a.acc64_stride = (unsigned int)c->in.slots;
    } else if (plan && plan->symmetric) {   // one shard, triangular schedule: row sum of the partial rows + update in one launch
        hipLaunchKernelGGL(murb_sym_rowsum_integrate_kernel, dim3((unsigned)(c->in.slots / 64)), dim3(MURB_ROWSUM_THREADS), 0, sh.compute,
                           sh.sym_main.part, sh.sym_main.comp_stride, sh.sym_main.rows, a);
        return hip_rc(hipGetLastError());
    }
    if (!acc_from_out && !a.acc64) { RC_TRY(ensure_accp(c, sh)); a.accp = sh.accp; }
    const unsigned pairs = (unsigned)(c->in.slice / 2);
    hipLaunchKernelGGL(murb_integrate_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, a);
    return hip_rc(hipGetLastError());
}

// Publish this shard's freshly integrated slice of rec[buf] to all shards and collect theirs (exchange stream).  Runs on
// the shard's own thread; every shard's job calls it (it contains a meet()).  `failed`: an earlier phase of this shard's
// job failed — keep meeting the others, enqueue nothing.
int shard_exchange(murbhip_ctx* c, Shard& sh, int buf, int failed)
{
    const size_t slice_f4 = c->in.slice;                  // float4 records per slice (1 per body slot)
    const size_t slice_bytes = slice_f4 * sizeof(float4);
    const bool idle = is_idle(c, sh);
    int rc = failed;
    if (!rc && !idle) rc = hip_rc(hipEventRecord(sh.ev_integrated, sh.compute));
    if (c->exchange == 0) c->crew->meet();             // the peers' ev_integrated are recorded
    if (rc) return rc;
    int span = -1;
    if (c->exchange == 1) {
        // one communicator per shard, each driven by its own thread: no ncclGroupStart/End around the calls
        HIP_TRY(hipStreamWaitEvent(sh.comm, sh.ev_integrated, 0));
        span = span_begin(c, sh, kProfAllGather, sh.comm, &rc);
        RC_TRY(rc);
        float4* base = sh.rec[buf];
        if (c->exchange_p2p && c->in.world > 1) {   // every slice straight to every peer: W - 1 sends and receives, one hop each
            Rccl& r = rccl();
            RC_TRY(nccl_rc(r.GroupStart()));
            for (int d = 1; d < c->in.world; ++d) {
                const int to = (sh.rank + d) % c->in.world, from = (sh.rank - d + c->in.world) % c->in.world;
                RC_TRY(nccl_rc(r.Send(base + (size_t)sh.rank * slice_f4, slice_f4 * 4, kRcclFloat, to, sh.comm_rccl, sh.comm)));
                RC_TRY(nccl_rc(r.Recv(base + (size_t)from * slice_f4, slice_f4 * 4, kRcclFloat, from, sh.comm_rccl, sh.comm)));
            }
            RC_TRY(nccl_rc(r.GroupEnd()));
        } else {
            RC_TRY(nccl_rc(rccl().AllGather(base + (size_t)sh.rank * slice_f4, base, slice_f4 * 4, kRcclFloat, sh.comm_rccl, sh.comm)));
        }
    } else {
        if (idle) return 0;
        // pull model: each shard copies every peer's slice out of the peer's buffer
        for (Shard& peer : c->shards) {
            if (&peer == &sh || is_idle(c, peer)) continue;
            HIP_TRY(hipStreamWaitEvent(sh.comm, peer.ev_integrated, 0));
        }
        HIP_TRY(hipStreamWaitEvent(sh.comm, sh.ev_integrated, 0));
        span = span_begin(c, sh, kProfAllGather, sh.comm, &rc);
        RC_TRY(rc);
        for (Shard& peer : c->shards) {
            if (&peer == &sh) continue;
            const size_t off = (size_t)peer.rank * slice_f4;
            if (peer.device == sh.device)
                HIP_TRY(hipMemcpyAsync(sh.rec[buf] + off, peer.rec[buf] + off, slice_bytes, hipMemcpyDeviceToDevice, sh.comm));
            else
                HIP_TRY(hipMemcpyPeerAsync(sh.rec[buf] + off, sh.device, peer.rec[buf] + off, peer.device, slice_bytes, sh.comm));
        }
    }
    RC_TRY(span_end(sh, span, sh.comm));
    if (!idle) HIP_TRY(hipEventRecord(sh.ev_gathered, sh.comm));
    return 0;
}

// three components, and behind them one float per group of 4 i bodies for the pair potential of a tracked evaluation
// (murb_kernels_sym.h, PHI = 2: entry ioff / 4 + group; zero wherever no item has groups)
inline size_t sym_part_bytes(size_t floats) { return (3 * floats + floats / MURB_SYM_R + 1) * sizeof(float); }

void free_sym_set(Shard& sh, SymSet& st)
{
    shard_free(sh, st.part, sym_part_bytes(st.comp_stride));
    shard_free(sh, st.rows, (size_t)st.nblocks * sizeof(MurbSymBlockRows));
    st = SymSet{};
}

int upload_sym_set(Shard& sh, SymSet& st, const std::vector<MurbSymBlockRows>& table, size_t floats)
{
    st.comp_stride = floats;
    st.nblocks = (int)table.size();
    if (floats == 0) return 0;
    // every cell has a writer; zero anyway (on OUR stream: non-blocking w.r.t. stream 0)
    RC_TRY(shard_alloc(sh, st.part, sym_part_bytes(floats), sh.compute));
    RC_TRY(shard_alloc(sh, st.rows, table.size() * sizeof(MurbSymBlockRows)));
    HIP_TRY(hipMemcpy(st.rows, table.data(), table.size() * sizeof(MurbSymBlockRows), hipMemcpyHostToDevice));
    return 0;
}

// ---- pair-symmetric schedule over several ranks ("half ring") --------------------------------------
// Rank r evaluates, once each, the block pairs of (own slice x own slice) and of (own slice x slice
// r+d) for d = 1 .. floor(W/2); for even W the pair of slices half a ring apart is shared: the lower
// rank takes the first half of ITS blocks against all of the other's, the higher rank the rest.  Every
// unordered body pair is evaluated by exactly one rank.  A rank's partial sums for ALL slices it
// touched are then row-summed into one chunk per slice and combined with ONE reduce-scatter (each
// rank receives the complete accelerations of its own bodies); positions travel as before.
inline bool exchange_mode(const murbhip_ctx* c) { return c->in.world > 1 || c->force_exchange; }
SymLayoutKey layout_key(const murbhip_ctx* c, const Plan& p)
{
    return sym_layout_key(c->in, p, exchange_mode(c), c->overlap, c->tri_first_pct, c->xcd_order != 0, c->pad_aware != 0);
}

// false when the shard's tables were built for exactly this key.  A rebuild of EXISTING tables needs every shard of the
// process drained first (the peer-read sums of the previous step may still be reading this shard's send buffer):
// drain_for_rebuild does that on the caller's thread before the shards' threads start.
inline bool sym_schedule_stale(const Shard& sh, const SymLayoutKey& key) { return !sh.sym_items || !(sh.key == key); }
int drain_for_rebuild(murbhip_ctx* c, const Plan& p)
{
    if (!p.symmetric) return 0;
    const SymLayoutKey key = layout_key(c, p);
    for (const Shard& sh : c->shards)
        if (sh.sym_items && sym_schedule_stale(sh, key)) return murbhip_sync(c);   // nothing may be in flight
    return 0;
}

int build_sym_schedule(murbhip_ctx* c, Shard& sh, const Plan& p)
{
    const SymLayoutKey key = layout_key(c, p);
    sh.sym_red = p.red;
    if (!sym_schedule_stale(sh, key)) return 0;
    shard_free(sh, sh.sym_items, (size_t)sh.sym_items_total * sizeof(MurbSymItem));
    free_sym_set(sh, sh.sym_main);
    free_sym_set(sh, sh.sym_tri);

    SymHostLayout L;
    plan_sym_layout(c->in.world, sh.rank, sym_fill(c->in.n, c->in.world, key.pad_aware), key, L);
    if (!key.exchange_mode && L.passes.size() == 1 && (int)L.table_main.size() != (int)(c->in.slots / MURB_SYM_BLOCK))
        return MURBHIP_E_STATE;   // the fused row sum + integrate walks every block
    RC_TRY(upload_sym_set(sh, sh.sym_tri, L.table_tri, L.floats_tri));
    RC_TRY(upload_sym_set(sh, sh.sym_main, L.table_main, L.floats_main));
    sh.sym_main.passes = L.passes;
    if (L.passes.size() > 1) RC_TRY(shard_alloc(sh, sh.sym_acc64, 3 * c->in.slots * sizeof(double)));
    sh.sym_items_own = L.own;
    sh.sym_items_total = (int)L.items.size();
    sh.sym_t1 = L.t1;
    RC_TRY(shard_alloc(sh, sh.sym_items, L.items.size() * sizeof(MurbSymItem)));
    HIP_TRY(hipMemcpy(sh.sym_items, L.items.data(), L.items.size() * sizeof(MurbSymItem), hipMemcpyHostToDevice));
    sh.key = key;
    if (key.exchange_mode) {
        const int W = c->in.world;
        const size_t chunk = (size_t)3 * c->in.slice * sizeof(float);
        RC_TRY(shard_alloc(sh, sh.sym_send, chunk * W));
        RC_TRY(shard_alloc(sh, sh.sym_recv, chunk));
        RC_TRY(shard_alloc(sh, sh.sym_tri_acc, chunk));
        // receive area of the point-to-point exchange (read as 0 where nothing has arrived yet)
        if (W > 1) RC_TRY(shard_alloc(sh, sh.sym_p2p, chunk * (size_t)(W / 2), sh.compute));
        if (!sh.ev_rowsum) HIP_TRY(hipEventCreateWithFlags(&sh.ev_rowsum, hipEventDisableTiming));
        if (!sh.ev_reduced) HIP_TRY(hipEventCreateWithFlags(&sh.ev_reduced, hipEventDisableTiming));
        // chunks of slices this rank has no rows for are never written by the row sum: they must read as 0
        HIP_TRY(hipMemsetAsync(sh.sym_send, 0, chunk * W, sh.compute));
    }
    return 0;
}

// form: 0 forces, i-side sums in registers; 1 potential sweep; 2 forces + pair potential; 3 forces, i-side sums through LDS
// WIDE: the pair factor as (G m inv) inv^2 ("sym_wide"; the potential sweep has no cube and one form)
template <int WAVES, int WIDE>
void launch_sym_t(int form, int count, hipStream_t stream, const MurbSymArgs& sa)
{
    const dim3 grid((unsigned)count), block(64 * WAVES);
    if (form == 1) hipLaunchKernelGGL((murb_force_sym_kernel<4, WAVES, 1, 1>), grid, block, 0, stream, sa);
    else if (form == 2) hipLaunchKernelGGL((murb_force_sym_kernel<4, WAVES, 1, 2, 1, WIDE>), grid, block, 0, stream, sa);
    else if (form == 3) hipLaunchKernelGGL((murb_force_sym_kernel<4, WAVES, 1, 0, 1, WIDE>), grid, block, 0, stream, sa);
    else hipLaunchKernelGGL((murb_force_sym_kernel<4, WAVES, 1, 0, 0, WIDE>), grid, block, 0, stream, sa);
}

int enqueue_sym_launch(murbhip_ctx* c, Shard& sh, int first, int count, bool own_triangle_rows, hipStream_t stream,
                       bool potential, size_t comp_stride, int kind)
{
    if (count <= 0) return 0;
    if (!stream) stream = sh.compute;
    ++sh.sym_launches;
    const SymSet& st = own_triangle_rows ? sh.sym_tri : sh.sym_main;
    MurbSymArgs sa{};
    sa.rec = sh.rec[c->cur];
    sa.part = st.part;
    sa.comp_stride = comp_stride ? comp_stride : st.comp_stride;
    sa.items = sh.sym_items;
    sa.item_first = first;
    sa.soft2 = c->soft2;
    const bool with_pe = !potential && c->want_pe;           // force + pair potential in one pass (murb_kernels_sym.h, PHI = 2)
    const bool timed = stream == sh.compute && !potential;   // the profiling events live on the main compute stream
    int rc_span = 0;
    const int sp = timed ? span_begin(c, sh, kind, stream, &rc_span) : -1;
    RC_TRY(rc_span);
    const int form = potential ? 1 : (with_pe ? 2 : (sh.sym_red == 1 ? 3 : 0));
    const bool wide = sym_wide_chosen(c->sym_wide, c->sym_wide_needed);
    if (sh.key.waves == 8) { if (wide) launch_sym_t<8, 1>(form, count, stream, sa); else launch_sym_t<8, 0>(form, count, stream, sa); }
    else { if (wide) launch_sym_t<4, 1>(form, count, stream, sa); else launch_sym_t<4, 0>(form, count, stream, sa); }
    RC_TRY(hip_rc(hipGetLastError()));
    RC_TRY(span_end(sh, sp, stream));
    return 0;
}

// row sum of a set's partial rows into `out` (chunks of [3][out_slice_slots])
int enqueue_sym_rowsum(const SymSet& st, float* out, unsigned int out_slice_slots, hipStream_t stream)
{
    if (st.nblocks <= 0) return 0;
    hipLaunchKernelGGL(murb_sym_rowsum_kernel, dim3((unsigned)st.nblocks * (MURB_SYM_BLOCK / 64)), dim3(MURB_ROWSUM_THREADS), 0, stream,
                       st.part, st.comp_stride, st.rows, out, out_slice_slots);
    return hip_rc(hipGetLastError());
}

// The reduce-scatter of the send chunks on the exchange stream: every rank ends up with the other ranks' (and its own
// rectangles') contributions to its own bodies in sym_recv.  Called by every shard's thread after its row sum has been
// enqueued (ev_rowsum recorded; with peer copies: after the meet() that follows).
int shard_reduce_scatter(murbhip_ctx* c, Shard& sh)
{
    const unsigned int chunk_floats = (unsigned int)(3 * c->in.slice);
    const bool idle = is_idle(c, sh);
    int rc = 0, span = -1;
    if (c->exchange == 1 && c->exchange_p2p && c->in.world > 1) {
        // Point-to-point form.  Under the half-ring schedule a rank only has contributions for the floor(W/2) slices ahead of
        // it (and its own): the reduce-scatter moves and adds zeros for the rest.  Here every rank sends those chunks straight
        // to their owners (one xGMI hop each, all links at once) and adds up what the floor(W/2) ranks behind it sent.
        Rccl& r = rccl();
        const int W = c->in.world, D = W / 2;
        HIP_TRY(hipStreamWaitEvent(sh.comm, sh.ev_rowsum, 0));
        span = span_begin(c, sh, kProfReduceScatter, sh.comm, &rc);
        RC_TRY(rc);
        RC_TRY(nccl_rc(r.GroupStart()));
        for (int d = 1; d <= D; ++d) {
            const int to = (sh.rank + d) % W, from = (sh.rank - d + W) % W;
            RC_TRY(nccl_rc(r.Send(sh.sym_send + (size_t)to * chunk_floats, chunk_floats, kRcclFloat, to, sh.comm_rccl, sh.comm)));
            RC_TRY(nccl_rc(r.Recv(sh.sym_p2p + (size_t)(d - 1) * chunk_floats, chunk_floats, kRcclFloat, from, sh.comm_rccl, sh.comm)));
        }
        RC_TRY(nccl_rc(r.GroupEnd()));
        hipLaunchKernelGGL(murb_sym_chunk_sum_kernel, dim3((chunk_floats + 255) / 256), dim3(256), 0, sh.comm,
                           sh.sym_send + (size_t)sh.rank * chunk_floats, sh.sym_p2p, D, chunk_floats, sh.sym_recv);
        RC_TRY(hip_rc(hipGetLastError()));
    } else if (c->exchange == 1) {
        HIP_TRY(hipStreamWaitEvent(sh.comm, sh.ev_rowsum, 0));
        span = span_begin(c, sh, kProfReduceScatter, sh.comm, &rc);
        RC_TRY(rc);
        RC_TRY(nccl_rc(rccl().ReduceScatter(sh.sym_send, sh.sym_recv, chunk_floats, kRcclFloat, kRcclSum, sh.comm_rccl, sh.comm)));
    } else {
        if (idle) return 0;
        // Under the half-ring schedule only the floor(W/2) ranks BEHIND this one (and the rank itself) hold contributions to its
        // slice: the chunks the others keep for it are zero and are not read (no xGMI traffic for zeros).  Fixed order: own,
        // then by distance along the ring.
        const int W = c->in.world, D = W / 2;
        MurbPeerPtrs peers{};
        peers.n = 0;
        for (int d = 0; d <= D; ++d) {
            const int from = (sh.rank - d + W) % W;
            if (d > 0 && from == sh.rank) break;
            for (Shard& peer : c->shards)
                if (peer.rank == from) { peers.p[peers.n++] = peer.sym_send; HIP_TRY(hipStreamWaitEvent(sh.comm, peer.ev_rowsum, 0)); }
        }
        span = span_begin(c, sh, kProfReduceScatter, sh.comm, &rc);
        RC_TRY(rc);
        hipLaunchKernelGGL(murb_sym_peer_sum_kernel, dim3((chunk_floats + 255) / 256), dim3(256), 0, sh.comm, peers,
                           (unsigned long)sh.rank * chunk_floats, chunk_floats, sh.sym_recv);
        RC_TRY(hip_rc(hipGetLastError()));
    }
    RC_TRY(span_end(sh, span, sh.comm));
    if (!idle) HIP_TRY(hipEventRecord(sh.ev_reduced, sh.comm));
    return 0;
}

// nobody may still be reading our send buffer: the peer-read sums of the previous step (one process), or our own
// previous reduce-scatter (RCCL reads it on the exchange stream)
int wait_send_buffer_free(murbhip_ctx* c, Shard& sh)
{
    if (!c->reduce_pending) return 0;
    if (c->exchange == 0) {   // the readers of this shard's send buffer: itself and the floor(W/2) ranks AHEAD of it (shard_reduce_scatter)
        const int W = c->in.world, D = W / 2;
        for (Shard& peer : c->shards)
            if ((peer.rank - sh.rank + W) % W <= D) HIP_TRY(hipStreamWaitEvent(sh.compute, peer.ev_reduced, 0));
    } else HIP_TRY(hipStreamWaitEvent(sh.compute, sh.ev_reduced, 0));
    return 0;
}

// One iteration under the half-ring schedule: ONE shard's share, enqueued by that shard's own thread (ShardCrew).  On the
// compute stream unless noted:
//   T1  first part of the own-slice triangle          (needs no remote data: overlaps the position gather)
//       wait: positions of the previous step gathered
//   R   rectangles against the other slices            -> the rectangles' rows (sym_main)
//   SR  row sum of those rows -> send chunks           (own-slice chunk = i-side sums of the rectangles)
//       [exchange stream] reduce-scatter of the chunks -> recv          (overlaps T2)
//   T2  rest of the own-slice triangle                 -> the triangle's rows (sym_tri)
//       wait: reduce-scatter done
//   I   row sum of the triangle's rows + recv, state update: one launch ; then [exchange stream] all-gather of the new positions
// The triangle never enters the reduce-scatter (it only touches the rank's own bodies), which is what
// lets half of it hide the collective's latency.
// The context's fields (cur, gather_pending, ...) are read-only while the shards' threads run; the caller updates them
// afterwards.  meet() only where a stream must wait for an event ANOTHER shard's thread records (peer-copy exchange): the
// shards otherwise never wait for each other on the host.
int shard_iteration_sym_multi(murbhip_ctx* c, Shard& sh, const Plan& p, float dt, int update_state)
{
    const bool idle = is_idle(c, sh);   // "solo_shard" timing aid: idle shards enqueue no work of their own
    const bool copies = c->exchange == 0;
    int rc = build_sym_schedule(c, sh, p);
    const int own = sh.sym_items_own, t1 = sh.sym_t1;
    int step_span = -1;
    if (!rc && !idle) rc = [&]() -> int {
        int r = 0;
        step_span = span_begin(c, sh, kProfStep, sh.compute, &r);
        RC_TRY(r);
        if (c->overlap == 2) {
            // the whole own-slice triangle on a second, lowest-priority compute stream: it runs alone while
            // the positions are still being gathered, then fills the gaps and the tail of the rectangles
            if (c->gather_pending || c->reduce_pending) HIP_TRY(hipStreamWaitEvent(sh.compute_low, sh.ev_integrated, 0));
            RC_TRY(enqueue_sym_launch(c, sh, 0, own, true, sh.compute_low));
            RC_TRY(enqueue_sym_rowsum(sh.sym_tri, sh.sym_tri_acc, (unsigned int)c->in.slice, sh.compute_low));
            HIP_TRY(hipEventRecord(sh.ev_tri, sh.compute_low));
        }
        RC_TRY(enqueue_sym_launch(c, sh, 0, t1, true, nullptr, false, 0, kProfTri1));
        if (c->gather_pending) RC_TRY(timed_wait(c, sh, kProfWaitGather, sh.compute, sh.ev_gathered));
        RC_TRY(enqueue_sym_launch(c, sh, own, sh.sym_items_total - own, false, nullptr, false, 0, kProfRect));
        RC_TRY(wait_send_buffer_free(c, sh));
        RC_TRY(enqueue_sym_rowsum(sh.sym_main, sh.sym_send, (unsigned int)c->in.slice, sh.compute));
        HIP_TRY(hipEventRecord(sh.ev_rowsum, sh.compute));
        // what ONE launch covers on average: the rank's share of the step over its non-empty force launches
        const int launches = (t1 > 0) + (own - t1 > 0 || c->overlap == 2) + (sh.sym_items_total - own > 0);
        note_interactions(c, sh, (double)sh.count * (double)c->in.n / (double)std::max(launches, 1));
        return 0;
    }();
    if (copies) c->crew->meet();   // every shard's ev_rowsum is recorded
    if (!rc) rc = shard_reduce_scatter(c, sh);
    if (!rc && !idle) rc = [&]() -> int {
        // meanwhile: the rest of the own-slice triangle and its row sum
        if (c->overlap == 2) {
            HIP_TRY(hipStreamWaitEvent(sh.compute, sh.ev_tri, 0));
        } else {
            RC_TRY(enqueue_sym_launch(c, sh, t1, own - t1, true, nullptr, false, 0, kProfTri2));
        }
        RC_TRY(timed_wait(c, sh, kProfWaitReduce, sh.compute, sh.ev_reduced));
        MurbIntegrateArgs a = integrate_args(c, sh, 0, dt, update_state);   // no one-sided partial rows: the sums come in planes
        a.acc_planes = sh.sym_recv;
        if (c->overlap == 2) {   // the triangle's row sums were taken on the other stream
            a.acc_planes2 = sh.sym_tri_acc;
            hipLaunchKernelGGL(murb_integrate_kernel, dim3((unsigned)((c->in.slice / 2 + 255) / 256)), dim3(256), 0, sh.compute, a);
        } else {                 // row sum of the triangle's rows + the reduced share + state update in one launch
            hipLaunchKernelGGL(murb_sym_rowsum_integrate_kernel, dim3((unsigned)(c->in.slice / 64)), dim3(MURB_ROWSUM_THREADS), 0, sh.compute,
                               sh.sym_tri.part, sh.sym_tri.comp_stride, sh.sym_tri.rows, a);
        }
        RC_TRY(hip_rc(hipGetLastError()));
        RC_TRY(span_end(sh, step_span, sh.compute));
        if (!update_state) HIP_TRY(hipEventRecord(sh.ev_integrated, sh.compute));   // else shard_exchange records it
        return 0;
    }();
    if (update_state) rc = shard_exchange(c, sh, c->cur ^ 1, rc);
    return rc;
}

// One GPU, several passes: every pass's items into the shared row buffer, its row sums added to the fp64 accumulator.
int enqueue_sym_passes(murbhip_ctx* c, Shard& sh, bool potential)
{
    HIP_TRY(hipMemsetAsync(sh.sym_acc64, 0, 3 * c->in.slots * sizeof(double), sh.compute));
    // force + pair potential (murbhip_energy): every pass has a layout of its own in the shared buffer, so the plane of the
    // groups' potentials — one float per group of the pass's i rows, zero elsewhere — is cleared before the pass and summed
    // right after it, into the same doubles of the read-out buffer pass after pass
    const bool with_pe = !potential && c->want_pe && sh.metrics;
    bool first = true;
    for (const SymPass& ps : sh.sym_main.passes) {
        float* const pe_plane = sh.sym_main.part + 3 * ps.floats;
        const size_t pe_count = ps.floats / MURB_SYM_R + 1;
        if (with_pe) HIP_TRY(hipMemsetAsync(pe_plane, 0, pe_count * sizeof(float), sh.compute));
        RC_TRY(enqueue_sym_launch(c, sh, ps.item_first, ps.item_count, false, nullptr, potential, ps.floats));
        if (with_pe) {
            hipLaunchKernelGGL(murb_sym_pe_sum_kernel, dim3(kPeSumBlocks), dim3(1024), 0, sh.compute, pe_plane, (unsigned long)pe_count,
                               sh.metrics + metrics_layout(c).pe_main, first ? 0 : 1);
            RC_TRY(hip_rc(hipGetLastError()));
            first = false;
        }
        hipLaunchKernelGGL(murb_sym_rowsum_acc_kernel, dim3((unsigned)ps.table_count * (MURB_SYM_BLOCK / 64)), dim3(MURB_ROWSUM_THREADS), 0,
                           sh.compute, sh.sym_main.part, ps.floats, sh.sym_main.rows + ps.table_first, sh.sym_acc64, (unsigned int)c->in.slots);
        RC_TRY(hip_rc(hipGetLastError()));
    }
    return 0;
}

// The potential sweep of murbhip_energy under the half-ring schedule: the same items as a force evaluation in the
// kernel's PHI form (phi_i += G m_j / r and phi_j += G m_i / r per pair, once), the same reduce-scatter — half the
// pair terms of a one-sided sweep per rank.  No overlap games here: triangle, rectangles, row sums, reduce-scatter,
// phi = received + own triangle.  A collective in one-process-per-GPU mode, like a step.  One shard's share, on its thread.
int shard_potential_sym_multi(murbhip_ctx* c, Shard& sh, const Plan& p)
{
    const bool idle = is_idle(c, sh);
    int rc = build_sym_schedule(c, sh, p);
    if (!rc && !idle) rc = [&]() -> int {
        if (c->gather_pending) HIP_TRY(hipStreamWaitEvent(sh.compute, sh.ev_gathered, 0));
        RC_TRY(enqueue_sym_launch(c, sh, 0, sh.sym_items_own, true, nullptr, true));
        RC_TRY(enqueue_sym_launch(c, sh, sh.sym_items_own, sh.sym_items_total - sh.sym_items_own, false, nullptr, true));
        RC_TRY(enqueue_sym_rowsum(sh.sym_tri, sh.sym_tri_acc, (unsigned int)c->in.slice, sh.compute));
        RC_TRY(wait_send_buffer_free(c, sh));
        RC_TRY(enqueue_sym_rowsum(sh.sym_main, sh.sym_send, (unsigned int)c->in.slice, sh.compute));
        HIP_TRY(hipEventRecord(sh.ev_rowsum, sh.compute));
        return 0;
    }();
    if (c->exchange == 0) c->crew->meet();
    if (!rc) rc = shard_reduce_scatter(c, sh);
    if (rc || idle) return rc;
    HIP_TRY(hipStreamWaitEvent(sh.compute, sh.ev_reduced, 0));
    MurbIntegrateArgs a{};   // no state update: phi_out = received + own triangle (component 0 is the potential)
    a.rec_in = sh.rec[c->cur];
    a.rec_out = sh.rec[c->cur ^ 1];
    a.vel = sh.vel;
    a.acc_out = sh.phi_out;
    a.acc_planes = sh.sym_recv;
    a.acc_planes2 = sh.sym_tri_acc;
    a.i_first_slot = (int)((unsigned long)sh.rank * c->in.slice);
    a.count = (int)sh.count;
    a.acc_stride = (unsigned int)c->in.slice;
    a.update_state = 0;
    hipLaunchKernelGGL(murb_integrate_kernel, dim3((unsigned)((c->in.slice / 2 + 255) / 256)), dim3(256), 0, sh.compute, a);
    return hip_rc(hipGetLastError());
}

// One iteration with the one-sided kernels (or with one shard and no exchange): one shard's share, on its thread.
int shard_iteration_plain(murbhip_ctx* c, Shard& sh, const Plan& p, float dt, int update_state, bool reuse)
{
    const bool exchange = update_state && (c->in.world > 1 || c->force_exchange);
    int rc = 0;
    if (!is_idle(c, sh)) rc = [&]() -> int {   // timing aid: see "solo_shard"
        // one-sided kernel, one GPU, one j chunk: the state update rides in the tail of the force launch (murb_force_integrate_kernel)
        bool fused = false;
        MurbIntegrateArgs then{};
        const bool may_fuse = c->in.fuse_integrate && !reuse && !p.symmetric && !p.persistent && p.variant == kOneSidedVariant &&
                              c->in.world == 1 && p.parts_local + p.parts_remote == 1;
        if (may_fuse) {
            RC_TRY(ensure_accp(c, sh));
            then = integrate_args(c, sh, p.parts_local + p.parts_remote, dt, update_state);
        }
        const MurbIntegrateArgs* const tail = may_fuse ? &then : nullptr;
        if (c->in.world == 1 || reuse) {   // reuse: the forces at these positions are in acc_out, only the update is left
            if (c->gather_pending) HIP_TRY(hipStreamWaitEvent(sh.compute, sh.ev_gathered, 0));
            if (!reuse) RC_TRY(enqueue_force(c, sh, p, 0, tail, &fused));
        } else if (c->overlap) {
            RC_TRY(enqueue_force(c, sh, p, 0));   // own slice: written by our own integrate, already ordered
            if (c->gather_pending) RC_TRY(timed_wait(c, sh, kProfWaitGather, sh.compute, sh.ev_gathered));
            RC_TRY(enqueue_force(c, sh, p, 1, tail, &fused));
        } else {
            if (c->gather_pending) RC_TRY(timed_wait(c, sh, kProfWaitGather, sh.compute, sh.ev_gathered));
            RC_TRY(enqueue_force(c, sh, p, 0));
            RC_TRY(enqueue_force(c, sh, p, 1, tail, &fused));
        }
        if (fused) return 0;
        return enqueue_integrate(c, sh, p.parts_local + p.parts_remote, dt, update_state, reuse ? nullptr : &p, -1, nullptr, reuse);
    }();
    if (exchange) rc = shard_exchange(c, sh, c->cur ^ 1, rc);
    return rc;
}

// The body state changed (upload, device initialisation, an update from host accelerations, a step of any integrator):
// neither the remembered forces, nor the remembered pair potential, nor the Hermite integrator's remembered (a0, j0), nor
// the metric sums (state_serial) belong to the new one.  Every change of the bodies goes through here.
void invalidate_cached_forces(murbhip_ctx* c)
{
    c->acc_current = false;
    c->pe_current = false;
    c->herm_current = false;
    c->herm_proposal = false;
    c->blk_open = false;        // murbhip_evolve_block: an open block is closed, the bodies' levels are dropped
    c->blk_have_levels = 0;
    c->trc_current = false;     // the tracers' (a0, j0) were made against the old bodies (murbtracer.h)
    c->ac_live = false;         // an Ahmad-Cohen scheme ends with whatever steps the bodies another way (murbac.h)
    ++c->state_serial;
}

int enqueue_iteration(murbhip_ctx* c, float dt, int update_state)
{
    const Plan p = current_plan(c);
    c->herm_in_acc_out = false;   // acc_out is the force plan's from here on
    // forces at the current positions are already in acc_out (compute_acc, or a leapfrog read-out, just ran): an
    // evaluation needs nothing at all, a state update (one shard, no exchange) only the integrate launch
    const bool have_acc = c->acc_current;
    const bool have_pe = c->pe_current;
    c->acc_current = false;
    c->pe_current = false;
    if (have_acc && !update_state && (!c->want_pe || have_pe)) { c->acc_current = true; c->pe_current = have_pe; return 0; }
    const bool exchanging = exchange_mode(c);
    // ... with several shards: the integrate launch from the remembered forces and the position exchange
    const bool reuse = have_acc && update_state && c->solo_shard < 0;
    RC_TRY(drain_for_rebuild(c, p));   // tables are rebuilt below
    if (p.symmetric && exchanging && !reuse)
        RC_TRY(crew_run(c, [&](Shard& sh) { return shard_iteration_sym_multi(c, sh, p, dt, update_state); }));
    else
        RC_TRY(crew_run(c, [&](Shard& sh) { return shard_iteration_plain(c, sh, p, dt, update_state, reuse); }));
    if (p.symmetric && exchanging && !reuse) c->reduce_pending = true;
    if (update_state) {
        if (exchanging) c->gather_pending = true;
        c->cur ^= 1;
        invalidate_cached_forces(c);
    } else {
        c->acc_current = true;
        c->pe_current = c->want_pe && p.symmetric;
    }
    return 0;
}

// ---- 4th-order Hermite predictor-corrector ("integrator" 2, murb_kernels_hermite.h) ------------------------------------------
// One shard only.  A step is predictor, ONE acceleration + jerk sweep at the predicted state, corrector; the first step after
// a change of the bodies evaluates (a0, j0) at the current state first.  One launch shape for every N: 4 i bodies per wave,
// 4 waves per workgroup, 2 position + 2 velocity tiles per stage (32 KiB of LDS, like the one-sided force kernel).
constexpr int kHermiteR = 4, kHermiteWaves = 4, kHermiteStage = 2;
constexpr int kTidalStage = 4;   // the tidal sweep stages positions alone: 4 tiles fill the 32 KiB the sweeps' 2 tiles with velocities do

int ensure_hermite(murbhip_ctx* c, Shard& sh, int rows)
{
    // each buffer under its own guard: a failed allocation leaves its pointer null and the next call tries again
    const size_t rec_bytes = c->in.slots * sizeof(float4), plane_bytes = 3 * c->in.slots * sizeof(float);
    for (float4** p : {&sh.herm_rec, &sh.herm_vel}) RC_TRY(shard_alloc(sh, *p, rec_bytes));
    for (float** p : {&sh.herm_a0, &sh.herm_j0}) RC_TRY(shard_alloc(sh, *p, plane_bytes, sh.compute));
    if (rows > sh.herm_rows) {   // more chunks than before ("jsplit"): the rows in flight are read by an enqueued corrector
        HIP_TRY(hipStreamSynchronize(sh.compute));
        shard_free(sh, sh.herm_part, (size_t)2 * sh.herm_rows * c->in.slots * sizeof(float4));
        sh.herm_rows = 0;
        // slots past the last i group have no writer: they read as 0
        RC_TRY(shard_alloc(sh, sh.herm_part, (size_t)2 * rows * c->in.slots * sizeof(float4), sh.compute));
        sh.herm_rows = rows;
    }
    if (c->nearest || c->contact) {
        RC_TRY(shard_alloc(sh, sh.nn_idx, c->in.slots * sizeof(int), sh.compute));
        RC_TRY(shard_alloc(sh, sh.nn_r2, c->in.slots * sizeof(float), sh.compute));
        RC_TRY(shard_alloc(sh, sh.enc, sizeof(MurbEncList), sh.compute));
    }
    if (c->potential) RC_TRY(shard_alloc(sh, sh.herm_phi, c->in.slots * sizeof(float), sh.compute));
    return 0;
}

// radius^2 + soft^2 as the kernels compare it with r2; -1 (no r2 is that small): no encounter stop
inline float encounter_threshold(const murbhip_ctx* c)
{
    return c->enc_radius > 0.f ? (float)((double)c->enc_radius * (double)c->enc_radius + (double)c->soft2) : -1.f;
}

// The side product the Hermite sweeps keep: murbhip_set_option lets at most one of the three options be on.
inline MurbSide sweep_side(const murbhip_ctx* c)
{
    return c->potential ? MurbSide::Potential : c->contact ? MurbSide::Contact : c->nearest ? MurbSide::Nearest : MurbSide::None;
}

// side -> the kernel of the fixed sweep and of the active sweep.  The forms with a side product take the control block of an
// adaptive step or null; the plain fixed sweep is two kernels, one that takes none and one that takes it.
#define MURB_SWEEP(name) ((const void*)name<kHermiteR, kHermiteWaves, kHermiteStage>)
const void* fixed_sweep_kernel(const MurbSide side, const bool with_ctl)
{
    switch (side) {
    case MurbSide::Potential: return MURB_SWEEP(murb_force_jerk_pot_kernel);
    case MurbSide::Contact: return MURB_SWEEP(murb_contact_sweep_kernel);
    case MurbSide::Nearest: return MURB_SWEEP(murb_nn_sweep_kernel);
    case MurbSide::None: break;
    }
    return !with_ctl ? MURB_SWEEP(murb_force_jerk_kernel) : MURB_SWEEP(murb_force_jerk_adaptive_kernel);
}
const void* active_sweep_kernel(const MurbSide side)
{
    switch (side) {
    case MurbSide::Potential: return MURB_SWEEP(murb_force_jerk_pot_block_kernel);
    case MurbSide::Contact: return MURB_SWEEP(murb_contact_active_sweep_kernel);
    case MurbSide::Nearest: return MURB_SWEEP(murb_nn_active_sweep_kernel);
    case MurbSide::None: break;
    }
    return MURB_SWEEP(murb_force_jerk_block_kernel);
}
#undef MURB_SWEEP

// the per-slot arrays of the side product as the correctors take them (MurbHermiteArgs, MurbBlockArgs)
template <typename Args>
void side_slots(const murbhip_ctx* c, const Shard& sh, Args& a)
{
    if (c->nearest || c->contact) { a.nn_idx = sh.nn_idx; a.nn_r2 = sh.nn_r2; a.enc = sh.enc; }
    a.contact = c->contact;
    if (c->potential) a.phi = sh.herm_phi;
}

MurbHermiteArgs hermite_args(const murbhip_ctx* c, const Shard& sh, int parts, float dt, int update_state)
{
    MurbHermiteArgs a{};
    a.rec_in = sh.rec[c->cur];
    a.vel = sh.vel;
    a.a0 = sh.herm_a0;
    a.j0 = sh.herm_j0;
    a.part_a = sh.herm_part;
    a.part_j = sh.herm_part + (size_t)sh.herm_rows * c->in.slots;
    a.acc_out = sh.acc_out;
    a.nparts = parts;
    a.count = (int)sh.count;
    a.stride = (unsigned int)c->in.slots;
    a.dt = dt;
    a.update_state = update_state;
    side_slots(c, sh, a);
    return a;
}

// accelerations and jerks of the state (rec, vel) into the partial rows.  `ctl`: the control-block form of an adaptive step
// (enqueue_hermite_adaptive), which records no timing span.
int enqueue_hermite_sweep(murbhip_ctx* c, Shard& sh, const float4* rec, const float4* vel, int parts, const MurbEvolveCtl* ctl = nullptr)
{
    MurbNNJerkArgs a{};   // the plain sweeps take its base
    a.count = (int)sh.count;
    a.rec = rec;
    a.vel = vel;
    a.part_a = sh.herm_part;
    a.part_j = sh.herm_part + (size_t)sh.herm_rows * c->in.slots;
    a.tiles = (int)(c->in.slots / MURB_TILE_BODIES);
    a.nchunks = parts;
    a.stride = (unsigned int)c->in.slots;
    a.soft2 = c->soft2;
    constexpr int group = kHermiteWaves * kHermiteR;
    const dim3 grid((unsigned)((sh.count + group - 1) / group), (unsigned)parts, 1);   // whole i groups: the extra slots hold mass 0
    void* args[] = {&a, &ctl};   // a kernel takes as many as it has, and of `a` what its parameter's type holds
    RC_TRY(timed_launch(c, sh, kProfForce, [&] {
        (void)hipLaunchKernel(fixed_sweep_kernel(sweep_side(c), ctl != nullptr), grid, dim3(kHermiteWaves * 64), args, 0, sh.compute);
    }, ctl == nullptr));
    if (!ctl) note_interactions(c, sh, (double)sh.count * (double)c->in.slots);
    return 0;
}

// ---- a call's points, launch by launch: what the point read-outs and the tracers share (the planning: murb_field.h) -----------
// Workgroups the chip holds at once: of the active sweep (32 KiB of LDS each: 5 per CU) ...
inline int block_grid(const murbhip_ctx* c) { return 5 * std::max(c->in.cu_count, 1); }
// ... and of a sweep that runs 4 waves per SIMD, 4 resident workgroups per CU: every sweep over packed points, and the active sweep
// with a side product.  murb_field_cut's grid_full.
inline long sweep_grid(const murbhip_ctx* c) { return block_grid(c) / 5 * 4; }

// The plan of every such call.  Its points go to the device in launches of at most `batch` points, synchronously on the compute
// stream.  A launch's points [first, first + bn) are staged (stage_points), packed into records in whole groups of
// MURB_FIELD_GROUP (`padded` of them: the filler records are swept and never read back), swept by a grid that murb_field_cut
// sizes, and their partial rows folded by the read-out's rows kernel; only the last launch is ragged.  Every buffer of a launch
// is sized by `cap`, the largest launch's points in whole groups, so a plane of staged input or of results starts at k * cap.
struct Launch {
    unsigned long first, bn, padded;
};
// for (const Launch ln : Launches{count, batch})
struct Launches {
    unsigned long count, batch;
    struct Iterator {
        unsigned long count, batch, first;
        Launch operator*() const
        {
            const unsigned long bn = std::min(batch, count - first);
            return Launch{first, bn, murb_field_padded(bn)};
        }
        void operator++() { first += batch; }
        bool operator!=(const Iterator&) const { return first < count; }
    };
    Iterator begin() const { return Iterator{count, batch, 0ul}; }
    Iterator end() const { return Iterator{count, batch, count}; }
};

struct PointCall {
    Shard* sh = nullptr;
    MurbFieldLayout l{};
    unsigned long count = 0, batch = 0;
    size_t cap = 0;
    long grid_full = 0;
    std::vector<float> host;   // host_planes planes of `cap` floats, zeroed: a launch's input on its way up, and the caller's to use after
    std::vector<int> order;    // "all bodies in order" of one launch
    Launches launches() const { return Launches{count, batch}; }
};

// The plan of a call of `count` points under layout `l`, in launches of `batch` points.  prepare: wait for enqueued work and select
// the device first; false where the caller has, and has enqueued what the sweep reads since.
int point_call(murbhip_ctx* c, bool prepare, const MurbFieldLayout& l, unsigned long batch, unsigned long count, size_t host_planes,
               PointCall& pc)
{
    pc.sh = &c->shards[0];
    if (prepare) {
        RC_TRY(murbhip_sync(c));
        HIP_TRY(hipSetDevice(pc.sh->device));
    }
    pc.l = l;
    pc.count = count;
    pc.batch = batch;
    pc.cap = std::min<unsigned long>(batch, murb_field_padded(count));
    pc.grid_full = sweep_grid(c);
    pc.host.assign(host_planes * pc.cap, 0.f);
    return 0;
}
inline MurbFieldLayout field_layout(const murbhip_ctx* c) { return murb_field_layout(c->in.n, c->field_chunks, c->field_batch); }
// ... under "field_chunks" / "field_batch", as every read-out but the pair separations' cuts its calls
int field_call(murbhip_ctx* c, bool prepare, unsigned long count, size_t host_planes, PointCall& pc)
{
    const MurbFieldLayout l = field_layout(c);
    return point_call(c, prepare, l, l.batch, count, host_planes, pc);
}

// A launch's input on the device: `in` the float planes at stride cap (null: the points are bodies), `idx` an int per point (the
// bodies, or the body each point skips; null: none).
struct StagedPoints {
    const float* in;
    const int* idx;
};
constexpr int kFieldIntPlane = 6;   // of fld_in's 7 planes: six of floats, then the ints

// Brings launch `ln` of the call to `dev`, a buffer of the caller's with int_plane + 1 planes or more.  of_bodies false: the
// `nplanes` host planes (a null one stays zero) go to planes [0, nplanes) in one copy, and idx, where set, holds a skip per point.
// of_bodies true: idx lists the bodies, null standing for all bodies in order (point i is body i).  The ints go to plane
// int_plane, and stay there until the next launch is staged: murbsplit_of's hook reads the launch's bodies from it.
int stage_points(PointCall& pc, const Launch& ln, const float* const* planes, int nplanes, const int* idx, bool of_bodies, float* dev,
                 int int_plane, StagedPoints& st)
{
    const size_t cap = pc.cap;
    if (!of_bodies) {
        for (int k = 0; k < nplanes; ++k)
            if (planes[k]) std::memcpy(pc.host.data() + k * cap, planes[k] + ln.first, ln.bn * sizeof(float));
        HIP_TRY(hipMemcpy(dev, pc.host.data(), nplanes * cap * sizeof(float), hipMemcpyHostToDevice));
    }
    const int* list = idx ? idx + ln.first : nullptr;
    if (of_bodies && !idx) {
        pc.order.resize(ln.bn);
        for (unsigned long e = 0; e < ln.bn; ++e) pc.order[e] = (int)(ln.first + e);
        list = pc.order.data();
    }
    int* const dev_idx = (int*)(dev + int_plane * cap);
    if (list) HIP_TRY(hipMemcpy(dev_idx, list, ln.bn * sizeof(int), hipMemcpyHostToDevice));
    st.in = of_bodies ? nullptr : dev;
    st.idx = list ? dev_idx : nullptr;
    return 0;
}

// `count` staged points as `padded` packed records at pts (murb_field_pack_kernel: position, velocity where has_vel, the int)
int pack_points(murbhip_ctx* c, Shard& sh, const StagedPoints& st, float4* pts, unsigned long count, unsigned long padded, size_t in_stride,
                bool has_vel)
{
    MurbFieldPackArgs pa{};
    pa.in = st.in;
    pa.idx = st.idx;
    pa.rec = sh.rec[c->cur];
    pa.vel = sh.vel;
    pa.pts = pts;
    pa.count = (int)count;
    pa.padded = (int)padded;
    pa.in_stride = (unsigned int)in_stride;
    pa.has_vel = has_vel ? 1 : 0;
    hipLaunchKernelGGL(murb_field_pack_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, sh.compute, pa);
    return hip_rc(hipGetLastError());
}

// ---- massless tracers (include/murbtracer.h; kernels: murb_kernels_tracer.h, host logic: murb_tracer.h) ----------------------
// Resident beside the bodies on the one shard, carried by the Hermite steps on the compute stream, enqueue-only.  Everything
// they write is their own; of the context they read the records and velocities a sweep is made at, and soft2.
inline MurbFieldLayout tracer_layout(const murbhip_ctx* c) { return murb_field_layout(c->in.n, c->tracer_chunks, c->tracer_batch); }

// room for `count` tracers; the caller has waited for enqueued work where buffers are replaced
int ensure_tracers(Shard& sh, unsigned long count)
{
    const size_t cap = murb_field_padded(count);
    if (cap <= sh.trc_cap) return 0;
    shard_free(sh, sh.trc_state, 18 * sh.trc_cap * sizeof(float));
    shard_free(sh, sh.trc_pts, 2 * sh.trc_cap * sizeof(float4));
    sh.trc_cap = 0;
    RC_TRY(shard_alloc(sh, sh.trc_state, 18 * cap * sizeof(float)));   // q, v: the upload fills them; the rest is written before it is read
    RC_TRY(shard_alloc(sh, sh.trc_pts, 2 * cap * sizeof(float4)));
    sh.trc_cap = cap;
    return 0;
}

// the partial rows of one launch under the options in force ("tracer_chunks" may have grown since the last sweep)
int ensure_tracer_rows(murbhip_ctx* c, Shard& sh)
{
    const MurbFieldLayout l = tracer_layout(c);
    const size_t rows = std::min<size_t>(l.batch, murb_field_padded(c->tracers)) * (size_t)l.chunks;
    if (rows <= sh.trc_rows) return 0;
    HIP_TRY(hipStreamSynchronize(sh.compute));   // an enqueued rows kernel may still read the old ones
    shard_free(sh, sh.trc_part, 2 * sh.trc_rows * sizeof(float4));
    sh.trc_rows = 0;
    RC_TRY(shard_alloc(sh, sh.trc_part, 2 * rows * sizeof(float4)));
    sh.trc_rows = rows;
    return 0;
}

MurbTracerArgs tracer_args(const murbhip_ctx* c, const Shard& sh, float dt, int predict)
{
    MurbTracerArgs a{};
    const size_t cap = sh.trc_cap;
    a.q = sh.trc_state;
    a.v = sh.trc_state + 3 * cap;
    a.a0 = sh.trc_state + 6 * cap;
    a.j0 = sh.trc_state + 9 * cap;
    a.a1 = sh.trc_state + 12 * cap;
    a.j1 = sh.trc_state + 15 * cap;
    a.pts = sh.trc_pts;
    a.count = (int)c->tracers;
    a.padded = (int)murb_field_padded(c->tracers);
    a.stride = (unsigned int)cap;
    a.dt = dt;
    a.predict = predict;
    a.fold_dt = c->tracer_dt;
    return a;
}

// the tracers' predicted records (predict 1) or their current ones (0) into trc_pts
int enqueue_tracer_predict(murbhip_ctx* c, Shard& sh, float dt, int predict, const MurbEvolveCtl* ctl = nullptr)
{
    RC_TRY(ensure_tracer_rows(c, sh));
    const MurbTracerArgs a = tracer_args(c, sh, dt, predict);
    hipLaunchKernelGGL(murb_tracer_predict_kernel, dim3((unsigned)((a.padded + 255) / 256)), dim3(256), 0, sh.compute, a, ctl);
    return hip_rc(hipGetLastError());
}

// (a, j) of the records in trc_pts against the bodies' state (rec, vel), in launches of at most "tracer_batch" tracers, each
// with its row sum: into (a1, j1), or into (a0, j0) for an evaluation at the current state.  `ctl`: the control-block form of
// an adaptive step, which records no timing span.
int enqueue_tracer_sweeps(murbhip_ctx* c, Shard& sh, const float4* rec, const float4* vel, bool evaluation, const MurbEvolveCtl* ctl = nullptr)
{
    const MurbFieldLayout l = tracer_layout(c);
    const MurbTracerArgs a = tracer_args(c, sh, 0.f, 0);
    float* const out_a = evaluation ? a.a0 : a.a1;
    float* const out_j = evaluation ? a.j0 : a.j1;
    const long grid_full = sweep_grid(c);
    for (const Launch ln : Launches{c->tracers, l.batch}) {
        const MurbFieldCut cut = murb_field_cut(l, ln.padded, grid_full, false);   // a sum: the layout's chunks whatever the launch holds
        MurbTracerSweepArgs s{};
        s.rec = rec;
        s.vel = vel;
        s.pts = sh.trc_pts + 2 * ln.first;   // first + padded <= trc_cap: only the last launch is ragged
        s.part_a = sh.trc_part;
        s.part_j = sh.trc_part + sh.trc_rows;
        s.groups = cut.groups;
        s.chunks = cut.chunks;
        s.tiles = l.tiles;
        s.stride = (unsigned int)ln.padded;   // chunks * padded <= trc_rows
        s.soft2 = c->soft2;
        RC_TRY(timed_launch(c, sh, kProfTracer, [&] {
            hipLaunchKernelGGL((murb_tracer_sweep_kernel<4, 4, 2>), dim3((unsigned)cut.grid), dim3(256), 0, sh.compute, s, ctl);
        }, ctl == nullptr));
        hipLaunchKernelGGL(murb_tracer_rows_kernel, dim3((unsigned)((ln.bn + 255) / 256)), dim3(256), 0, sh.compute, (const float4*)s.part_a,
                           (const float4*)s.part_j, out_a + ln.first, out_j + ln.first, (int)ln.bn, s.chunks, s.stride, a.stride, ctl);
        RC_TRY(hip_rc(hipGetLastError()));
    }
    return 0;
}

// make sure the tracers' (a0, j0) are those of the current state; never touches the bodies' remembered evaluation
int enqueue_tracer_evaluation(murbhip_ctx* c, Shard& sh)
{
    if (!c->tracers || c->trc_current) return 0;
    RC_TRY(enqueue_tracer_predict(c, sh, 0.f, 0));
    RC_TRY(enqueue_tracer_sweeps(c, sh, sh.rec[c->cur], sh.vel, true));
    c->trc_current = true;
    return 0;
}

int enqueue_tracer_correct(murbhip_ctx* c, Shard& sh, float dt, MurbEvolveCtl* ctl = nullptr)
{
    const MurbTracerArgs a = tracer_args(c, sh, dt, 1);
    hipLaunchKernelGGL(murb_tracer_correct_kernel, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, sh.compute, a, ctl);
    return hip_rc(hipGetLastError());
}

// update_state 0: make sure (a0, j0) of the current state are remembered; 1: one step.
int enqueue_hermite(murbhip_ctx* c, float dt, int update_state)
{
    if (c->in.world != 1 || c->shards.size() != 1 || c->force_exchange) return MURBHIP_E_STATE;
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    const int parts = hermite_parts(c->in);
    RC_TRY(ensure_hermite(c, sh, parts));
    if (c->gather_pending) HIP_TRY(hipStreamWaitEvent(sh.compute, sh.ev_gathered, 0));
    const unsigned pairs = (unsigned)(c->in.slots / 2);
    if (!c->herm_current) {
        RC_TRY(enqueue_hermite_sweep(c, sh, sh.rec[c->cur], sh.vel, parts));
        const MurbHermiteArgs a = hermite_args(c, sh, parts, 0.f, 0);
        hipLaunchKernelGGL(murb_hermite_correct_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, a);
        RC_TRY(hip_rc(hipGetLastError()));
        c->acc_current = false;   // acc_out now holds this sweep's accelerations, not the force plan's
        c->pe_current = false;
        c->herm_current = true;
        c->herm_in_acc_out = true;
    }
    if (!update_state) {
        if (!c->herm_in_acc_out) {   // a force evaluation has used acc_out since: murbhip_download_acc is to return THIS evaluation's
            HIP_TRY(hipMemcpyAsync(sh.acc_out, sh.herm_a0, 3 * c->in.slots * sizeof(float), hipMemcpyDeviceToDevice, sh.compute));
            c->acc_current = false;
            c->pe_current = false;
            c->herm_in_acc_out = true;
        }
        return 0;
    }
    const bool tracers = c->tracers != 0;   // carried along (murbtracer.h): their launches behind the bodies' of the same kind
    RC_TRY(enqueue_tracer_evaluation(c, sh));
    MurbHermiteArgs a = hermite_args(c, sh, parts, dt, 1);
    a.rec_out = sh.herm_rec;
    a.vel_out = sh.herm_vel;
    hipLaunchKernelGGL(murb_hermite_predict_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, a);
    RC_TRY(hip_rc(hipGetLastError()));
    if (tracers) RC_TRY(enqueue_tracer_predict(c, sh, dt, 1));
    RC_TRY(enqueue_hermite_sweep(c, sh, sh.herm_rec, sh.herm_vel, parts));
    if (tracers) RC_TRY(enqueue_tracer_sweeps(c, sh, sh.herm_rec, sh.herm_vel, false));   // at the bodies' PREDICTED state
    a.rec_out = sh.rec[c->cur ^ 1];
    a.vel_out = nullptr;
    hipLaunchKernelGGL(murb_hermite_correct_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, a);
    RC_TRY(hip_rc(hipGetLastError()));
    if (tracers) RC_TRY(enqueue_tracer_correct(c, sh, dt));
    c->cur ^= 1;
    invalidate_cached_forces(c);
    c->herm_current = true;   // (a1, j1) of this step are the next step's (a0, j0)
    c->herm_in_acc_out = true;
    c->trc_current = tracers; // ... for the tracers too
    return 0;
}

// ---- shared adaptive steps (murbhip_evolve; control block and kernels: murb_kernels_adaptive.h) -------------------------
constexpr int kEvolveBatch = 64;                              // steps enqueued between two looks at the control block
constexpr size_t kEvolveHead = offsetof(MurbEvolveCtl, ring);   // what the host reads back after a batch

// One adaptive step: enqueue_hermite's three launches in their control-block form, and the bookkeeping launch.  Whether
// the device still takes the step or has finished, the records end up in the other position buffer.
int enqueue_hermite_adaptive(murbhip_ctx* c, Shard& sh, int parts)
{
    const unsigned pairs = (unsigned)(c->in.slots / 2);
    MurbHermiteArgs a = hermite_args(c, sh, parts, 0.f, 1);
    a.rec_out = sh.herm_rec;
    a.vel_out = sh.herm_vel;
    const bool tracers = c->tracers != 0;   // murbtracer.h: every tracer launch reads dt and `done` from the control block too
    hipLaunchKernelGGL(murb_hermite_predict_adaptive_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, a, sh.herm_ctl);
    RC_TRY(hip_rc(hipGetLastError()));
    if (tracers) RC_TRY(enqueue_tracer_predict(c, sh, 0.f, 1, sh.herm_ctl));
    RC_TRY(enqueue_hermite_sweep(c, sh, sh.herm_rec, sh.herm_vel, parts, sh.herm_ctl));
    if (tracers) RC_TRY(enqueue_tracer_sweeps(c, sh, sh.herm_rec, sh.herm_vel, false, sh.herm_ctl));
    a.rec_out = sh.rec[c->cur ^ 1];
    a.vel_out = nullptr;
    hipLaunchKernelGGL(murb_hermite_correct_adaptive_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, a, sh.herm_ctl);
    RC_TRY(hip_rc(hipGetLastError()));
    if (tracers) RC_TRY(enqueue_tracer_correct(c, sh, 0.f, sh.herm_ctl));   // in front of the bookkeeping: its minimum is folded by then
    hipLaunchKernelGGL(murb_evolve_book_kernel, dim3(1), dim3(1), 0, sh.compute, sh.herm_ctl);
    RC_TRY(hip_rc(hipGetLastError()));
    c->cur ^= 1;
    return 0;
}

// ---- individual block time steps (murbhip_evolve_block; control block and kernels: murb_kernels_block.h) ----------------------
constexpr int kBlockBatch = 64;        // block steps enqueued between two looks at the control block
constexpr int kBlockMaxUnits = 65536;  // "block_units"

// The default "block_units": one unit per workgroup of the active sweep that the chip holds at once (block_grid).
inline int block_units(const murbhip_ctx* c) { return c->block_units > 0 ? c->block_units : block_grid(c); }

int ensure_block(murbhip_ctx* c, Shard& sh)
{
    const size_t slots = c->in.slots;
    RC_TRY(shard_alloc(sh, sh.blk_ctl, sizeof(MurbBlockCtl), sh.compute));
    if (!sh.blk_ctl_host) HIP_TRY(hipHostMalloc((void**)&sh.blk_ctl_host, sizeof(MurbBlockCtl), hipHostMallocDefault));
    RC_TRY(shard_alloc(sh, sh.blk_ticks, slots * sizeof(unsigned int), sh.compute));
    RC_TRY(shard_alloc(sh, sh.blk_levels, slots * sizeof(int), sh.compute));
    RC_TRY(shard_alloc(sh, sh.blk_list, slots * sizeof(int), sh.compute));
    for (float4** p : {&sh.blk_rec, &sh.blk_vel}) RC_TRY(shard_alloc(sh, *p, slots * sizeof(float4), sh.compute));
    // groups * chunks <= max(groups, units + groups - 1) with chunks = ceil(units / groups) clamped, and 16 * groups <= slots
    const size_t rows = slots + (size_t)MURB_BLOCK_GROUP * (size_t)block_units(c);
    if (rows > sh.blk_rows) {   // "block_units" grew: no step is in flight between two calls, but the stream may still run
        HIP_TRY(hipStreamSynchronize(sh.compute));
        shard_free(sh, sh.blk_part, 2 * sh.blk_rows * sizeof(float4));
        sh.blk_rows = 0;
        RC_TRY(shard_alloc(sh, sh.blk_part, 2 * rows * sizeof(float4), sh.compute));
        sh.blk_rows = rows;
    }
    return 0;
}

MurbBlockArgs block_args(const murbhip_ctx* c, const Shard& sh)
{
    MurbBlockArgs a{};
    a.rec = sh.rec[c->cur];
    a.vel = sh.vel;
    a.rec_pred = sh.herm_rec;
    a.vel_pred = sh.herm_vel;
    a.rec_act = sh.blk_rec;
    a.vel_act = sh.blk_vel;
    a.a0 = sh.herm_a0;
    a.j0 = sh.herm_j0;
    a.acc_out = sh.acc_out;
    a.part_a = sh.blk_part;
    a.part_j = sh.blk_part + sh.blk_rows;
    a.ticks = sh.blk_ticks;
    a.levels = sh.blk_levels;
    a.list = sh.blk_list;
    side_slots(c, sh, a);
    a.count = (int)sh.count;
    a.stride = (unsigned int)c->in.slots;
    a.soft2 = c->soft2;
    return a;
}

// One block step: six launches of fixed size, whatever the device makes of them (nothing, once `done` is set).
int enqueue_block_step(murbhip_ctx* c, Shard& sh, const MurbBlockArgs& a)
{
    const unsigned per_body = (unsigned)((sh.count + 255) / 256), per_pair = (unsigned)((c->in.slots / 2 + 255) / 256);
    hipLaunchKernelGGL(murb_block_min_kernel, dim3(per_body), dim3(256), 0, sh.compute, a, sh.blk_ctl);
    hipLaunchKernelGGL(murb_block_predict_kernel, dim3(per_pair), dim3(256), 0, sh.compute, a, sh.blk_ctl);
    hipLaunchKernelGGL(murb_block_plan_kernel, dim3(1), dim3(1), 0, sh.compute, sh.blk_ctl);
    const MurbSide side = sweep_side(c);
    MurbBlockNNSweepArgs na{};   // the plain sweep takes its base
    na.rec_pred = a.rec_pred; na.vel_pred = a.vel_pred; na.soft2 = a.soft2; na.count = a.count;
    na.grid = side == MurbSide::None ? block_grid(c) : (int)sweep_grid(c);
    na.ctl = sh.blk_ctl;
    const MurbBlockCtl* ctl = sh.blk_ctl;
    void* args[] = {&na, &ctl};   // an error of this launch shows in hipGetLastError below, like the others'
    (void)hipLaunchKernel(active_sweep_kernel(side), dim3((unsigned)na.grid), dim3(kHermiteWaves * 64), args, 0, sh.compute);
    hipLaunchKernelGGL(murb_block_correct_kernel, dim3(per_body), dim3(256), 0, sh.compute, a, sh.blk_ctl);
    hipLaunchKernelGGL(murb_block_book_kernel, dim3(1), dim3(1), 0, sh.compute, sh.blk_ctl);
    return hip_rc(hipGetLastError());
}

// The compute streams of a shard.  reserve > 0: created with a CU mask that leaves out the `reserve` highest-numbered
// CUs.  The force kernels fill every CU they may use (4 waves per SIMD, 120 VGPRs each), and stream priority does
// not pre-empt resident workgroups: a collective's kernel would otherwise wait for a workgroup to retire before it can
// start.  Bit b of the mask is CU b / 8 of XCD b % 8 (the driver deals the mask's bits to the XCDs round-robin), so
// 8 reserved CUs are one per XCD, 16 two per XCD.  hipExtStreamCreateWithCUMask has no flags argument: such a stream
// has default priority and the default (blocking with respect to stream 0) flag — the library never uses stream 0, but a
// host application that does (torch's default stream) then synchronises with the force kernels implicitly
// (include/murbhip.h, "cu_reserve").  The low-priority stream of "overlap" 2 stays unmasked so that it keeps its priority.
int create_compute_streams(const murbhip_ctx* c, Shard& sh, int reserve, int* highest_priority = nullptr)
{
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (highest_priority) *highest_priority = greatest;
    HIP_TRY(hipStreamCreateWithPriority(&sh.compute_low, hipStreamNonBlocking, least));
    if (reserve > 0 && c->in.cu_count > reserve) {
        std::vector<uint32_t> mask((size_t)(c->in.cu_count + 31) / 32, 0u);
        for (int b = 0; b < c->in.cu_count - reserve; ++b) mask[(size_t)b / 32] |= 1u << (b % 32);
        HIP_TRY(hipExtStreamCreateWithCUMask(&sh.compute, (uint32_t)mask.size(), mask.data()));
        return 0;
    }
    HIP_TRY(hipStreamCreateWithFlags(&sh.compute, hipStreamNonBlocking));
    return 0;
}

int create_common(murbhip_ctx** out, unsigned long n, float soft, float g, int world, int nlocal, const int* devices,
                  const int* ranks, int exchange, bool rank_mode)
{
    if (!out || n == 0 || world < 1 || world > MURB_SYM_MAX_RANKS || nlocal < 1 || !(soft == soft)) return MURBHIP_E_INVALID;
    if (!(g > 0.f) || !std::isfinite(g)) return MURBHIP_E_INVALID;   // murbhip_energy divides by it; G*m is folded into the records
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MURBHIP_E_NO_DEVICE;
    for (int i = 0; i < nlocal; ++i)
        if (devices[i] < 0 || devices[i] >= ndev) return MURBHIP_E_INVALID;
    if (slice_slots(n, world) * (unsigned long)world > 0x7fffffffUL) return MURBHIP_E_INVALID;

    murbhip_ctx* c = new (std::nothrow) murbhip_ctx;
    if (!c) return MURBHIP_E_NOMEM;
    c->in.n = n;
    c->in.world = world;
    c->in.slice = slice_slots(n, world);
    c->in.slots = c->in.slice * (unsigned long)world;
    c->soft2 = soft * soft;
    c->g = g;
    c->exchange = exchange;
    c->rank_mode = rank_mode;
    c->shards.resize(nlocal);

    hipDeviceProp_t prop;
    int rc = hip_rc(hipGetDeviceProperties(&prop, devices[0]));
    if (rc == 0) { c->in.cu_count = prop.multiProcessorCount; c->clock_mhz = prop.clockRate / 1000; c->in.device_mem = prop.totalGlobalMem; }

    for (int i = 0; rc == 0 && i < nlocal; ++i) {
        Shard& sh = c->shards[i];
        sh.device = devices[i];
        sh.rank = ranks[i];
        partition(n, world, sh.rank, &sh.first, &sh.count);
        if ((rc = hip_rc(hipSetDevice(sh.device)))) break;
        int greatest = 0;
        if ((rc = create_compute_streams(c, sh, 0, &greatest))) break;
        // the exchange stream gets the highest priority: its (few, small) collective kernels must be
        // dispatched as soon as they are ready although the force kernel keeps every CU full
        if ((rc = hip_rc(hipStreamCreateWithPriority(&sh.comm, hipStreamNonBlocking, greatest)))) break;
        if ((rc = hip_rc(hipEventCreateWithFlags(&sh.ev_tri, hipEventDisableTiming)))) break;
        if ((rc = hip_rc(hipEventCreateWithFlags(&sh.ev_integrated, hipEventDisableTiming)))) break;
        if ((rc = hip_rc(hipEventCreateWithFlags(&sh.ev_gathered, hipEventDisableTiming)))) break;
        const size_t rec_bytes = c->in.slots * sizeof(float4);
        const size_t vel_bytes = c->in.slice * sizeof(float4);
        const size_t acco_bytes = 3 * c->in.slice * sizeof(float);
        if ((rc = shard_alloc(sh, sh.rec[0], rec_bytes))) break;
        if ((rc = shard_alloc(sh, sh.rec[1], rec_bytes))) break;
        if ((rc = shard_alloc(sh, sh.vel, vel_bytes))) break;
        if ((rc = shard_alloc(sh, sh.acc_out, acco_bytes))) break;
        if ((rc = hip_rc(hipMemset(sh.acc_out, 0, acco_bytes)))) break;
    }
    // peer access for the copy exchange between distinct devices
    if (rc == 0 && world > 1 && !rank_mode && exchange == 0) {
        for (Shard& a : c->shards)
            for (Shard& b : c->shards)
                if (a.device != b.device) {
                    int can = 0;
                    if ((rc = hip_rc(hipSetDevice(a.device)))) break;
                    if (hipDeviceCanAccessPeer(&can, a.device, b.device) == hipSuccess && can) {
                        hipError_t e = hipDeviceEnablePeerAccess(b.device, 0);
                        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) rc = hip_rc(e);
                        (void)hipGetLastError();
                    }
                }
    }
    if (rc != 0) { murbhip_destroy(c); return rc; }
    {   // after the shards exist: the members bind to their devices at once
        std::vector<int> devs;
        for (const Shard& sh : c->shards) devs.push_back(sh.device);
        c->crew = new (std::nothrow) ShardCrew((int)devs.size(), [devs](int i) { (void)hipSetDevice(devs[(size_t)i]); });
    }
    if (!c->crew) { murbhip_destroy(c); return MURBHIP_E_NOMEM; }
    *out = c;
    return 0;
}

// The four values of body slot `slot` in packed records (murb_layout.h), as offsets from the returned pointer.
constexpr size_t kSlotX = 0, kSlotY = 2, kSlotZ = 4 * MURB_TILE_PAIRS, kSlotW = kSlotZ + 2;
template <class F4>
auto* slot_values(F4* recs, unsigned long slot)
{
    using F = std::conditional_t<std::is_const_v<F4>, const float, float>;
    return reinterpret_cast<F*>(recs + murb_rec_a(slot >> 1)) + (slot & 1);
}

// host SoA -> pair records for all slots
void pack_records(const float* x, const float* y, const float* z, const float* w, float scale_w, bool w_present, unsigned long first_body,
                  unsigned long nbodies, unsigned long first_slot, std::vector<float4>& out)
{
    // writes bodies [first_body, first_body + nbodies) at slots first_slot..; caller zero-fills `out`
    for (unsigned long k = 0; k < nbodies; ++k) {
        const unsigned long body = first_body + k;
        float* const v = slot_values(out.data(), first_slot + k);
        v[kSlotX] = x[body];
        v[kSlotY] = y[body];
        v[kSlotZ] = z[body];
        v[kSlotW] = w_present ? scale_w * w[body] : 0.f;
    }
}

// A fresh set of bodies is on the device (murbhip_upload, murbhip_init_bodies).
void bodies_loaded(murbhip_ctx* c)
{
    for (Shard& sh : c->shards) sh.prof_used = 0;
    c->cur = 0;
    c->gather_pending = false;
    c->uploaded = true;
    c->lf_half = false;
    invalidate_cached_forces(c);
}

// "contact": the bodies' radii into the two spare lanes of the velocity B records (0 with the option off or no radii set), on
// the compute stream.  One shard; runs at the option's switch and wherever the velocity records or the radii are replaced.
int enqueue_radii_lanes(murbhip_ctx* c)
{
    if (!c->uploaded || c->shards.size() != 1 || c->in.world != 1) return 0;
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    const unsigned pairs = (unsigned)(c->in.slots / 2);
    hipLaunchKernelGGL(murb_radii_lanes_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, sh.vel,
                       c->contact ? (const float*)sh.radius : (const float*)nullptr, (int)sh.count, (unsigned int)c->in.slots);
    return hip_rc(hipGetLastError());
}

// "nearest", "contact", "potential": the side products of the Hermite sweeps.  One shard under "integrator" 2; at most one of
// them at a time, because all three use the rows' fourth floats (and two of them the per-slot arrays); no change of form
// while a block is open, whose inactive bodies have their side product or do not (with "contact": whose velocity records
// carry the radii or do not); and a change drops the remembered forces: a remembered (a0, j0) always has its side product
// beside it.  The order of the checks decides which error a refused call reports.
int set_side_option(murbhip_ctx* c, const std::string& k, long value)
{
    const bool nearest = k == "nearest", contact = k == "contact";
    int& field = nearest ? c->nearest : contact ? c->contact : c->potential;
    if (value < 0 || value > (contact ? 2 : 1)) return MURBHIP_E_INVALID;   // "contact" 2: with the contact stop
    if (c->integrator != 2 || c->in.world != 1 || c->shards.size() != 1) return MURBHIP_E_STATE;
    if (value && c->nearest + c->contact + c->potential != field) return MURBHIP_E_STATE;   // another one is on
    if (nearest && !value && c->enc_radius > 0.f) return MURBHIP_E_STATE;   // the encounter stop reads the neighbours: murbhip_set_encounter(0) first
    if ((field != 0) != (value != 0)) {
        if (c->blk_open) return MURBHIP_E_STATE;
        field = (int)value;
        if (contact) c->enc_count = 0;
        invalidate_cached_forces(c);
        if (contact) RC_TRY(enqueue_radii_lanes(c));
    }
    field = (int)value;   // "contact" 1 <-> 2: only the stop; the evaluation and an open block stay
    return 0;
}

// The hit list of the last evolve call (encounters or contacts: the options exclude each other), sorted by i.
int read_hit_list(murbhip_ctx* c, bool mine, int* i, int* j, float* v, unsigned long capacity, unsigned long* count, double* time)
{
    const unsigned long hits = mine ? c->enc_count : 0ul;
    *count = hits;
    if (time) *time = c->enc_time;
    const unsigned long kept = std::min<unsigned long>(hits, MURB_ENC_CAP);
    if ((!i && !j && !v) || kept == 0) return 0;
    if (capacity < kept) return MURBHIP_E_INVALID;
    Shard& sh = c->shards[0];
    if (!sh.enc) return MURBHIP_E_STATE;
    RC_TRY(murbhip_sync(c));
    HIP_TRY(hipSetDevice(sh.device));
    std::vector<int> li(kept), lj(kept);
    std::vector<float> lr(kept);
    HIP_TRY(hipMemcpy(li.data(), sh.enc->i, kept * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lj.data(), sh.enc->j, kept * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lr.data(), sh.enc->r2, kept * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<unsigned long> order(kept);   // the device's order is that of its atomics: sort by i
    for (unsigned long k = 0; k < kept; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](unsigned long a, unsigned long b) { return li[a] < li[b]; });
    for (unsigned long k = 0; k < kept; ++k) {
        if (i) i[k] = li[order[k]];
        if (j) j[k] = lj[order[k]];
        if (v) v[k] = lr[order[k]];
    }
    return 0;
}

// ---- field read-out (murbfield_at / murbfield_of; kernels: murb_kernels_field.h, planning: murb_field.h) ----------
// Synchronous, on the compute stream, in launches of at most "field_batch" points.  Everything it writes is its own: the
// uploaded points, their packed records, the partial rows and the results.  Of the context it reads rec[cur], vel and soft2.
int ensure_field(Shard& sh, size_t points, size_t rows)
{
    if (points > sh.fld_points) {
        shard_free(sh, sh.fld_in, 7 * sh.fld_points * sizeof(float));
        shard_free(sh, sh.fld_pts, 2 * sh.fld_points * sizeof(float4));
        shard_free(sh, sh.fld_out, 7 * sh.fld_points * sizeof(float));
        sh.fld_points = 0;
        RC_TRY(shard_alloc(sh, sh.fld_in, 7 * points * sizeof(float)));
        RC_TRY(shard_alloc(sh, sh.fld_pts, 2 * points * sizeof(float4)));
        RC_TRY(shard_alloc(sh, sh.fld_out, 7 * points * sizeof(float)));
        sh.fld_points = points;
    }
    if (rows > sh.fld_rows) {
        shard_free(sh, sh.fld_part, 2 * sh.fld_rows * sizeof(float4));
        sh.fld_rows = 0;
        RC_TRY(shard_alloc(sh, sh.fld_part, 2 * rows * sizeof(float4)));
        sh.fld_rows = rows;
    }
    return 0;
}

// What both entry points share once their arguments are checked.  p: the six input planes (murbfield_at; p[3..5] null:
// at rest) or all null (murbfield_of: idx are the bodies); out: ax ay az jx jy jz phi, null where not asked for.
int field_run(murbhip_ctx* c, unsigned long count, const float* const* p, const int* idx, bool of_bodies, float* const (&out)[7])
{
    PointCall pc;
    RC_TRY(field_call(c, true, count, 7, pc));
    Shard& sh = *pc.sh;
    const size_t cap = pc.cap;
    RC_TRY(ensure_field(sh, cap, cap * (size_t)pc.l.chunks));
    const bool has_vel = p && p[3];
    for (const Launch ln : pc.launches()) {
        StagedPoints st;
        RC_TRY(stage_points(pc, ln, p, has_vel ? 6 : 3, idx, of_bodies, sh.fld_in, kFieldIntPlane, st));
        RC_TRY(pack_points(c, sh, st, sh.fld_pts, ln.bn, ln.padded, cap, has_vel));
        const MurbFieldCut cut = murb_field_cut(pc.l, ln.padded, pc.grid_full, false);
        MurbFieldArgs fa{};
        fa.rec = sh.rec[c->cur];
        fa.vel = sh.vel;
        fa.pts = sh.fld_pts;
        fa.part_a = sh.fld_part;
        fa.part_j = sh.fld_part + sh.fld_rows;
        fa.groups = cut.groups;
        fa.chunks = cut.chunks;
        fa.tiles = pc.l.tiles;
        fa.stride = (unsigned int)ln.padded;   // chunks * padded <= fld_rows
        fa.soft2 = c->soft2;
        RC_TRY(timed_launch(c, sh, kProfField, [&] {
            hipLaunchKernelGGL((murb_force_field_kernel<kHermiteR, kHermiteWaves, kHermiteStage>), dim3((unsigned)cut.grid),
                               dim3(kHermiteWaves * 64), 0, sh.compute, fa);
        }));
        hipLaunchKernelGGL(murb_field_rows_kernel, dim3((unsigned)((ln.bn + 255) / 256)), dim3(256), 0, sh.compute,
                           (const float4*)fa.part_a, (const float4*)fa.part_j, sh.fld_out, (int)ln.bn, fa.chunks, fa.stride, (unsigned int)cap);
        RC_TRY(hip_rc(hipGetLastError()));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        int lo = 7, hi = 0;   // the planes the caller asked for: one copy from the first to the last of them
        for (int k = 0; k < 7; ++k)
            if (out[k]) { lo = std::min(lo, k); hi = k + 1; }
        float* const host = pc.host.data();
        if (lo < hi) HIP_TRY(hipMemcpy(host + lo * cap, sh.fld_out + lo * cap, (size_t)(hi - lo) * cap * sizeof(float), hipMemcpyDeviceToHost));
        for (int k = 0; k < 7; ++k)
            if (out[k]) std::memcpy(out[k] + ln.first, host + k * cap, ln.bn * sizeof(float));
    }
    return 0;
}

// ---- tidal read-out (murbtidal_at / murbtidal_of; kernels: murb_kernels_tidal.h) -----------------------------------
// Under "field_chunks" / "field_batch" and in the field read-out's own buffers (both calls are synchronous on the compute stream,
// so neither sees the other's rows).  p: the three position planes (murbtidal_at) or all null (murbtidal_of: idx are the
// bodies); out: txx tyy tzz txy txz tyz, all set or all null.
int tidal_run(murbhip_ctx* c, unsigned long count, const float* const* p, const int* idx, bool of_bodies, float* const (&out)[6])
{
    PointCall pc;
    RC_TRY(field_call(c, true, count, 6, pc));
    Shard& sh = *pc.sh;
    const size_t cap = pc.cap;
    RC_TRY(ensure_field(sh, cap, cap * (size_t)pc.l.chunks));
    for (const Launch ln : pc.launches()) {
        StagedPoints st;
        RC_TRY(stage_points(pc, ln, p, 3, idx, of_bodies, sh.fld_in, kFieldIntPlane, st));
        RC_TRY(pack_points(c, sh, st, sh.fld_pts, ln.bn, ln.padded, cap, false));
        const MurbFieldCut cut = murb_field_cut(pc.l, ln.padded, pc.grid_full, false);
        MurbTidalArgs ta{};
        ta.rec = sh.rec[c->cur];
        ta.pts = sh.fld_pts;
        ta.part_a = sh.fld_part;
        ta.part_b = sh.fld_part + sh.fld_rows;
        ta.groups = cut.groups;
        ta.chunks = cut.chunks;
        ta.tiles = pc.l.tiles;
        ta.stride = (unsigned int)ln.padded;   // chunks * padded <= fld_rows
        ta.soft2 = c->soft2;
        RC_TRY(timed_launch(c, sh, kProfTidal, [&] {
            hipLaunchKernelGGL((murb_tidal_sweep_kernel<kHermiteR, kHermiteWaves, kTidalStage>), dim3((unsigned)cut.grid),
                               dim3(kHermiteWaves * 64), 0, sh.compute, ta);
        }));
        hipLaunchKernelGGL(murb_tidal_rows_kernel, dim3((unsigned)((ln.bn + 255) / 256)), dim3(256), 0, sh.compute,
                           (const float4*)ta.part_a, (const float4*)ta.part_b, sh.fld_out, (int)ln.bn, ta.chunks, ta.stride, (unsigned int)cap);
        RC_TRY(hip_rc(hipGetLastError()));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        if (!out[0]) continue;
        HIP_TRY(hipMemcpy(pc.host.data(), sh.fld_out, 6 * cap * sizeof(float), hipMemcpyDeviceToHost));
        for (int k = 0; k < 6; ++k) std::memcpy(out[k] + ln.first, pc.host.data() + k * cap, ln.bn * sizeof(float));
    }
    return 0;
}

// ---- k nearest neighbours, densities, density centre (include/murbknn.h; kernels: murb_kernels_knn.h) --------------
constexpr int kKnnStage = 2;   // positions alone: 2 tiles of 8 KiB

template <typename T>
int grow(Shard& sh, T*& p, size_t& have, size_t want)
{
    if (want <= have) return 0;
    shard_free(sh, p, have * sizeof(T));
    have = 0;
    RC_TRY(shard_alloc(sh, p, want * sizeof(T)));
    have = want;
    return 0;
}

// A list of the k nearest bodies per point in the place of a sum, in the field read-out's point buffers, with lists and rows of
// its own.  p: the three position planes (murbknn_at) or null (of bodies: idx lists them, or null for all n in order).  out_idx,
// out_r2, out_rho: host arrays, null where not asked for; rho_all: the densities stay on the device, knn_rho[body]
// (murbdensity_centre; all bodies in order).
int knn_run(murbhip_ctx* c, int k, unsigned long count, const float* const* p, const int* idx, bool of_bodies, int* out_idx, float* out_r2,
            float* out_rho, bool rho_all)
{
    PointCall pc;
    RC_TRY(field_call(c, true, count, 3, pc));
    Shard& sh = *pc.sh;
    const size_t cap = pc.cap;
    const bool want_rho = out_rho || rho_all;
    RC_TRY(ensure_field(sh, cap, 0));
    {   // r2 and indices grow together: each pair shares one size
        const size_t part = cap * (size_t)pc.l.chunks * (size_t)k, list = cap * (size_t)k;
        size_t part_r2 = sh.knn_part, list_r2 = sh.knn_list;
        RC_TRY(grow(sh, sh.knn_part_r2, part_r2, part));
        RC_TRY(grow(sh, sh.knn_part_idx, sh.knn_part, part));
        RC_TRY(grow(sh, sh.knn_list_r2, list_r2, list));
        RC_TRY(grow(sh, sh.knn_list_idx, sh.knn_list, list));
        if (want_rho) RC_TRY(grow(sh, sh.knn_rho, sh.knn_rhos, rho_all ? std::max<size_t>(count, cap) : cap));
    }
    for (const Launch ln : pc.launches()) {
        StagedPoints st;
        RC_TRY(stage_points(pc, ln, p, 3, idx, of_bodies, sh.fld_in, kFieldIntPlane, st));
        RC_TRY(pack_points(c, sh, st, sh.fld_pts, ln.bn, ln.padded, cap, false));
        // a list does not depend on the cut, and every chunk starts its lists empty and pays the slow path's first trips again
        const MurbFieldCut cut = murb_field_cut(pc.l, ln.padded, pc.grid_full, true);
        MurbKnnArgs ka{};
        ka.rec = sh.rec[c->cur];
        ka.pts = sh.fld_pts;
        ka.part_r2 = sh.knn_part_r2;
        ka.part_idx = sh.knn_part_idx;
        ka.groups = cut.groups;
        ka.chunks = cut.chunks;
        ka.tiles = pc.l.tiles;
        ka.count = (int)c->in.n;
        ka.k = k;
        ka.stride = (unsigned int)ln.padded;   // chunks * padded * k <= knn_part
        ka.soft2 = c->soft2;
        RC_TRY(timed_launch(c, sh, kProfKnn, [&] {
            hipLaunchKernelGGL((murb_knn_sweep_kernel<kHermiteR, kHermiteWaves, kKnnStage>), dim3((unsigned)cut.grid),
                               dim3(kHermiteWaves * 64), 0, sh.compute, ka);
        }));
        const dim3 per_point((unsigned)((ln.bn + 255) / 256));
        hipLaunchKernelGGL(murb_knn_rows_kernel, per_point, dim3(256), 0, sh.compute, (const float*)ka.part_r2,
                           (const int*)ka.part_idx, sh.knn_list_idx, sh.knn_list_r2, (int)ln.bn, ka.chunks, ka.stride, k);
        float* const rho = want_rho ? sh.knn_rho + (rho_all ? ln.first : 0ul) : nullptr;
        if (rho)
            hipLaunchKernelGGL(murb_knn_density_kernel, per_point, dim3(256), 0, sh.compute, (const int*)sh.knn_list_idx,
                               (const float*)sh.knn_list_r2, (const float*)sh.mass, rho, (int)ln.bn, k, c->soft2);
        RC_TRY(hip_rc(hipGetLastError()));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        if (out_idx) HIP_TRY(hipMemcpy(out_idx + ln.first * k, sh.knn_list_idx, ln.bn * k * sizeof(int), hipMemcpyDeviceToHost));
        if (out_r2) HIP_TRY(hipMemcpy(out_r2 + ln.first * k, sh.knn_list_r2, ln.bn * k * sizeof(float), hipMemcpyDeviceToHost));
        if (out_rho) HIP_TRY(hipMemcpy(out_rho + ln.first, rho, ln.bn * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
}

// The density of every body, then the centre: two launches of block sums, their rows added on the host in index order.
int knn_centre(murbhip_ctx* c, int k, double* out8)
{
    const unsigned long n = c->in.n;
    RC_TRY(knn_run(c, k, n, nullptr, nullptr, true, nullptr, nullptr, nullptr, true));
    Shard& sh = c->shards[0];
    const size_t blocks = (n + 255) / 256;
    RC_TRY(grow(sh, sh.knn_sums, sh.knn_blocks, blocks * MURB_KNN_CENTRE_VALUES));
    std::vector<double> rows(blocks * MURB_KNN_CENTRE_VALUES);
    double sum[MURB_KNN_CENTRE_VALUES], x[3] = {0.0, 0.0, 0.0};
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(murb_knn_centre_kernel, dim3((unsigned)blocks), dim3(256), 0, sh.compute, (const float4*)sh.rec[c->cur],
                           (const float*)sh.knn_rho, sh.knn_sums, (int)n, pass, x[0], x[1], x[2]);
        RC_TRY(hip_rc(hipGetLastError()));
        HIP_TRY(hipMemcpyAsync(rows.data(), sh.knn_sums, rows.size() * sizeof(double), hipMemcpyDeviceToHost, sh.compute));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        double s[MURB_KNN_CENTRE_VALUES] = {0};
        for (size_t b = 0; b < blocks; ++b)
            for (int e = 0; e < MURB_KNN_CENTRE_VALUES; ++e) s[e] += rows[b * MURB_KNN_CENTRE_VALUES + e];
        if (pass == 0) {
            for (int e = 0; e < MURB_KNN_CENTRE_VALUES; ++e) sum[e] = s[e];
            for (int e = 0; e < 3; ++e) x[e] = sum[2 + e] / sum[0];
            out8[5] = sum[0];
            out8[6] = sum[5];
            out8[7] = (double)n - sum[5];
            if (sum[0] == 0.0) {
                for (int e = 0; e < 5; ++e) out8[e] = std::numeric_limits<double>::quiet_NaN();
                return 0;
            }
        } else {
            for (int e = 0; e < 3; ++e) out8[e] = x[e];
            out8[3] = std::sqrt(s[0] / sum[1]);
            out8[4] = sum[1] / sum[0];
        }
    }
    return 0;
}

// ---- neighbours within a radius (include/murbnbr.h; kernels: murb_kernels_nbr.h, the cut: murb_nbr.h) -----------------
// A count per point, then (lists asked for, and they fit) a second pass that fills them, in the field read-out's point buffers.
// p: the three position planes (murbnbr_at) or null (of bodies: idx lists them, or null for all n in order).  thr: a threshold
// per point.  offsets: count + 1 entries.  out_idx, out_r2: host arrays of `capacity` entries, null where not asked for; both
// null: the count pass alone.
// consume (murbsplit_of): called after every filled range [lo, hi) of the launch that starts at point `first`, with the launch's
// point capacity, while the range's entries sit in the list buffer at offsets[first + e] - offsets[first + lo] and the launch's
// bodies where stage_points left them; the lists then count as asked for and nothing of them is copied to the host.
using NbrConsume = std::function<int(unsigned long first, unsigned long lo, unsigned long hi, size_t cap)>;

// the list buffer (nbr_idx, nbr_r2) holds the `total` entries of a range: "list_entries" entries, or a single list that is longer,
// and never more than the call's `all`
int list_buffer(Shard& sh, unsigned long entries, unsigned long total, unsigned long all)
{
    size_t have = sh.nbr_list;
    const size_t want = std::max(have, (size_t)std::min<unsigned long>(std::max(entries, total), all));
    RC_TRY(grow(sh, sh.nbr_idx, have, want));
    return grow(sh, sh.nbr_r2, sh.nbr_list, want);
}

// one sweep of the neighbour kernels, counting or filling, as a span
int nbr_sweep(murbhip_ctx* c, Shard& sh, const MurbNbrArgs& na, long grid, bool fill)
{
    return timed_launch(c, sh, kProfNbr, [&] {
        if (fill)
            hipLaunchKernelGGL((murb_nbr_fill_kernel<kHermiteR, kHermiteWaves, kKnnStage>), dim3((unsigned)grid), dim3(kHermiteWaves * 64), 0,
                               sh.compute, na);
        else
            hipLaunchKernelGGL((murb_nbr_count_kernel<kHermiteR, kHermiteWaves, kKnnStage>), dim3((unsigned)grid), dim3(kHermiteWaves * 64), 0,
                               sh.compute, na);
    });
}

int nbr_run(murbhip_ctx* c, unsigned long count, const float* const* p, const int* idx, bool of_bodies, const std::vector<float>& thr,
            unsigned long* offsets, int* out_idx, float* out_r2, unsigned long capacity, const NbrConsume* consume = nullptr)
{
    PointCall pc;
    RC_TRY(field_call(c, true, count, 4, pc));
    Shard& sh = *pc.sh;
    const MurbFieldLayout& l = pc.l;
    const size_t cap = pc.cap;
    const bool lists = out_idx || out_r2 || consume;
    const unsigned long launches = murb_field_batches(l, count);
    RC_TRY(ensure_field(sh, cap, 0));
    // with lists every launch keeps its rows of prefix sums until the fill pass: launch b's rows start at b * batch * chunks
    RC_TRY(grow(sh, sh.nbr_part, sh.nbr_parts, (lists ? (launches - 1) * l.batch + cap : cap) * (size_t)l.chunks));
    {
        size_t points = sh.nbr_points;
        RC_TRY(grow(sh, sh.nbr_counts, points, cap));
        RC_TRY(grow(sh, sh.nbr_base, sh.nbr_points, cap));
    }
    std::vector<unsigned int> counts(cap), base(cap);
    const float* const planes[4] = {p ? p[0] : nullptr, p ? p[1] : nullptr, p ? p[2] : nullptr, thr.data()};   // the thresholds: a fourth plane

    // stages and packs launch `ln`; the sweeps' arguments but for the fill's own
    const auto stage = [&](const Launch& ln, MurbNbrArgs& na, long& grid) -> int {
        if (of_bodies) {   // no plane goes up with the bodies: the thresholds alone, to their plane
            std::memcpy(pc.host.data() + 3 * cap, thr.data() + ln.first, ln.bn * sizeof(float));
            HIP_TRY(hipMemcpy(sh.fld_in + 3 * cap, pc.host.data() + 3 * cap, cap * sizeof(float), hipMemcpyHostToDevice));
        }
        StagedPoints st;
        RC_TRY(stage_points(pc, ln, planes, 4, idx, of_bodies, sh.fld_in, kFieldIntPlane, st));
        MurbNbrPackArgs pa{};
        pa.in = st.in;
        pa.thr = sh.fld_in + 3 * cap;
        pa.idx = st.idx;
        pa.rec = sh.rec[c->cur];
        pa.pts = sh.fld_pts;
        pa.count = (int)ln.bn;
        pa.padded = (int)ln.padded;
        pa.in_stride = (unsigned int)cap;
        hipLaunchKernelGGL(murb_nbr_pack_kernel, dim3((unsigned)((ln.padded + 255) / 256)), dim3(256), 0, sh.compute, pa);
        const MurbFieldCut cut = murb_field_cut(l, ln.padded, pc.grid_full, true);   // a count does not depend on the cut
        na = MurbNbrArgs{};
        na.rec = sh.rec[c->cur];
        na.pts = sh.fld_pts;
        na.part = sh.nbr_part + (lists ? ln.first * (size_t)l.chunks : 0ul);   // first is a multiple of the batch
        na.group_first = 0;
        na.groups = cut.groups;
        na.chunks = cut.chunks;
        na.tiles_each = cut.tiles_each;
        na.tiles_more = cut.tiles_more;
        na.count = (int)c->in.n;
        na.stride = (unsigned int)ln.padded;   // chunks * padded <= the launch's rows
        na.soft2 = c->soft2;
        grid = cut.grid;
        return 0;
    };

    offsets[0] = 0;
    MurbNbrArgs na{};
    long grid = 0;
    for (const Launch ln : pc.launches()) {   // the count pass
        const unsigned long first = ln.first, bn = ln.bn;
        RC_TRY(stage(ln, na, grid));
        RC_TRY(nbr_sweep(c, sh, na, grid, false));
        hipLaunchKernelGGL(murb_nbr_rows_kernel, dim3((unsigned)((bn + 255) / 256)), dim3(256), 0, sh.compute, na.part, sh.nbr_counts,
                           (int)bn, na.chunks, na.stride);
        RC_TRY(hip_rc(hipGetLastError()));
        HIP_TRY(hipMemcpyAsync(counts.data(), sh.nbr_counts, bn * sizeof(unsigned int), hipMemcpyDeviceToHost, sh.compute));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        for (unsigned long e = 0; e < bn; ++e) offsets[first + e + 1] = offsets[first + e] + counts[e];
    }
    if (!lists) return 0;
    if (offsets[count] > capacity) return MURBHIP_E_INVALID;   // idx and r2 untouched: the caller sizes them from the offsets

    const unsigned long entries = murb_nbr_entries(c->nbr_list_entries);
    for (const Launch ln : pc.launches()) {   // the fill pass
        const unsigned long first = ln.first, bn = ln.bn;
        if (offsets[first + bn] == offsets[first]) continue;
        if (launches > 1) RC_TRY(stage(ln, na, grid));   // one launch: its points are still packed
        for (unsigned long lo = 0, hi; lo < bn; lo = hi) {   // ranges of the launch's points whose lists fit the buffer
            hi = murb_nbr_cut(bn, offsets + first, lo, entries);
            const unsigned long total = offsets[first + hi] - offsets[first + lo];
            if (total == 0) continue;
            RC_TRY(list_buffer(sh, entries, total, offsets[count]));
            const unsigned long g0 = lo / MURB_FIELD_GROUP, g1 = (hi + MURB_FIELD_GROUP - 1) / MURB_FIELD_GROUP;
            for (unsigned long e = g0 * MURB_FIELD_GROUP; e < g1 * MURB_FIELD_GROUP; ++e)
                base[e - g0 * MURB_FIELD_GROUP] = e >= lo && e < hi ? (unsigned int)(offsets[first + e] - offsets[first + lo]) : MURB_NBR_NO_BASE;
            HIP_TRY(hipMemcpyAsync(sh.nbr_base, base.data(), (g1 - g0) * MURB_FIELD_GROUP * sizeof(unsigned int), hipMemcpyHostToDevice, sh.compute));
            MurbNbrArgs fa = na;
            fa.base = sh.nbr_base;
            fa.out_idx = sh.nbr_idx;
            fa.out_r2 = sh.nbr_r2;
            fa.capacity = (unsigned int)sh.nbr_list;   // >= total: no place of the range lies beyond it
            fa.group_first = (int)g0;
            fa.groups = (int)(g1 - g0);   // the range's groups under the launch's cut
            RC_TRY(nbr_sweep(c, sh, fa, murb_field_grid(fa.groups, fa.chunks, pc.grid_full), true));
            HIP_TRY(hipStreamSynchronize(sh.compute));
            if (out_idx) HIP_TRY(hipMemcpy(out_idx + offsets[first + lo], sh.nbr_idx, total * sizeof(int), hipMemcpyDeviceToHost));
            if (out_r2) HIP_TRY(hipMemcpy(out_r2 + offsets[first + lo], sh.nbr_r2, total * sizeof(float), hipMemcpyDeviceToHost));
            if (consume) RC_TRY((*consume)(first, lo, hi, cap));
        }
    }
    return 0;
}

// ---- bound pairs (include/murbbind.h; kernels: murb_kernels_bind.h, the elements: murb_bind.h) ----------------------------
// One (partner, h) per point: the most bound partner, a minimum.  The field read-out's packed-point buffer; input, rows and
// results of its own.  p: the seven input planes px py pz pvx pvy pvz gm (murbbind_at; p[3..5] null: at rest, p[6] null:
// massless) or null (of bodies: idx lists them, or null for all n in order).  out_idx, out_h: host arrays, null where not asked
// for; all: the results stay on the device, bnd_idx / bnd_h [body] (murbbind_pairs; all bodies in order).
int bind_run(murbhip_ctx* c, unsigned long count, const float* const* p, const int* idx, bool of_bodies, int* out_idx, float* out_h, bool all)
{
    PointCall pc;
    RC_TRY(field_call(c, true, count, 7, pc));
    Shard& sh = *pc.sh;
    const size_t cap = pc.cap;
    RC_TRY(ensure_field(sh, cap, 0));
    {   // partners and h grow together: they share one size
        size_t h_points = sh.bnd_points;
        RC_TRY(grow(sh, sh.bnd_in, sh.bnd_ins, 8 * cap));
        RC_TRY(grow(sh, sh.bnd_part, sh.bnd_parts, cap * (size_t)pc.l.chunks));
        RC_TRY(grow(sh, sh.bnd_h, h_points, all ? std::max<size_t>(count, cap) : cap));
        RC_TRY(grow(sh, sh.bnd_idx, sh.bnd_points, all ? std::max<size_t>(count, cap) : cap));
    }
    const bool has_vel = p && p[3], has_gm = p && p[6];
    for (const Launch ln : pc.launches()) {
        StagedPoints st;
        RC_TRY(stage_points(pc, ln, p, 7, idx, of_bodies, sh.bnd_in, 7, st));
        MurbBindPackArgs pa{};
        pa.in = st.in;
        pa.idx = st.idx;
        pa.rec = sh.rec[c->cur];
        pa.vel = sh.vel;
        pa.pts = sh.fld_pts;
        pa.count = (int)ln.bn;
        pa.padded = (int)ln.padded;
        pa.in_stride = (unsigned int)cap;
        pa.has_vel = has_vel ? 1 : 0;
        pa.has_gm = has_gm ? 1 : 0;
        hipLaunchKernelGGL(murb_bind_pack_kernel, dim3((unsigned)((ln.padded + 255) / 256)), dim3(256), 0, sh.compute, pa);
        const MurbFieldCut cut = murb_field_cut(pc.l, ln.padded, pc.grid_full, true);   // a minimum does not depend on the cut
        MurbBindArgs ba{};
        ba.rec = sh.rec[c->cur];
        ba.vel = sh.vel;
        ba.pts = sh.fld_pts;
        ba.part = sh.bnd_part;
        ba.groups = cut.groups;
        ba.chunks = cut.chunks;
        ba.tiles_each = cut.tiles_each;
        ba.tiles_more = cut.tiles_more;
        ba.count = (int)c->in.n;
        ba.stride = (unsigned int)ln.padded;   // chunks * padded <= bnd_parts
        ba.soft2 = c->soft2;
        RC_TRY(timed_launch(c, sh, kProfBind, [&] {
            hipLaunchKernelGGL((murb_bind_sweep_kernel<kHermiteR, kHermiteWaves, kHermiteStage>), dim3((unsigned)cut.grid),
                               dim3(kHermiteWaves * 64), 0, sh.compute, ba);
        }));
        int* const res_idx = sh.bnd_idx + (all ? ln.first : 0ul);
        float* const res_h = sh.bnd_h + (all ? ln.first : 0ul);
        hipLaunchKernelGGL(murb_bind_rows_kernel, dim3((unsigned)((ln.bn + 255) / 256)), dim3(256), 0, sh.compute, (const uint2*)ba.part,
                           res_idx, res_h, (int)ln.bn, ba.chunks, ba.stride);
        RC_TRY(hip_rc(hipGetLastError()));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        if (out_idx) HIP_TRY(hipMemcpy(out_idx + ln.first, res_idx, ln.bn * sizeof(int), hipMemcpyDeviceToHost));
        if (out_h) HIP_TRY(hipMemcpy(out_h + ln.first, res_h, ln.bn * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
}

// The sweep over all bodies, then one thread per body: the elements of the bound pairs in dense per-body arrays, compacted
// here in index order, and the census.  pi, pj, elems: all set (capacity pairs each) or all null.
int bind_pairs(murbhip_ctx* c, int* pi, int* pj, double* elems, unsigned long capacity, unsigned long* count, double* out8)
{
    const unsigned long n = c->in.n;
    RC_TRY(bind_run(c, n, nullptr, nullptr, true, nullptr, nullptr, true));
    Shard& sh = c->shards[0];
    const size_t blocks = (n + 255) / 256;
    RC_TRY(grow(sh, sh.bnd_flag, sh.bnd_flags, (size_t)n));
    RC_TRY(grow(sh, sh.bnd_sums, sh.bnd_rows, blocks * MURB_BIND_SUMS));
    RC_TRY(grow(sh, sh.bnd_elems, sh.bnd_elem, (size_t)n * MURB_BIND_ELEMS));
    hipLaunchKernelGGL(murb_bind_pairs_kernel, dim3((unsigned)blocks), dim3(256), 0, sh.compute, (const float4*)sh.rec[c->cur],
                       (const float4*)sh.vel, (const float*)sh.mass, (const int*)sh.bnd_idx, (const float*)sh.bnd_h, sh.bnd_elems,
                       sh.bnd_flag, sh.bnd_sums, (int)n, c->soft2);
    RC_TRY(hip_rc(hipGetLastError()));
    std::vector<double> rows(blocks * MURB_BIND_SUMS), dense(n * MURB_BIND_ELEMS);
    std::vector<int> flag(n), partner(n);
    HIP_TRY(hipMemcpyAsync(rows.data(), sh.bnd_sums, rows.size() * sizeof(double), hipMemcpyDeviceToHost, sh.compute));
    HIP_TRY(hipMemcpyAsync(flag.data(), sh.bnd_flag, n * sizeof(int), hipMemcpyDeviceToHost, sh.compute));
    HIP_TRY(hipMemcpyAsync(partner.data(), sh.bnd_idx, n * sizeof(int), hipMemcpyDeviceToHost, sh.compute));
    HIP_TRY(hipMemcpyAsync(dense.data(), sh.bnd_elems, dense.size() * sizeof(double), hipMemcpyDeviceToHost, sh.compute));
    HIP_TRY(hipStreamSynchronize(sh.compute));
    double s[MURB_BIND_SUMS] = {0.0, 0.0, 0.0, 0.0};
    for (size_t b = 0; b < blocks; ++b)
        for (int e = 0; e < MURB_BIND_SUMS; ++e) s[e] += rows[b * MURB_BIND_SUMS + e];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double hard_i = nan, hard_j = nan, hard_e = nan, least_a = nan;
    unsigned long pairs = 0;
    for (unsigned long i = 0; i < n; ++i) {
        if (!flag[i]) continue;
        const double* const e = dense.data() + i * MURB_BIND_ELEMS;
        if (pairs == 0 || e[4] < hard_e) { hard_i = (double)i; hard_j = (double)partner[i]; hard_e = e[4]; }   // the lowest i among equals
        if (pairs == 0 || e[0] < least_a) least_a = e[0];
        ++pairs;
    }
    *count = pairs;
    out8[0] = s[0]; out8[1] = s[1]; out8[2] = hard_i; out8[3] = hard_j; out8[4] = hard_e; out8[5] = least_a; out8[6] = s[2]; out8[7] = s[3];
    if (!pi) return 0;
    if (capacity < pairs) return MURBHIP_E_INVALID;
    unsigned long at = 0;
    for (unsigned long i = 0; i < n; ++i) {
        if (!flag[i]) continue;
        pi[at] = (int)i;
        pj[at] = partner[i];
        std::memcpy(elems + at * MURB_BIND_ELEMS, dense.data() + i * MURB_BIND_ELEMS, MURB_BIND_ELEMS * sizeof(double));
        ++at;
    }
    return 0;
}

// ---- potential read-out and bound members (include/murbbound.h; kernels: murb_kernels_pot.h, the arithmetic: murb_bound.h) ----
// The masked copy of the records from the mask on the device (pot_member): the sweep's j side under a mask.
int pot_mask(murbhip_ctx* c, Shard& sh)
{
    const MurbFieldLayout l = murb_field_layout(c->in.n, c->field_chunks, c->field_batch);
    const size_t records = (size_t)l.tiles * MURB_TILE_F4;   // the tiles that hold real bodies: all the sweep reads
    RC_TRY(grow(sh, sh.pot_rec, sh.pot_recs, records));
    hipLaunchKernelGGL(murb_pot_mask_kernel, dim3((unsigned)((records + 255) / 256)), dim3(256), 0, sh.compute,
                       (const float4*)sh.rec[c->cur], (const unsigned char*)sh.pot_member, sh.pot_rec, (int)c->in.n, (unsigned int)records);
    return hip_rc(hipGetLastError());
}

int pot_upload_mask(murbhip_ctx* c, Shard& sh, const unsigned char* member)
{
    RC_TRY(grow(sh, sh.pot_member, sh.pot_members, (size_t)c->in.n));
    HIP_TRY(hipMemcpy(sh.pot_member, member, c->in.n, hipMemcpyHostToDevice));
    return 0;
}

// One potential per point, a sum, in the field read-out's packed-point buffer; input, rows and results of its own.  The caller
// has prepared the stream.  p: the three position planes (murbpot_at) or null (of bodies: idx lists them, or null for all n in
// order).  masked: the j side is the masked copy (pot_mask has run on the compute stream).  out: a host array, or null; all: the
// results stay on the device, pot_phi[body] (murbbound_members; all bodies in order).
int pot_run(murbhip_ctx* c, unsigned long count, const float* const* p, const int* idx, bool of_bodies, bool masked, float* out, bool all)
{
    PointCall pc;
    RC_TRY(field_call(c, false, count, 3, pc));
    Shard& sh = *pc.sh;
    const size_t cap = pc.cap;
    RC_TRY(ensure_field(sh, cap, 0));
    RC_TRY(grow(sh, sh.pot_in, sh.pot_ins, 4 * cap));
    RC_TRY(grow(sh, sh.pot_part, sh.pot_parts, cap * (size_t)pc.l.chunks));
    RC_TRY(grow(sh, sh.pot_phi, sh.pot_phis, all ? std::max<size_t>(count, cap) : cap));
    for (const Launch ln : pc.launches()) {
        StagedPoints st;
        RC_TRY(stage_points(pc, ln, p, 3, idx, of_bodies, sh.pot_in, 3, st));
        RC_TRY(pack_points(c, sh, st, sh.fld_pts, ln.bn, ln.padded, cap, false));
        const MurbFieldCut cut = murb_field_cut(pc.l, ln.padded, pc.grid_full, false);   // a sum depends on the cut
        MurbPotArgs ta{};
        ta.rec = masked ? sh.pot_rec : sh.rec[c->cur];
        ta.pts = sh.fld_pts;
        ta.part = sh.pot_part;
        ta.groups = cut.groups;
        ta.chunks = cut.chunks;
        ta.tiles = pc.l.tiles;
        ta.stride = (unsigned int)ln.padded;   // chunks * padded <= pot_parts
        ta.soft2 = c->soft2;
        RC_TRY(timed_launch(c, sh, kProfPot, [&] {
            hipLaunchKernelGGL((murb_pot_sweep_kernel<kHermiteR, kHermiteWaves, kKnnStage>), dim3((unsigned)cut.grid), dim3(kHermiteWaves * 64),
                               0, sh.compute, ta);
        }));
        float* const res = sh.pot_phi + (all ? ln.first : 0ul);
        hipLaunchKernelGGL(murb_pot_rows_kernel, dim3((unsigned)((ln.bn + 255) / 256)), dim3(256), 0, sh.compute, (const float*)ta.part, res,
                           (int)ln.bn, ta.chunks, ta.stride);
        RC_TRY(hip_rc(hipGetLastError()));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        if (out) HIP_TRY(hipMemcpy(out + ln.first, res, ln.bn * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
}

// murbpot_of / murbpot_at once their arguments are checked
int pot_call(murbhip_ctx* c, unsigned long count, const float* const* p, const int* idx, bool of_bodies, const unsigned char* member,
             float* phi)
{
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    if (member) {
        RC_TRY(pot_upload_mask(c, sh, member));
        RC_TRY(pot_mask(c, sh));
    }
    return pot_run(c, count, p, idx, of_bodies, member != nullptr, phi, false);
}

// The rounds of include/murbbound.h, 2.  Every round sweeps all bodies against the masked records, so the evaluation of the
// round that converges is the final pass.
int bound_members(murbhip_ctx* c, const unsigned char* start, const double* frame_v, int max_iter, unsigned char* member, double* e,
                  double* out16)
{
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    const unsigned long n = c->in.n;
    const size_t blocks = (n + 255) / 256;
    RC_TRY(grow(sh, sh.pot_e, sh.pot_es, (size_t)n));
    RC_TRY(grow(sh, sh.pot_rows, sh.pot_row, blocks * (MURB_BOUND_SUMS + 1)));
    {
        std::vector<unsigned char> s0(n, 1);   // 0 / 1: the bytes go back to the caller as they are
        for (unsigned long i = 0; start && i < n; ++i) s0[i] = start[i] ? 1 : 0;
        RC_TRY(pot_upload_mask(c, sh, s0.data()));
    }
    double* const sums_dev = sh.pot_rows;
    double* const removed_dev = sh.pot_rows + blocks * MURB_BOUND_SUMS;
    std::vector<double> rows(blocks * (MURB_BOUND_SUMS + 1));
    double s[MURB_BOUND_SUMS + 1], V[3] = {0.0, 0.0, 0.0};
    // the sums of the set on the device (with_energy: K, m phi and the bodies with e >= 0 too), the block rows added in index
    // order; the rows of the energy kernel before it come along in the same copy
    const auto sums = [&](bool with_energy, bool with_removed) -> int {
        hipLaunchKernelGGL(murb_bound_sums_kernel, dim3((unsigned)blocks), dim3(256), 0, sh.compute, (const float4*)sh.rec[c->cur],
                           (const float4*)sh.vel, (const float*)sh.mass, (const unsigned char*)sh.pot_member, (const float*)sh.pot_phi,
                           (const double*)sh.pot_e, sums_dev, (int)n, with_energy ? 1 : 0, V[0], V[1], V[2]);
        RC_TRY(hip_rc(hipGetLastError()));
        const size_t take = blocks * (MURB_BOUND_SUMS + (with_removed ? 1 : 0));
        HIP_TRY(hipMemcpyAsync(rows.data(), sh.pot_rows, take * sizeof(double), hipMemcpyDeviceToHost, sh.compute));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        for (int k = 0; k <= MURB_BOUND_SUMS; ++k) s[k] = 0.0;
        for (size_t b = 0; b < blocks; ++b)
            for (int k = 0; k < MURB_BOUND_SUMS; ++k) s[k] += rows[b * MURB_BOUND_SUMS + k];
        for (size_t b = 0; with_removed && b < blocks; ++b) s[MURB_BOUND_SUMS] += rows[blocks * MURB_BOUND_SUMS + b];
        return 0;
    };
    const auto frame = [&]() {
        if (frame_v) { V[0] = frame_v[0]; V[1] = frame_v[1]; V[2] = frame_v[2]; }
        else murb_bound_frame(s[1], s + 2, V);
    };
    const auto evaluate = [&](bool update) -> int {
        RC_TRY(pot_mask(c, sh));
        RC_TRY(pot_run(c, n, nullptr, nullptr, true, true, nullptr, true));
        hipLaunchKernelGGL(murb_bound_energy_kernel, dim3((unsigned)blocks), dim3(256), 0, sh.compute, (const float4*)sh.vel,
                           (const float*)sh.pot_phi, sh.pot_member, sh.pot_e, removed_dev, (int)n, update ? 1 : 0, V[0], V[1], V[2]);
        return hip_rc(hipGetLastError());
    };
    RC_TRY(sums(false, false));
    const double members_start = s[0];
    frame();
    int rounds = 0;
    bool converged = false;
    while (rounds < max_iter && !converged) {
        RC_TRY(evaluate(true));
        ++rounds;
        RC_TRY(sums(false, true));   // of S_{t+1}
        converged = s[MURB_BOUND_SUMS] == 0.0;
        if (!converged) frame();     // the same set has the same frame: nothing to redo
    }
    if (!converged) RC_TRY(evaluate(false));   // the final pass against S_{max_iter} and its V
    RC_TRY(sums(true, false));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const bool empty = s[0] == 0.0;
    const double K = s[8], W = -0.5 * s[9];
    out16[0] = s[0];
    out16[1] = s[1];
    out16[2] = (double)rounds;
    out16[3] = converged ? 1.0 : 0.0;
    for (int k = 0; k < 3; ++k) out16[4 + k] = empty ? nan : V[k];
    for (int k = 0; k < 3; ++k) out16[7 + k] = s[5 + k] / s[1];   // 0 / 0: NaN
    out16[10] = K;
    out16[11] = W;
    out16[12] = K / std::fabs(W);
    out16[13] = members_start - s[0];
    out16[14] = s[10];
    out16[15] = 0.0;
    if (member) HIP_TRY(hipMemcpy(member, sh.pot_member, n, hipMemcpyDeviceToHost));
    if (e) HIP_TRY(hipMemcpy(e, sh.pot_e, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// ---- nearest body of another label and the spanning tree (include/murbmst.h; kernels: murb_kernels_mst.h, the rounds: murb_mst.h)
// The labels to the device and the labelled copy of the records from them: the sweep's j side.
int foreign_labels(murbhip_ctx* c, Shard& sh, const int* label)
{
    const MurbFieldLayout l = murb_field_layout(c->in.n, c->field_chunks, c->field_batch);
    const size_t records = (size_t)l.tiles * MURB_TILE_F4;   // the tiles that hold real bodies: all the sweep reads
    RC_TRY(grow(sh, sh.mst_label, sh.mst_labels, (size_t)c->in.n));
    RC_TRY(grow(sh, sh.mst_rec, sh.mst_recs, records));
    HIP_TRY(hipMemcpy(sh.mst_label, label, c->in.n * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(murb_mst_label_kernel, dim3((unsigned)((records + 255) / 256)), dim3(256), 0, sh.compute,
                       (const float4*)sh.rec[c->cur], (const int*)sh.mst_label, sh.mst_rec, (int)c->in.n, (unsigned int)records);
    return hip_rc(hipGetLastError());
}

// One (partner, r2) per point: the nearest body of another label, a minimum.  The field read-out's packed-point buffer; bodies,
// rows and results of its own.  The caller has prepared the stream, and foreign_labels has run on it.  The points are listed
// bodies (idx, or null for all n in order).
int foreign_run(murbhip_ctx* c, unsigned long count, const int* idx, int* out_idx, float* out_r2)
{
    PointCall pc;
    RC_TRY(field_call(c, false, count, 0, pc));
    Shard& sh = *pc.sh;
    const size_t cap = pc.cap;
    RC_TRY(ensure_field(sh, cap, 0));
    {   // partners and r2 grow together: they share one size
        size_t r2_points = sh.mst_points;
        RC_TRY(grow(sh, sh.mst_in, sh.mst_ins, cap));
        RC_TRY(grow(sh, sh.mst_part, sh.mst_parts, cap * (size_t)pc.l.chunks));
        RC_TRY(grow(sh, sh.mst_r2, r2_points, cap));
        RC_TRY(grow(sh, sh.mst_idx, sh.mst_points, cap));
    }
    for (const Launch ln : pc.launches()) {
        StagedPoints st;   // mst_in is the one plane, of ints
        RC_TRY(stage_points(pc, ln, nullptr, 0, idx, true, (float*)sh.mst_in, 0, st));
        hipLaunchKernelGGL(murb_foreign_pack_kernel, dim3((unsigned)((ln.padded + 255) / 256)), dim3(256), 0, sh.compute,
                           (const float4*)sh.rec[c->cur], (const int*)sh.mst_label, st.idx, sh.fld_pts, (int)ln.bn, (int)ln.padded);
        const MurbFieldCut cut = murb_field_cut(pc.l, ln.padded, pc.grid_full, true);   // a minimum does not depend on the cut
        MurbForeignArgs fa{};
        fa.rec = sh.mst_rec;
        fa.pts = sh.fld_pts;
        fa.part = sh.mst_part;
        fa.groups = cut.groups;
        fa.chunks = cut.chunks;
        fa.tiles_each = cut.tiles_each;
        fa.tiles_more = cut.tiles_more;
        fa.stride = (unsigned int)ln.padded;   // chunks * padded <= mst_parts
        fa.soft2 = c->soft2;
        RC_TRY(timed_launch(c, sh, kProfMst, [&] {
            hipLaunchKernelGGL((murb_foreign_sweep_kernel<kHermiteR, kHermiteWaves, kKnnStage>), dim3((unsigned)cut.grid),
                               dim3(kHermiteWaves * 64), 0, sh.compute, fa);
        }));
        hipLaunchKernelGGL(murb_foreign_rows_kernel, dim3((unsigned)((ln.bn + 255) / 256)), dim3(256), 0, sh.compute, (const uint2*)fa.part,
                           (const float4*)sh.fld_pts, sh.mst_idx, sh.mst_r2, (int)ln.bn, fa.chunks, fa.stride);
        RC_TRY(hip_rc(hipGetLastError()));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        if (out_idx) HIP_TRY(hipMemcpy(out_idx + ln.first, sh.mst_idx, ln.bn * sizeof(int), hipMemcpyDeviceToHost));
        if (out_r2) HIP_TRY(hipMemcpy(out_r2 + ln.first, sh.mst_r2, ln.bn * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
}

// murbforeign_of once its arguments are checked
int foreign_call(murbhip_ctx* c, unsigned long count, const int* bodies, const int* label, int* partner, float* r2)
{
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    RC_TRY(foreign_labels(c, sh, label));
    return foreign_run(c, count, bodies, partner, r2);
}

// The rounds of include/murbmst.h.  The points of every round are the members alone.
int mst_call(murbhip_ctx* c, const unsigned char* member, unsigned long capacity, int* ei, int* ej, float* er2, double* elen, int* label,
             double* out8)
{
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    const unsigned long n = c->in.n;
    std::vector<int> lab(n), members;
    for (unsigned long i = 0; i < n; ++i) {
        lab[i] = !member || member[i] ? (int)i : -1;
        if (lab[i] >= 0) members.push_back((int)i);
    }
    const unsigned long m = members.size();
    std::vector<int> got_idx(m), partner(n, -1);
    std::vector<float> got_r2(m), r2(n, std::numeric_limits<float>::infinity());
    std::vector<MurbMstEdge> tree, chosen;
    int rounds = 0;
    // a round that adds no edge ends the rounds and is not counted; with one component left there is nothing to sweep for
    for (bool more = m > 1; more;) {
        if (rounds == MURB_MST_ROUNDS_MAX) return MURBHIP_E_STATE;   // never reached: every round at least halves the components
        RC_TRY(foreign_labels(c, sh, lab.data()));
        RC_TRY(foreign_run(c, m, members.data(), got_idx.data(), got_r2.data()));
        for (unsigned long k = 0; k < m; ++k) {
            partner[members[k]] = got_idx[k];
            r2[members[k]] = got_r2[k];
        }
        if (!murb_mst_round(n, lab.data(), partner.data(), r2.data(), chosen)) return MURBHIP_E_STATE;   // the sweep's rule rules it out
        rounds += chosen.empty() ? 0 : 1;
        tree.insert(tree.end(), chosen.begin(), chosen.end());
        more = !chosen.empty() && tree.size() + 1 < m;
    }
    std::sort(tree.begin(), tree.end(), murb_mst_before);
    unsigned long components = 0;
    for (unsigned long k = 0; k < m; ++k) components += lab[members[k]] == members[k];
    // the lengths from the device's fp32 coordinates
    std::vector<double> len(tree.size());
    if (!tree.empty()) {
        const MurbFieldLayout l = murb_field_layout(n, c->field_chunks, c->field_batch);
        std::vector<float4> rec((size_t)l.tiles * MURB_TILE_F4);
        HIP_TRY(hipMemcpy(rec.data(), sh.rec[c->cur], rec.size() * sizeof(float4), hipMemcpyDeviceToHost));
        const auto q = [&](int s, float (&out)[3]) {
            const float* const f = (const float*)(rec.data() + murb_rec_a((unsigned long)(s >> 1))) + (s & 1);
            out[0] = f[0]; out[1] = f[2]; out[2] = f[4 * MURB_TILE_PAIRS];
        };
        for (size_t e = 0; e < tree.size(); ++e) {
            float a[3], b[3];
            q(tree[e].i, a);
            q(tree[e].j, b);
            len[e] = murb_mst_length(a[0], a[1], a[2], b[0], b[1], b[2]);
        }
    }
    double total = 0.0, longest = 0.0;
    for (const double v : len) {
        total += v;
        longest = std::max(longest, v);
    }
    out8[0] = (double)m;
    out8[1] = (double)tree.size();
    out8[2] = (double)components;
    out8[3] = (double)rounds;
    out8[4] = total;
    out8[5] = tree.empty() ? std::numeric_limits<double>::quiet_NaN() : total / (double)tree.size();
    out8[6] = longest;
    out8[7] = 0.0;
    if (label) std::memcpy(label, lab.data(), n * sizeof(int));
    if (!ei && !ej && !er2 && !elen) return 0;
    if (capacity < tree.size()) return MURBHIP_E_INVALID;   // the edge arrays untouched: the caller sizes them from out8[1]
    for (size_t e = 0; e < tree.size(); ++e) {
        if (ei) ei[e] = tree[e].i;
        if (ej) ej[e] = tree[e].j;
        if (er2) er2[e] = tree[e].r2;
        if (elen) elen[e] = len[e];
    }
    return 0;
}

// ---- pair separations (include/murbsep.h; kernels: murb_kernels_sep.h, the bins and the launch cut: murb_sep.h) ---------------
// murbsep_of / murbsep_at once their arguments are checked.  A sum per point and, with bins, a histogram, in the field read-out's
// packed-point buffer; the launches are cut by murb_sep_cut, so that no 32-bit counter of a workgroup can wrap.  p: the three
// position planes (murbsep_at) or null (of bodies: idx lists them, or null for all n in order).  bins == 0: the sum-only sweep.
int sep_call(murbhip_ctx* c, unsigned long count, const float* const* p, const int* idx, bool of_bodies, const unsigned char* member,
             double* sum, int lo_exp, int sub, int bins, unsigned long long* hist, unsigned long long* out4)
{
    const unsigned long n = c->in.n;
    const MurbFieldLayout l = field_layout(c);
    const long grid_full = sweep_grid(c);
    PointCall pc;
    RC_TRY(point_call(c, true, l, murb_sep_cut(l, grid_full), count, of_bodies ? 0 : 3, pc));
    if (pc.batch == 0) return MURBHIP_E_INVALID;   // one group of points against the longest chunk would pass 2^32 pairs
    Shard& sh = *pc.sh;
    const size_t cap = pc.cap;
    const int width = bins > 0 ? MURB_SEP_TABLE : 0;   // the table's slots: below | the bins | above, the rest above too
    const size_t pairs = (size_t)l.tiles * MURB_TILE_PAIRS, records = (size_t)l.tiles * MURB_TILE_F4;
    RC_TRY(ensure_field(sh, cap, 0));
    RC_TRY(grow(sh, sh.sep_in, sh.sep_ins, 4 * cap));
    RC_TRY(grow(sh, sh.sep_rec, sh.sep_recs, records));
    RC_TRY(grow(sh, sh.sep_part, sh.sep_parts, cap * (size_t)l.chunks));
    RC_TRY(grow(sh, sh.sep_sum, sh.sep_sums, cap));
    if (width) {
        RC_TRY(grow(sh, sh.sep_rows, sh.sep_row, (size_t)grid_full * MURB_SEP_TABLE));
        RC_TRY(grow(sh, sh.sep_total, sh.sep_totals, (size_t)MURB_SEP_TABLE));
        HIP_TRY(hipMemsetAsync(sh.sep_total, 0, (size_t)width * sizeof(unsigned long long), sh.compute));
    }
    unsigned long in_set = n;   // |S|
    if (member) {
        RC_TRY(grow(sh, sh.sep_member, sh.sep_members, (size_t)n));
        HIP_TRY(hipMemcpy(sh.sep_member, member, n, hipMemcpyHostToDevice));
        in_set = 0;
        for (unsigned long i = 0; i < n; ++i) in_set += member[i] != 0;
    }
    hipLaunchKernelGGL(murb_sep_mask_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, sh.compute, (const float4*)sh.rec[c->cur],
                       member ? (const unsigned char*)sh.sep_member : nullptr, sh.sep_rec, (int)n, (unsigned int)pairs);
    RC_TRY(hip_rc(hipGetLastError()));
    unsigned long long not_counted = 0;   // entries the slots outside S and the filler points left in the table's last slot
    for (const Launch ln : pc.launches()) {
        StagedPoints st;
        RC_TRY(stage_points(pc, ln, p, 3, idx, of_bodies, sh.sep_in, 3, st));
        RC_TRY(pack_points(c, sh, st, sh.fld_pts, ln.bn, ln.padded, cap, false));
        const MurbFieldCut cut = murb_field_cut(l, ln.padded, grid_full, false);   // a sum depends on the cut; grid * width <= sep_row
        MurbSepArgs ta{};
        ta.rec = sh.sep_rec;
        ta.pts = sh.fld_pts;
        ta.part = sh.sep_part;
        ta.rows = sh.sep_rows;
        ta.groups = cut.groups;
        ta.chunks = cut.chunks;
        ta.tiles = l.tiles;
        ta.count = (int)ln.bn;
        ta.stride = (unsigned int)ln.padded;   // chunks * padded <= sep_parts
        ta.sh = murb_sep_shift(sub);
        ta.minus4 = -4 * (murb_sep_base(lo_exp, sub) - 1);
        RC_TRY(timed_launch(c, sh, kProfSep, [&] {
            if (width)
                hipLaunchKernelGGL((murb_sep_sweep_kernel<kHermiteR, kHermiteWaves, kKnnStage, true>), dim3((unsigned)cut.grid),
                                   dim3(kHermiteWaves * 64), 0, sh.compute, ta);
            else
                hipLaunchKernelGGL((murb_sep_sweep_kernel<kHermiteR, kHermiteWaves, kKnnStage, false>), dim3((unsigned)cut.grid),
                                   dim3(kHermiteWaves * 64), 0, sh.compute, ta);
        }));
        const unsigned long threads = std::max<unsigned long>(ln.bn, (unsigned long)width);
        hipLaunchKernelGGL(murb_sep_rows_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, sh.compute, (const float*)ta.part,
                           sh.sep_sum, (int)ln.bn, ta.chunks, ta.stride, (const unsigned int*)sh.sep_rows, sh.sep_total, width, (int)cut.grid);
        RC_TRY(hip_rc(hipGetLastError()));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        if (sum) HIP_TRY(hipMemcpy(sum + ln.first, sh.sep_sum, ln.bn * sizeof(double), hipMemcpyDeviceToHost));
        not_counted += (unsigned long long)ln.padded * ((unsigned long long)l.tiles * MURB_TILE_BODIES) - (unsigned long long)ln.bn * in_set;
    }
    if (!width) return 0;
    std::vector<unsigned long long> total((size_t)width);
    HIP_TRY(hipMemcpy(total.data(), sh.sep_total, (size_t)width * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long own = 0;   // listed bodies that are in S: each met itself at d2 == +0, below the lowest edge
    if (of_bodies)
        for (unsigned long i = 0; i < count; ++i) own += !member || member[idx ? idx[i] : (long)i] != 0;
    for (int k = 0; k < bins; ++k) hist[k] = total[(size_t)k + 1];
    out4[0] = (unsigned long long)count * in_set - own;
    out4[1] = total[0] - own;
    unsigned long long above = 0;
    for (size_t k = (size_t)bins + 1; k < total.size(); ++k) above += total[k];
    out4[2] = above - not_counted;
    out4[3] = 0;
    return 0;
}

// the checks murbsep_of and murbsep_at share: what is asked for, the histogram's parameters and where it goes
inline bool sep_request_valid(const double* sum, int lo_exp, int sub, int bins, const unsigned long long* hist, const unsigned long long* out4)
{
    if (bins == 0) return sum != nullptr;
    return hist && out4 && murb_sep_params_valid(lo_exp, sub, bins);
}

// ---- the field of listed bodies (include/murblist.h; kernels: murb_kernels_list.h, the checks: murb_list.h) ------------------
constexpr int kListWaves = 4;   // one wave per point

// The gather copy of the bodies, rewritten per call: read-outs are synchronous and the copy is 32 B x n.
int list_pack(murbhip_ctx* c, Shard& sh)
{
    const size_t n = c->in.n;
    RC_TRY(grow(sh, sh.lst_src, sh.lst_srcs, 2 * n));
    MurbListPackArgs pa{};
    pa.rec = sh.rec[c->cur];
    pa.vel = sh.vel;
    pa.src = sh.lst_src;
    pa.count = (int)n;
    hipLaunchKernelGGL(murb_list_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sh.compute, pa);
    return hip_rc(hipGetLastError());
}

// One range of `npts` points, packed at pts, whose entries sit in the list buffer (nbr_idx): range holds the points' list starts,
// then their lengths.  Synchronous: on return the list buffer, lst_range and fld_out are free again.  out: the caller's planes,
// null where not asked for; the range's first point is point `at` of the call.
int list_sweep(murbhip_ctx* c, Shard& sh, const float4* pts, unsigned long npts, const std::vector<unsigned int>& range, float* const (&out)[7],
               unsigned long at, std::vector<float>& host)
{
    RC_TRY(grow(sh, sh.lst_range, sh.lst_ranges, 2 * npts));
    HIP_TRY(hipMemcpy(sh.lst_range, range.data(), 2 * npts * sizeof(unsigned int), hipMemcpyHostToDevice));
    MurbListArgs la{};
    la.src = sh.lst_src;
    la.pts = pts;
    la.begin = sh.lst_range;
    la.len = sh.lst_range + npts;
    la.idx = sh.nbr_idx;
    la.out = sh.fld_out;   // 7 * npts <= 7 * fld_points
    la.count = (int)npts;
    la.out_stride = (unsigned int)npts;
    la.soft2 = c->soft2;
    RC_TRY(timed_launch(c, sh, kProfList, [&] {
        hipLaunchKernelGGL((murb_list_sweep_kernel<kListWaves>), dim3((unsigned)((npts + kListWaves - 1) / kListWaves)), dim3(kListWaves * 64), 0,
                           sh.compute, la);
    }));
    HIP_TRY(hipStreamSynchronize(sh.compute));
    host.resize(7 * npts);
    HIP_TRY(hipMemcpy(host.data(), sh.fld_out, 7 * npts * sizeof(float), hipMemcpyDeviceToHost));
    for (int k = 0; k < 7; ++k)
        if (out[k]) std::memcpy(out[k] + at, host.data() + k * npts, npts * sizeof(float));
    return 0;
}

// the starts and lengths of the lists of points [lo, hi) of a CSR pair, relative to the range's first entry
void list_range(const unsigned long* offsets, unsigned long lo, unsigned long hi, std::vector<unsigned int>& range)
{
    const unsigned long npts = hi - lo;
    range.resize(2 * npts);
    for (unsigned long e = 0; e < npts; ++e) {
        range[e] = (unsigned int)(offsets[lo + e] - offsets[lo]);
        range[npts + e] = (unsigned int)(offsets[lo + e + 1] - offsets[lo + e]);
    }
}

// What murblist_of and murblist_at share once their arguments are checked.  The launches and the packed points are the field
// read-out's; inside a launch the points are cut into ranges whose entries fit the list buffer (murb_nbr_cut under
// "list_entries"), staged there and swept.  p: the six input planes (murblist_at; p[3..5] null: at rest) or null (murblist_of: idx
// are the bodies, or null for all n in order).
int list_run(murbhip_ctx* c, unsigned long count, const float* const* p, const int* idx, bool of_bodies, const unsigned long* offsets,
             const int* entries_in, float* const (&out)[7])
{
    PointCall pc;
    RC_TRY(field_call(c, true, count, 6, pc));
    Shard& sh = *pc.sh;
    const size_t cap = pc.cap;
    RC_TRY(ensure_field(sh, cap, 0));
    RC_TRY(list_pack(c, sh));
    const unsigned long entries = murb_nbr_entries(c->nbr_list_entries);
    const bool has_vel = p && p[3];
    std::vector<float> results;
    std::vector<unsigned int> range;
    for (const Launch ln : pc.launches()) {
        const unsigned long first = ln.first, bn = ln.bn;
        if (offsets[first + bn] == offsets[first]) {   // empty lists alone: +0 seven times
            for (int k = 0; k < 7; ++k)
                if (out[k]) std::fill(out[k] + first, out[k] + first + bn, 0.f);
            continue;
        }
        StagedPoints st;
        RC_TRY(stage_points(pc, ln, p, has_vel ? 6 : 3, idx, of_bodies, sh.fld_in, kFieldIntPlane, st));
        RC_TRY(pack_points(c, sh, st, sh.fld_pts, bn, bn, cap, has_vel));   // a wave takes one point: no group to fill up
        for (unsigned long lo = 0, hi; lo < bn; lo = hi) {
            hi = murb_nbr_cut(bn, offsets + first, lo, entries);
            const unsigned long total = offsets[first + hi] - offsets[first + lo];
            if (total == 0) {
                for (int k = 0; k < 7; ++k)
                    if (out[k]) std::fill(out[k] + first + lo, out[k] + first + hi, 0.f);
                continue;
            }
            RC_TRY(list_buffer(sh, entries, total, offsets[count]));
            HIP_TRY(hipMemcpy(sh.nbr_idx, entries_in + offsets[first + lo], total * sizeof(int), hipMemcpyHostToDevice));
            list_range(offsets + first, lo, hi, range);
            RC_TRY(list_sweep(c, sh, sh.fld_pts + 2 * lo, hi - lo, range, out, first + lo, results));
        }
    }
    return 0;
}

// ---- the Ahmad-Cohen neighbour scheme (include/murbac.h; kernels: murb_kernels_ac.h, the polynomial: murb_ac.h) ---------------
// Hermite steps on the compute stream whose full sweep happens on every n_irr-th step only.  Lists, split forces and every
// buffer a step writes are the scheme's own (Shard::ac_*); of the Hermite integrator it uses the predicted records, the partial
// rows and the remembered (a0, j0).  The rebuild is the neighbour read-out's kernels (pack, count, rows, fill) as they are, over
// all bodies in ONE launch each and pointed at the records it is given; its one host round trip reads the counts.
inline int ac_requirements(const murbhip_ctx* c)
{
    const bool ok = c->uploaded && c->integrator == 2 && c->in.world == 1 && c->shards.size() == 1 && !c->force_exchange && !c->blk_open &&
                    !c->lf_half && !c->tracers && !c->nearest && !c->contact && !c->potential;
    return ok ? 0 : MURBHIP_E_STATE;
}

// the buffers whose size the body count fixes; the caller has waited for enqueued work
int ac_ensure(murbhip_ctx* c, Shard& sh)
{
    const size_t n = c->in.n, padded = murb_field_padded(n);
    RC_TRY(grow(sh, sh.ac_src, sh.ac_srcs, 2 * n));
    RC_TRY(grow(sh, sh.ac_in, sh.ac_ins, 2 * n));
    RC_TRY(grow(sh, sh.ac_pts, sh.ac_ptss, 2 * padded));
    RC_TRY(grow(sh, sh.ac_out, sh.ac_outs, 14 * n));
    RC_TRY(grow(sh, sh.ac_force, sh.ac_forces, 18 * n));
    for (int b = 0; b < 2; ++b) {
        size_t have = sh.ac_points[b];
        RC_TRY(grow(sh, sh.ac_begin[b], have, padded));
        RC_TRY(grow(sh, sh.ac_len[b], sh.ac_points[b], padded));
    }
    return 0;
}

// the gather copy of the state (rec, vel)
int ac_pack(murbhip_ctx* c, Shard& sh, const float4* rec, const float4* vel)
{
    MurbListPackArgs pa{};
    pa.rec = rec;
    pa.vel = vel;
    pa.src = sh.ac_src;
    pa.count = (int)c->in.n;
    hipLaunchKernelGGL(murb_list_pack_kernel, dim3((unsigned)((c->in.n + 255) / 256)), dim3(256), 0, sh.compute, pa);
    return hip_rc(hipGetLastError());
}

// every body's list field over the lists of buffer `buf`, at its own gather records; asynchronous
int ac_sweep(murbhip_ctx* c, Shard& sh, int buf, float* out)
{
    MurbAcSweepArgs a{};
    a.src = sh.ac_src;
    a.begin = sh.ac_begin[buf];
    a.len = sh.ac_len[buf];
    a.idx = sh.ac_idx[buf];
    a.out = out;
    a.count = (int)c->in.n;
    a.out_stride = (unsigned int)c->in.n;
    a.soft2 = c->soft2;
    return timed_launch(c, sh, kProfList, [&] {   // a list span
        hipLaunchKernelGGL((murb_ac_sweep_kernel<kListWaves>), dim3((unsigned)((c->in.n + kListWaves - 1) / kListWaves)), dim3(kListWaves * 64), 0,
                           sh.compute, a);
    });
}

// The lists of all bodies at the positions `rec`, into list buffer `buf`: begin, length and entries on the device, the offsets
// and their statistics on the host.  Waits for the stream once, after the count pass.
int ac_rebuild(murbhip_ctx* c, Shard& sh, const float4* rec, int buf)
{
    const size_t n = c->in.n, padded = murb_field_padded(n);
    const MurbFieldCut cut = murb_field_cut(murb_field_layout(n, c->field_chunks, 0), padded, sweep_grid(c), true);   // a list does not depend on the cut
    MurbNbrPackArgs pa{};
    pa.thr = sh.ac_in;
    pa.idx = (const int*)(sh.ac_in + n);
    pa.rec = rec;
    pa.pts = sh.ac_pts;
    pa.count = (int)n;
    pa.padded = (int)padded;
    pa.in_stride = (unsigned int)n;
    MurbNbrArgs na{};
    na.rec = rec;
    na.pts = sh.ac_pts;
    na.groups = cut.groups;
    na.chunks = cut.chunks;
    na.tiles_each = cut.tiles_each;
    na.tiles_more = cut.tiles_more;
    na.count = (int)n;
    na.stride = (unsigned int)padded;
    na.soft2 = c->soft2;
    if ((size_t)na.chunks * padded > sh.ac_parts) {   // "field_chunks" grew: the last rebuild's fill may still read the rows
        HIP_TRY(hipStreamSynchronize(sh.compute));
        RC_TRY(grow(sh, sh.ac_part, sh.ac_parts, (size_t)na.chunks * padded));
    }
    na.part = sh.ac_part;
    hipLaunchKernelGGL(murb_nbr_pack_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, sh.compute, pa);
    RC_TRY(hip_rc(hipGetLastError()));
    RC_TRY(nbr_sweep(c, sh, na, cut.grid, false));
    hipLaunchKernelGGL(murb_nbr_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sh.compute, na.part, sh.ac_len[buf], (int)n,
                       na.chunks, na.stride);
    RC_TRY(hip_rc(hipGetLastError()));
    std::vector<unsigned int> counts(n), base(padded, MURB_NBR_NO_BASE);
    HIP_TRY(hipMemcpyAsync(counts.data(), sh.ac_len[buf], n * sizeof(unsigned int), hipMemcpyDeviceToHost, sh.compute));
    HIP_TRY(hipStreamSynchronize(sh.compute));   // the one host round trip of a regular step; nothing is in flight behind it
    std::vector<unsigned long> offsets(n + 1, 0ul);
    unsigned long longest = 0, empty = 0;
    for (size_t i = 0; i < n; ++i) {
        offsets[i + 1] = offsets[i] + counts[i];
        longest = std::max<unsigned long>(longest, counts[i]);
        empty += counts[i] == 0u;
    }
    const unsigned long total = offsets[n];
    if (total > 0x7ffffffful) return MURBHIP_E_INVALID;   // the sweeps' places are 32-bit
    for (size_t i = 0; i < n; ++i) base[i] = (unsigned int)offsets[i];
    const size_t want = std::max<size_t>(total, 1);
    RC_TRY(grow(sh, sh.ac_idx[buf], sh.ac_cap[buf], want));
    RC_TRY(grow(sh, sh.ac_r2, sh.ac_r2s, want));
    HIP_TRY(hipMemcpy(sh.ac_begin[buf], base.data(), padded * sizeof(unsigned int), hipMemcpyHostToDevice));
    if (total > 0) {
        MurbNbrArgs fa = na;
        fa.base = sh.ac_begin[buf];
        fa.out_idx = sh.ac_idx[buf];
        fa.out_r2 = sh.ac_r2;
        fa.capacity = (unsigned int)std::min<size_t>(sh.ac_cap[buf], sh.ac_r2s);   // >= total: no place lies beyond it
        RC_TRY(nbr_sweep(c, sh, fa, cut.grid, true));
    }
    c->ac_offsets.swap(offsets);
    c->ac_longest = longest;
    c->ac_empty = empty;
    return 0;
}

MurbAcArgs ac_args(const murbhip_ctx* c, const Shard& sh, int parts, float dt, int elapsed)
{
    MurbAcArgs a{};
    a.h = hermite_args(c, sh, parts, dt, 1);
    a.h.rec_out = sh.rec[c->cur ^ 1];
    a.f_cur = sh.ac_out;
    a.f_new = sh.ac_out + 7 * c->in.n;
    a.irr = sh.ac_force;
    a.reg = sh.ac_force + 6 * c->in.n;
    a.n = (unsigned int)c->in.n;
    a.elapsed = elapsed;
    return a;
}

// what a step of either kind leaves behind: the Hermite step's bookkeeping, with the scheme still live
void ac_stepped(murbhip_ctx* c, float dt)
{
    c->cur ^= 1;
    invalidate_cached_forces(c);
    c->herm_current = true;   // (a1, j1) of this step are the next step's (a0, j0)
    c->herm_in_acc_out = true;
    c->ac_live = true;
    ++c->ac_steps;
    c->ac_time += (double)dt;
}

// The scheme is over; an extrapolated total is no Hermite evaluation and is not kept as one.  Every call that ends a live
// scheme without replacing the bodies comes through here: murbac_end, a failed step, and the calls that step the bodies another
// way (the others go through invalidate_cached_forces, which drops the Hermite memory anyway).
void ac_finish(murbhip_ctx* c)
{
    if (c->ac_live && c->ac_m != 0) { c->herm_current = false; c->herm_proposal = false; }
    c->ac_live = false;
}

int ac_irregular_step(murbhip_ctx* c, Shard& sh, int parts, float dt)
{
    const unsigned pairs = (unsigned)(c->in.slots / 2);
    MurbAcPredictArgs pa{};
    pa.rec = sh.rec[c->cur];
    pa.vel = sh.vel;
    pa.a0 = sh.herm_a0;
    pa.j0 = sh.herm_j0;
    pa.src = sh.ac_src;
    pa.count = (int)c->in.n;
    pa.stride = (unsigned int)c->in.slots;
    pa.dt = dt;
    RC_TRY(timed_launch(c, sh, kProfAcPredict, [&] {   // the two small launches have span kinds of their own
        hipLaunchKernelGGL(murb_ac_predict_kernel, dim3((unsigned)((c->in.n + 255) / 256)), dim3(256), 0, sh.compute, pa);
    }));
    RC_TRY(ac_sweep(c, sh, c->ac_buf, sh.ac_out));
    const MurbAcArgs a = ac_args(c, sh, parts, dt, c->ac_m + 1);
    RC_TRY(timed_launch(c, sh, kProfAcCorrect, [&] {
        hipLaunchKernelGGL(murb_ac_correct_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, a);
    }));
    ac_stepped(c, dt);
    ++c->ac_m;
    return 0;
}

int ac_regular_step(murbhip_ctx* c, Shard& sh, int parts, float dt)
{
    const unsigned pairs = (unsigned)(c->in.slots / 2);
    MurbHermiteArgs p = hermite_args(c, sh, parts, dt, 1);
    p.rec_out = sh.herm_rec;
    p.vel_out = sh.herm_vel;
    hipLaunchKernelGGL(murb_hermite_predict_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, p);
    RC_TRY(hip_rc(hipGetLastError()));
    RC_TRY(ac_pack(c, sh, sh.herm_rec, sh.herm_vel));
    RC_TRY(ac_sweep(c, sh, c->ac_buf, sh.ac_out));                          // (aIo, jIo): the old lists
    RC_TRY(enqueue_hermite_sweep(c, sh, sh.herm_rec, sh.herm_vel, parts));    // the rows of (a1, j1)
    RC_TRY(ac_rebuild(c, sh, sh.herm_rec, c->ac_buf ^ 1));                  // nothing of the bodies has changed where this fails
    RC_TRY(ac_sweep(c, sh, c->ac_buf ^ 1, sh.ac_out + 7 * c->in.n));        // (aIn, jIn): the new lists
    const MurbAcArgs a = ac_args(c, sh, parts, dt, c->ac_nirr);
    RC_TRY(timed_launch(c, sh, kProfAcCorrect, [&] {
        hipLaunchKernelGGL(murb_ac_regular_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, a);
    }));
    ac_stepped(c, dt);
    c->ac_buf ^= 1;
    c->ac_m = 0;
    ++c->ac_regular;
    return 0;
}

int ac_begin(murbhip_ctx* c, const std::vector<float>& thr, int n_irr)
{
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    ac_finish(c);
    const size_t n = c->in.n;
    const int parts = hermite_parts(c->in);
    RC_TRY(ac_ensure(c, sh));
    std::vector<int> all(n);
    for (size_t i = 0; i < n; ++i) all[i] = (int)i;
    HIP_TRY(hipMemcpy(sh.ac_in, thr.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sh.ac_in + n, all.data(), n * sizeof(int), hipMemcpyHostToDevice));
    RC_TRY(enqueue_hermite(c, 0.f, 0));   // (a0, j0): murbhip_compute_acc_jerk's
    RC_TRY(ac_pack(c, sh, sh.rec[c->cur], sh.vel));
    RC_TRY(ac_rebuild(c, sh, sh.rec[c->cur], 0));
    RC_TRY(ac_sweep(c, sh, 0, sh.ac_out + 7 * n));
    MurbAcArgs a = ac_args(c, sh, parts, 0.f, n_irr);
    a.begin = 1;
    hipLaunchKernelGGL(murb_ac_regular_kernel, dim3((unsigned)((c->in.slots / 2 + 255) / 256)), dim3(256), 0, sh.compute, a);
    RC_TRY(hip_rc(hipGetLastError()));
    c->ac_live = true;
    c->ac_nirr = n_irr;
    c->ac_m = 0;
    c->ac_buf = 0;
    c->ac_steps = c->ac_regular = 0;
    c->ac_time = 0.0;
    return 0;
}

// all of a group's pointers, or none of them
inline bool all_or_none(std::initializer_list<const void*> group)
{
    size_t set = 0;
    for (const void* q : group) set += q != nullptr;
    return set == 0 || set == group.size();
}

// The argument checks the entry points of the point read-outs share.  Each entry point keeps the order null context, count == 0,
// field_state, arguments, which decides the error a caller sees.
// every listed body in [0, n); no list: all n bodies in order where the entry point takes that (count == n), refused where not
inline bool bodies_valid(const murbhip_ctx* c, unsigned long count, const int* bodies, bool null_is_all)
{
    if (!bodies) return null_is_all && count == c->in.n;
    for (unsigned long i = 0; i < count; ++i)
        if (bodies[i] < 0 || (long)bodies[i] >= (long)c->in.n) return false;
    return true;
}
// every coordinate of every plane finite; a null plane is one the caller may leave out
inline bool planes_finite(unsigned long count, std::initializer_list<const float*> planes)
{
    for (const float* q : planes)
        for (unsigned long i = 0; q && i < count; ++i)
            if (!std::isfinite(q[i])) return false;
    return true;
}
// every skip entry a body or -1 (none); no list: no point skips a body
inline bool skips_valid(const murbhip_ctx* c, unsigned long count, const int* skip)
{
    for (unsigned long i = 0; skip && i < count; ++i)
        if (skip[i] < -1 || (long)skip[i] >= (long)c->in.n) return false;
    return true;
}

inline int field_state(const murbhip_ctx* c)
{
    // the bodies of an open block sit at different times; several shards or ranks: not covered
    return !c->uploaded || c->in.world != 1 || c->shards.size() != 1 || c->blk_open ? MURBHIP_E_STATE : 0;
}

}  // namespace

// ===================================================================================== C ABI
extern "C" {

int murbhip_version(void) { return 103; }   // 1.03: murbhip_warmup, murbhip_init_bodies, the potential out of the force evaluation

const char* murbhip_error_string(int code)
{
    static thread_local char buf[160];
    if (code == 0) return "success";
    if (code == MURBHIP_E_INVALID) return "murbhip: invalid argument";
    if (code == MURBHIP_E_STATE) return "murbhip: call made in the wrong state (upload first?)";
    if (code == MURBHIP_E_NO_DEVICE) return "murbhip: no usable HIP device";
    if (code == MURBHIP_E_NO_RCCL) return "murbhip: librccl could not be loaded";
    if (code == MURBHIP_E_NOMEM) return "murbhip: host allocation failed";
    if (code <= -3000 && code > -4000) {
        Rccl& r = rccl();
        snprintf(buf, sizeof buf, "RCCL error %d: %s", -code - 3000,
                 (r.ok && r.GetErrorString) ? r.GetErrorString(-code - 3000) : "?");
        return buf;
    }
    if (code < 0 && code > -2000) {
        snprintf(buf, sizeof buf, "HIP error %d: %s", -code, hipGetErrorString((hipError_t)(-code)));
        return buf;
    }
    snprintf(buf, sizeof buf, "murbhip: unknown code %d", code);
    return buf;
}

int murbhip_partition(unsigned long n, int world, int rank, unsigned long* first, unsigned long* count)
{
    if (world < 1 || rank < 0 || rank >= world || !first || !count) return MURBHIP_E_INVALID;
    partition(n, world, rank, first, count);
    return 0;
}

unsigned long murbhip_slice_slots(unsigned long n, int world) { return world < 1 ? 0 : slice_slots(n, world); }

unsigned long murbhip_slot_of_body(unsigned long n, int world, unsigned long i)
{
    if (world < 1 || i >= n) return ~0ul;
    const unsigned long base = n / (unsigned long)world, rem = n % (unsigned long)world;
    // ranks < rem own base+1 bodies, the rest own base
    unsigned long r, first;
    if (i < rem * (base + 1)) { r = i / (base + 1); first = r * (base + 1); }
    else { r = rem + (base ? (i - rem * (base + 1)) / base : 0); first = rem * (base + 1) + (r - rem) * base; }
    return r * slice_slots(n, world) + (i - first);
}

int murbhip_schedule_items(unsigned long n, int world, int rank, int split, int* pairs, unsigned long capacity,
                           unsigned long* count, unsigned long* own_count)
{
    if (world < 1 || world > MURB_SYM_MAX_RANKS || rank < 0 || rank >= world || !count || !own_count) return MURBHIP_E_INVALID;
    if (split != 1 && split != 2 && split != 4 && split != 8 && split != 16) return MURBHIP_E_INVALID;
    std::vector<int> flat;
    int own = 0;
    sym_schedule_items(world, rank, (int)(slice_slots(n, world) / MURB_SYM_BLOCK), split, sym_fill(n, world), flat, &own);
    *count = flat.size() / 2;
    *own_count = (unsigned long)own;
    if (pairs) {
        if (capacity < flat.size() / 2) return MURBHIP_E_INVALID;
        std::memcpy(pairs, flat.data(), flat.size() * sizeof(int));
    }
    return 0;
}

int murbhip_schedule_layout(unsigned long n, int world, int rank, int split, int waves, int taper_pct, int tri_first_pct,
                            int exchange_mode, long* items, unsigned long item_capacity, unsigned long* item_count, long* rows,
                            unsigned long row_capacity, unsigned long* row_count, unsigned long* floats_main,
                            unsigned long* floats_tri)
{
    if (world < 1 || world > MURB_SYM_MAX_RANKS || rank < 0 || rank >= world || !item_count || !row_count) return MURBHIP_E_INVALID;
    if (split != 1 && split != 2 && split != 4 && split != 8 && split != 16) return MURBHIP_E_INVALID;
    if ((waves != 4 && waves != 8) || taper_pct < 0 || (taper_pct & 0xff) > 100 || taper_pct > 0x7ff || tri_first_pct < 0 || tri_first_pct > 100)
        return MURBHIP_E_INVALID;
    if (MURB_SYM_BLOCK / split < 16 * waves) return MURBHIP_E_INVALID;
    SymHostLayout L;
    SymLayoutKey key;
    key.split = split; key.waves = waves; key.taper = taper_pct & 0xff; key.diag_tri = (taper_pct & 0x100) != 0;
    key.exchange_mode = exchange_mode != 0 || world > 1;
    key.overlap = 1; key.tri_first_pct = tri_first_pct; key.tri_div = 1 << ((taper_pct >> 9) & 3);
    plan_sym_layout(world, rank, sym_fill(n, world), key, L);
    *item_count = L.items.size();
    *row_count = L.table_main.size() + L.table_tri.size();
    if (floats_main) *floats_main = L.floats_main;
    if (floats_tri) *floats_tri = L.floats_tri;
    if (items) {
        if (item_capacity < L.items.size()) return MURBHIP_E_INVALID;
        const bool ex = key.exchange_mode;
        for (size_t k = 0; k < L.items.size(); ++k) {
            const MurbSymItem& it = L.items[k];
            long* o = items + 8 * k;
            o[0] = it.i_slot0; o[1] = (long)it.ngroups * waves * MURB_SYM_R; o[2] = it.J; o[3] = it.flags;
            o[4] = (ex && (int)k < L.own) ? 1 : 0;
            o[5] = (long)it.ioff; o[6] = (long)it.joff;
            o[7] = !ex ? 0 : ((int)k < L.t1 ? 0 : ((int)k < L.own ? 1 : 2));
        }
    }
    if (rows) {
        if (row_capacity < *row_count) return MURBHIP_E_INVALID;
        size_t e = 0;
        for (int set = 0; set < 2; ++set)
            for (const MurbSymBlockRows& br : (set == 0 ? L.table_main : L.table_tri)) {
                long* o = rows + 7 * e++;
                o[0] = set; o[1] = br.out_slice; o[2] = br.out_block; o[3] = (long)br.base_i; o[4] = br.ni; o[5] = (long)br.base_j; o[6] = br.nj;
            }
    }
    return 0;
}

int murbhip_device_count(int* count)
{
    if (!count) return MURBHIP_E_INVALID;
    *count = 0;
    return hip_rc(hipGetDeviceCount(count));
}

int murbhip_create(murbhip_ctx** out, unsigned long n, float soft, float g, int device)
{
    const int rank0 = 0;
    return create_common(out, n, soft, g, 1, 1, &device, &rank0, 0, false);
}

int murbhip_create_sharded(murbhip_ctx** out, unsigned long n, float soft, float g, int ndev, const int* devices,
                           int exchange)
{
    if (ndev < 1 || ndev > 64 || !devices || (exchange != 0 && exchange != 1)) return MURBHIP_E_INVALID;
    if ((unsigned long)ndev > n) return MURBHIP_E_INVALID;
    std::vector<int> ranks(ndev);
    for (int i = 0; i < ndev; ++i) ranks[i] = i;
    if (exchange == 1) {
        if (!rccl().ok) return MURBHIP_E_NO_RCCL;
    }
    RC_TRY(create_common(out, n, soft, g, ndev, ndev, devices, ranks.data(), exchange, false));
    if (exchange == 1 && ndev > 1) {
        std::vector<rccl_comm_t> comms(ndev);
        const int rc = nccl_rc(rccl().CommInitAll(comms.data(), ndev, devices));
        if (rc != 0) { murbhip_destroy(*out); *out = nullptr; return rc; }
        for (int i = 0; i < ndev; ++i) (*out)->shards[i].comm_rccl = comms[i];
    }
    return 0;
}

int murbhip_unique_id(void* id_out)
{
    if (!id_out) return MURBHIP_E_INVALID;
    Rccl& r = rccl();
    if (!r.ok) return MURBHIP_E_NO_RCCL;
    rccl_id_t id;
    RC_TRY(nccl_rc(r.GetUniqueId(&id)));
    std::memcpy(id_out, &id, sizeof id);
    return 0;
}

int murbhip_create_rank(murbhip_ctx** out, unsigned long n, float soft, float g, int device, int rank, int world,
                        const void* unique_id)
{
    if (world < 1 || rank < 0 || rank >= world || (unsigned long)world > n) return MURBHIP_E_INVALID;
    if (world > MURB_SYM_MAX_RANKS) return MURBHIP_E_INVALID;   // fixed-size per-rank tables (MurbPeerPtrs)
    if (world > 1 && !unique_id) return MURBHIP_E_INVALID;
    if ((world > 1 || unique_id) && !rccl().ok) return MURBHIP_E_NO_RCCL;
    RC_TRY(create_common(out, n, soft, g, world, 1, &device, &rank, 1, true));
    if (world > 1 || unique_id) {   // a one-rank communicator is legal and exercises the whole RCCL binding
        rccl_id_t id;
        std::memcpy(&id, unique_id, sizeof id);
        int rc = hip_rc(hipSetDevice(device));
        if (rc == 0) rc = nccl_rc(rccl().CommInitRank(&(*out)->shards[0].comm_rccl, world, id, rank));
        if (rc != 0) { murbhip_destroy(*out); *out = nullptr; return rc; }
    }
    return 0;
}

int murbhip_destroy(murbhip_ctx* c)
{
    if (!c) return 0;
    delete c->crew;   // joins the shards' threads (idle: every entry point returns only when they have finished enqueueing)
    c->crew = nullptr;
    for (Shard& sh : c->shards) {
        (void)hipSetDevice(sh.device);
        drain(sh.compute); drain(sh.comm); drain(sh.compute_low);
        if (sh.comm_rccl && rccl().ok) rccl().CommDestroy(sh.comm_rccl);
        for (hipEvent_t& e : sh.prof) release_event(e);
        for (hipEvent_t* e : {&sh.ev_tri, &sh.ev_integrated, &sh.ev_gathered, &sh.ev_rowsum, &sh.ev_reduced}) release_event(*e);
        for (hipStream_t* q : {&sh.compute_low, &sh.compute, &sh.comm}) release_stream(*q);
        release(sh.rec[0], sh.rec[1], sh.vel, sh.accp, sh.acc_out, sh.phi_out, sh.mass, sh.radius, sh.metrics);
        if (sh.metrics_host) (void)hipHostFree(sh.metrics_host);
        release(sh.herm_rec, sh.herm_vel, sh.herm_a0, sh.herm_j0, sh.herm_part, sh.herm_ctl);
        if (sh.herm_ctl_host) (void)hipHostFree(sh.herm_ctl_host);
        release(sh.blk_ctl, sh.blk_ticks, sh.blk_levels, sh.blk_list, sh.blk_rec, sh.blk_vel, sh.blk_part);
        release(sh.nn_idx, sh.nn_r2, sh.enc);
        release(sh.herm_phi, sh.pot_sums);
        release(sh.fld_in, sh.fld_pts, sh.fld_out, sh.fld_part);
        release(sh.trc_state, sh.trc_pts, sh.trc_part);
        release(sh.knn_part_r2, sh.knn_part_idx, sh.knn_list_r2, sh.knn_list_idx, sh.knn_rho, sh.knn_sums);
        release(sh.nbr_part, sh.nbr_counts, sh.nbr_base, sh.nbr_idx, sh.nbr_r2);
        release(sh.bnd_in, sh.bnd_part, sh.bnd_idx, sh.bnd_h, sh.bnd_elems, sh.bnd_flag, sh.bnd_sums);
        release(sh.pot_in, sh.pot_rec, sh.pot_member, sh.pot_part, sh.pot_phi, sh.pot_e, sh.pot_rows);
        release(sh.mst_label, sh.mst_rec, sh.mst_in, sh.mst_part, sh.mst_idx, sh.mst_r2);
        release(sh.sep_in, sh.sep_member, sh.sep_rec, sh.sep_part, sh.sep_sum, sh.sep_rows, sh.sep_total);
        release(sh.lst_src, sh.lst_range, sh.lst_pts);
        release(sh.ac_src, sh.ac_in, sh.ac_pts, sh.ac_part, sh.ac_r2, sh.ac_out, sh.ac_force);
        release(sh.ac_begin[0], sh.ac_begin[1], sh.ac_len[0], sh.ac_len[1], sh.ac_idx[0], sh.ac_idx[1]);
        if (sh.pot_sums_host) (void)hipHostFree(sh.pot_sums_host);
        if (sh.blk_ctl_host) (void)hipHostFree(sh.blk_ctl_host);
        release(sh.sym_items, sh.sym_send, sh.sym_recv, sh.sym_p2p, sh.sym_tri_acc, sh.sym_acc64);
        free_sym_set(sh, sh.sym_main); free_sym_set(sh, sh.sym_tri);
    }
    delete c;
    return 0;
}

int murbhip_upload(murbhip_ctx* c, const float* qx, const float* qy, const float* qz, const float* vx, const float* vy,
                   const float* vz, const float* m)
{
    if (!c || !qx || !qy || !qz || !vx || !vy || !vz || !m) return MURBHIP_E_INVALID;
    RC_TRY(murbhip_sync(c));
    {   // how far apart two bodies can be: decides the form of the pair-symmetric kernel's pair factor ("sym_wide")
        double reach2 = (double)c->soft2;
        for (const float* q : {qx, qy, qz}) {
            float lo = q[0], hi = q[0];
            bool finite = true;
            for (unsigned long i = 0; i < c->in.n; ++i) {
                lo = std::min(lo, q[i]);
                hi = std::max(hi, q[i]);
                finite = finite && std::isfinite(q[i]);
            }
            const double extent = finite ? (double)hi - (double)lo : (double)INFINITY;
            reach2 += extent * extent;
        }
        c->sym_wide_needed = sym_wide_needed(std::sqrt(reach2), std::sqrt((double)c->soft2));
    }
    // positions + GM for every slot (replicated), velocities for each local slice
    std::vector<float4> rec(c->in.slots, make_float4(0.f, 0.f, 0.f, 0.f));
    for (int r = 0; r < c->in.world; ++r) {
        unsigned long first, count;
        partition(c->in.n, c->in.world, r, &first, &count);
        pack_records(qx, qy, qz, m, c->g, true, first, count, (unsigned long)r * c->in.slice, rec);
    }
    for (Shard& sh : c->shards) {
        HIP_TRY(hipSetDevice(sh.device));
        std::vector<float4> vel(c->in.slice, make_float4(0.f, 0.f, 0.f, 0.f));
        pack_records(vx, vy, vz, nullptr, 0.f, false, sh.first, sh.count, 0, vel);
        HIP_TRY(hipMemcpy(sh.rec[0], rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(sh.rec[1], rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(sh.vel, vel.data(), vel.size() * sizeof(float4), hipMemcpyHostToDevice));
        RC_TRY(shard_alloc(sh, sh.mass, c->in.slice * sizeof(float)));
        std::vector<float> mass(c->in.slice, 0.f);
        std::copy(m + sh.first, m + sh.first + sh.count, mass.begin());
        HIP_TRY(hipMemcpy(sh.mass, mass.data(), mass.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    bodies_loaded(c);
    if (c->contact) RC_TRY(enqueue_radii_lanes(c));   // the velocity records were replaced; the radii stay
    return 0;
}

namespace {
// The 61 generator words around the first value rand() returns after srand(seed): glibc's srandom_r / random_r for the
// default TYPE_3 state (stdlib/random_r.c: 31 words from a 16807 Lehmer sequence, taps 3 apart, 310 outputs discarded).
MurbRandBase rand_base_words(unsigned int seed)
{
    int32_t st[MURB_RAND_DEG];
    int32_t word = seed == 0 ? 1 : (int32_t)seed;
    st[0] = word;
    for (int i = 1; i < MURB_RAND_DEG; ++i) {
        const long hi = word / 127773, lo = word % 127773;
        word = (int32_t)(16807 * lo - 2836 * hi);
        if (word < 0) word += 2147483647;
        st[i] = word;
    }
    const int discard = 10 * MURB_RAND_DEG, first = discard - MURB_RAND_DEG, count = 2 * MURB_RAND_DEG - 1;
    MurbRandBase b{};
    int f = 3, r = 0;
    for (int t = 0; t < first + count; ++t) {
        const uint32_t val = (uint32_t)st[f] + (uint32_t)st[r];
        st[f] = (int32_t)val;
        if (t >= first) b.u[t - first] = val;
        f = (f + 1) % MURB_RAND_DEG;
        r = (r + 1) % MURB_RAND_DEG;
    }
    return b;
}
}  // namespace

int murbhip_init_bodies(murbhip_ctx* c, const char* scheme, unsigned long seed)
{
    if (!c || !scheme) return MURBHIP_E_INVALID;
    const std::string sc(scheme);
    const bool galaxy = sc == "galaxy";
    if (!galaxy && sc != "random") return MURBHIP_E_INVALID;
    RC_TRY(murbhip_sync(c));
    const unsigned long draws = galaxy ? 4ul * (c->in.n - 1) : 7ul * c->in.n;
    const MurbRandBase base = rand_base_words((unsigned int)seed);
    // glibc picks its FMA build of sincosf on CPUs with FMA and AVX2 (sysdeps/x86_64/fpu/multiarch/ifunc-fma.h)
    const bool fma = c->init_libm_fma >= 0 ? c->init_libm_fma != 0 : (__builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2"));
    for (Shard& sh : c->shards) {
        HIP_TRY(hipSetDevice(sh.device));
        for (float** p : {&sh.mass, &sh.radius}) RC_TRY(shard_alloc(sh, *p, c->in.slice * sizeof(float)));
        unsigned int* d_draws = nullptr;
        HIP_TRY(hipMalloc((void**)&d_draws, std::max(draws, 1ul) * sizeof(unsigned int)));
        int rc = 0;
        const unsigned long chunks = (draws + MURB_RAND_CHUNK - 1) / MURB_RAND_CHUNK;
        if (chunks) hipLaunchKernelGGL(murb_rand_fill_kernel, dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, sh.compute, base, draws, d_draws);
        rc = hip_rc(hipGetLastError());
        // padding slots: position 0, mass 0, like the records murbhip_upload packs
        if (!rc) rc = hip_rc(hipMemsetAsync(sh.rec[0], 0, c->in.slots * sizeof(float4), sh.compute));
        if (!rc) rc = hip_rc(hipMemsetAsync(sh.rec[1], 0, c->in.slots * sizeof(float4), sh.compute));
        if (!rc) rc = hip_rc(hipMemsetAsync(sh.vel, 0, c->in.slice * sizeof(float4), sh.compute));
        if (!rc) rc = hip_rc(hipMemsetAsync(sh.mass, 0, c->in.slice * sizeof(float), sh.compute));
        if (!rc) rc = hip_rc(hipMemsetAsync(sh.radius, 0, c->in.slice * sizeof(float), sh.compute));
        if (!rc) {
            MurbInitArgs a{};
            a.draws = d_draws; a.rec0 = sh.rec[0]; a.rec1 = sh.rec[1]; a.vel = sh.vel; a.mass = sh.mass; a.radius = sh.radius;
            a.n = c->in.n; a.world = (unsigned int)c->in.world; a.rank = (unsigned int)sh.rank; a.slice = (unsigned int)c->in.slice; a.g = c->g;
            const dim3 grid((unsigned)((c->in.n + 255) / 256));
            if (!galaxy) hipLaunchKernelGGL(murb_init_random_kernel, grid, dim3(256), 0, sh.compute, a);
            else if (fma) hipLaunchKernelGGL((murb_init_galaxy_kernel<true>), grid, dim3(256), 0, sh.compute, a);
            else hipLaunchKernelGGL((murb_init_galaxy_kernel<false>), grid, dim3(256), 0, sh.compute, a);
            rc = hip_rc(hipGetLastError());
        }
        const int rs = hip_rc(hipStreamSynchronize(sh.compute));
        release(d_draws);
        if (rc || rs) return rc ? rc : rs;
    }
    c->sym_wide_needed = false;   // the reference's schemes span 1e9 m: the fast form of the pair-symmetric kernel ("sym_wide")
    bodies_loaded(c);
    if (c->contact) RC_TRY(enqueue_radii_lanes(c));   // the scheme's radii
    return 0;
}

int murbhip_download_mass(murbhip_ctx* c, float* m, float* r)
{
    if (!c || !m) return MURBHIP_E_INVALID;
    if (!c->uploaded) return MURBHIP_E_STATE;
    RC_TRY(murbhip_sync(c));
    std::vector<float> buf(c->in.slice);
    for (Shard& sh : c->shards) {
        HIP_TRY(hipSetDevice(sh.device));
        HIP_TRY(hipMemcpy(buf.data(), sh.mass, buf.size() * sizeof(float), hipMemcpyDeviceToHost));
        std::memcpy(m + sh.first, buf.data(), sh.count * sizeof(float));
        if (r) {
            if (!sh.radius) return MURBHIP_E_STATE;   // radii exist on the device only after murbhip_init_bodies or murbhip_upload_radii
            HIP_TRY(hipMemcpy(buf.data(), sh.radius, buf.size() * sizeof(float), hipMemcpyDeviceToHost));
            std::memcpy(r + sh.first, buf.data(), sh.count * sizeof(float));
        }
    }
    return 0;
}

namespace {
// v + a*h with the product rounded on its own, like the device kicks (murb_kernels.h)
float half_kick(float v, float a, float h)
{
#pragma clang fp contract(off)
    const float k = a * h;
    return v + k;
}
}  // namespace

int murbhip_sync(murbhip_ctx* c)
{
    if (!c) return MURBHIP_E_INVALID;
    int rc = 0;
    for (Shard& sh : c->shards) {
        int r1 = hip_rc(hipSetDevice(sh.device));
        if (!r1) r1 = hip_rc(hipStreamSynchronize(sh.compute));
        if (!r1) r1 = hip_rc(hipStreamSynchronize(sh.compute_low));
        if (!r1) r1 = hip_rc(hipStreamSynchronize(sh.comm));
        if (r1 && !rc) rc = r1;
    }
    if (rc && !c->async_error) c->async_error = rc;
    return c->async_error ? c->async_error : rc;
}

int murbhip_download_state(murbhip_ctx* c, float* qx, float* qy, float* qz, float* vx, float* vy, float* vz)
{
    if (!c) return MURBHIP_E_INVALID;
    if (!c->uploaded) return MURBHIP_E_STATE;
    // leapfrog: the device holds v_{n-1/2}; what the caller gets is v_n = v_{n-1/2} + a(q_n)*dt/2, which
    // costs one force evaluation (in one-process-per-GPU mode that makes this call a collective)
    const bool closing_kick = c->lf_half && (vx || vy || vz);
    if (closing_kick) RC_TRY(enqueue_iteration(c, 0.f, 0));
    RC_TRY(murbhip_sync(c));
    std::vector<float4> rec(c->in.slots), vel(c->in.slice);
    std::vector<float> acc(closing_kick ? 3 * c->in.slice : 0);
    // positions: any shard holds all of them once its exchange has landed (sync above)
    {
        Shard& sh = c->shards[0];
        HIP_TRY(hipSetDevice(sh.device));
        HIP_TRY(hipMemcpy(rec.data(), sh.rec[c->cur], rec.size() * sizeof(float4), hipMemcpyDeviceToHost));
        for (int r = 0; r < c->in.world; ++r) {
            unsigned long first, count;
            partition(c->in.n, c->in.world, r, &first, &count);
            for (unsigned long k = 0; k < count; ++k) {
                const float* const v = slot_values(rec.data(), (unsigned long)r * c->in.slice + k);
                if (qx) qx[first + k] = v[kSlotX];
                if (qy) qy[first + k] = v[kSlotY];
                if (qz) qz[first + k] = v[kSlotZ];
            }
        }
    }
    if (vx || vy || vz) {
        for (Shard& sh : c->shards) {
            HIP_TRY(hipSetDevice(sh.device));
            HIP_TRY(hipMemcpy(vel.data(), sh.vel, vel.size() * sizeof(float4), hipMemcpyDeviceToHost));
            if (closing_kick) HIP_TRY(hipMemcpy(acc.data(), sh.acc_out, acc.size() * sizeof(float), hipMemcpyDeviceToHost));
            const float half = 0.5f * c->lf_last_dt;
            for (unsigned long k = 0; k < sh.count; ++k) {
                const float* const v = slot_values(vel.data(), k);
                float ox = v[kSlotX], oy = v[kSlotY], oz = v[kSlotZ];
                if (closing_kick) {
                    ox = half_kick(ox, acc[k], half);
                    oy = half_kick(oy, acc[c->in.slice + k], half);
                    oz = half_kick(oz, acc[2 * c->in.slice + k], half);
                }
                if (vx) vx[sh.first + k] = ox;
                if (vy) vy[sh.first + k] = oy;
                if (vz) vz[sh.first + k] = oz;
            }
        }
    }
    return 0;
}

int murbhip_download_acc(murbhip_ctx* c, float* ax, float* ay, float* az)
{
    if (!c || !ax || !ay || !az) return MURBHIP_E_INVALID;
    if (!c->uploaded) return MURBHIP_E_STATE;
    RC_TRY(murbhip_sync(c));
    std::vector<float> a(3 * c->in.slice);
    for (Shard& sh : c->shards) {
        HIP_TRY(hipSetDevice(sh.device));
        HIP_TRY(hipMemcpy(a.data(), sh.acc_out, a.size() * sizeof(float), hipMemcpyDeviceToHost));
        std::memcpy(ax + sh.first, a.data(), sh.count * sizeof(float));
        std::memcpy(ay + sh.first, a.data() + c->in.slice, sh.count * sizeof(float));
        std::memcpy(az + sh.first, a.data() + 2 * c->in.slice, sh.count * sizeof(float));
    }
    return 0;
}

int murbhip_compute_acc(murbhip_ctx* c)
{
    if (!c) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->blk_open) return MURBHIP_E_STATE;
    return enqueue_iteration(c, 0.f, 0);
}

int murbhip_compute_acc_jerk(murbhip_ctx* c)
{
    if (!c) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->lf_half || c->blk_open) return MURBHIP_E_STATE;   // a leapfrog run in flight has half-step velocities
    return enqueue_hermite(c, 0.f, 0);
}

int murbhip_download_jerk(murbhip_ctx* c, float* jx, float* jy, float* jz)
{
    if (!c || !jx || !jy || !jz) return MURBHIP_E_INVALID;
    if (!c->uploaded || !c->herm_current) return MURBHIP_E_STATE;
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    std::vector<float> j(3 * c->in.slots);
    HIP_TRY(hipSetDevice(sh.device));
    HIP_TRY(hipMemcpy(j.data(), sh.herm_j0, j.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::memcpy(jx, j.data(), c->in.n * sizeof(float));
    std::memcpy(jy, j.data() + c->in.slots, c->in.n * sizeof(float));
    std::memcpy(jz, j.data() + 2 * c->in.slots, c->in.n * sizeof(float));
    return 0;
}

int murbhip_download_nearest(murbhip_ctx* c, int* idx, float* r2)
{
    if (!c) return MURBHIP_E_INVALID;
    if (!c->uploaded || !c->nearest || !c->herm_current) return MURBHIP_E_STATE;
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    if (idx) HIP_TRY(hipMemcpy(idx, sh.nn_idx, c->in.n * sizeof(int), hipMemcpyDeviceToHost));
    if (r2) HIP_TRY(hipMemcpy(r2, sh.nn_r2, c->in.n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int murbhip_set_encounter(murbhip_ctx* c, float radius)
{
    if (!c || !std::isfinite(radius) || radius < 0.f) return MURBHIP_E_INVALID;
    if (radius > 0.f && !c->nearest) return MURBHIP_E_STATE;
    c->enc_radius = radius;
    return 0;
}

int murbhip_encounters(murbhip_ctx* c, int* i, int* j, float* r2, unsigned long capacity, unsigned long* count, double* time)
{
    if (!c || !count) return MURBHIP_E_INVALID;
    if (!c->uploaded) return MURBHIP_E_STATE;
    return read_hit_list(c, !c->contact, i, j, r2, capacity, count, time);
}

int murbhip_contacts(murbhip_ctx* c, int* i, int* j, float* gap2, unsigned long capacity, unsigned long* count, double* time)
{
    if (!c || !count) return MURBHIP_E_INVALID;
    if (!c->uploaded) return MURBHIP_E_STATE;
    return read_hit_list(c, c->contact != 0, i, j, gap2, capacity, count, time);
}

int murbhip_download_contact(murbhip_ctx* c, int* idx, float* gap2)
{
    if (!c) return MURBHIP_E_INVALID;
    if (!c->uploaded || !c->contact || !c->herm_current) return MURBHIP_E_STATE;
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    if (idx) HIP_TRY(hipMemcpy(idx, sh.nn_idx, c->in.n * sizeof(int), hipMemcpyDeviceToHost));
    if (gap2) HIP_TRY(hipMemcpy(gap2, sh.nn_r2, c->in.n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int murbhip_download_potential(murbhip_ctx* c, float* phi)
{
    if (!c || !phi) return MURBHIP_E_INVALID;
    if (!c->uploaded || !c->potential || !c->herm_current) return MURBHIP_E_STATE;
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    HIP_TRY(hipMemcpy(phi, sh.herm_phi, c->in.n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// w = -1/2 sum_i m_i phi_i of the remembered evaluation: fp64 block sums in fixed order on the device (murb_potential_sum_kernel),
// the block rows added in index order here; the masses as uploaded, like murbhip_energy's metrics.
int murbhip_potential_energy(murbhip_ctx* c, double* w)
{
    if (!c || !w) return MURBHIP_E_INVALID;
    if (!c->uploaded || !c->potential || !c->herm_current) return MURBHIP_E_STATE;
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    const size_t blocks = (sh.count + 255) / 256, cap = (c->in.slots + 255) / 256;
    RC_TRY(shard_alloc(sh, sh.pot_sums, cap * sizeof(double)));
    if (!sh.pot_sums_host) HIP_TRY(hipHostMalloc((void**)&sh.pot_sums_host, cap * sizeof(double), hipHostMallocDefault));
    hipLaunchKernelGGL(murb_potential_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, sh.compute, (const float*)sh.mass,
                       (const float*)sh.herm_phi, sh.pot_sums, (int)sh.count);
    RC_TRY(hip_rc(hipGetLastError()));
    HIP_TRY(hipMemcpyAsync(sh.pot_sums_host, sh.pot_sums, blocks * sizeof(double), hipMemcpyDeviceToHost, sh.compute));
    RC_TRY(murbhip_sync(c));
    double sum = 0.0;
    for (size_t b = 0; b < blocks; ++b) sum += sh.pot_sums_host[b];
    *w = sum;
    return 0;
}

int murbfield_at(murbhip_ctx* c, unsigned long count, const float* px, const float* py, const float* pz, const float* pvx,
                 const float* pvy, const float* pvz, const int* skip, float* ax, float* ay, float* az, float* jx, float* jy,
                 float* jz, float* phi)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!px || !py || !pz || !all_or_none({pvx, pvy, pvz}) || !all_or_none({ax, ay, az}) || !all_or_none({jx, jy, jz})) return MURBHIP_E_INVALID;
    if (!planes_finite(count, {px, py, pz, pvx, pvy, pvz})) return MURBHIP_E_INVALID;
    if (!skips_valid(c, count, skip)) return MURBHIP_E_INVALID;
    const float* const p[6] = {px, py, pz, pvx, pvy, pvz};
    float* const out[7] = {ax, ay, az, jx, jy, jz, phi};
    return field_run(c, count, p, skip, false, out);
}

int murbfield_of(murbhip_ctx* c, unsigned long count, const int* bodies, float* ax, float* ay, float* az, float* jx, float* jy,
                 float* jz, float* phi)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!bodies_valid(c, count, bodies, false) || !all_or_none({ax, ay, az}) || !all_or_none({jx, jy, jz})) return MURBHIP_E_INVALID;
    float* const out[7] = {ax, ay, az, jx, jy, jz, phi};
    return field_run(c, count, nullptr, bodies, true, out);
}

int murbfield_layout(unsigned long n, long chunks_option, long batch_option, unsigned long* out4)
{
    if (n == 0 || !out4 || !murb_field_options_valid(chunks_option, batch_option)) return MURBHIP_E_INVALID;
    const MurbFieldLayout l = murb_field_layout(n, chunks_option, batch_option);
    const unsigned long count = out4[3];
    out4[0] = (unsigned long)l.chunks;
    out4[1] = l.groups;
    out4[2] = murb_field_batches(l, count);
    out4[3] = l.rows;
    return 0;
}

int murbfield_set_option(murbhip_ctx* c, const char* key, long value)
{
    if (!c || !key) return MURBHIP_E_INVALID;
    const std::string k(key);
    if (k != "field_chunks" && k != "field_batch") return MURBHIP_E_INVALID;
    const bool chunks = k == "field_chunks";
    if (!murb_field_options_valid(chunks ? value : 0, chunks ? 0 : value)) return MURBHIP_E_INVALID;
    (chunks ? c->field_chunks : c->field_batch) = value;   // read through field_layout by every point read-out
    return 0;
}

int murbfield_get_option(murbhip_ctx* c, const char* key, long* value)
{
    if (!c || !key || !value) return MURBHIP_E_INVALID;
    const std::string k(key);
    const MurbFieldLayout l = murb_field_layout(c->in.n, c->field_chunks, c->field_batch);   // as resolved
    if (k == "field_chunks") *value = l.chunks;
    else if (k == "field_batch") *value = (long)l.batch;
    else return MURBHIP_E_INVALID;
    return 0;
}

int murbtidal_at(murbhip_ctx* c, unsigned long count, const float* px, const float* py, const float* pz, const int* skip,
                 float* txx, float* tyy, float* tzz, float* txy, float* txz, float* tyz)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!px || !py || !pz || !all_or_none({txx, tyy, tzz, txy, txz, tyz})) return MURBHIP_E_INVALID;
    if (!planes_finite(count, {px, py, pz})) return MURBHIP_E_INVALID;
    if (!skips_valid(c, count, skip)) return MURBHIP_E_INVALID;
    const float* const p[3] = {px, py, pz};
    float* const out[6] = {txx, tyy, tzz, txy, txz, tyz};
    return tidal_run(c, count, p, skip, false, out);
}

int murbtidal_of(murbhip_ctx* c, unsigned long count, const int* bodies, float* txx, float* tyy, float* tzz, float* txy, float* txz,
                 float* tyz)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!bodies_valid(c, count, bodies, false) || !all_or_none({txx, tyy, tzz, txy, txz, tyz})) return MURBHIP_E_INVALID;
    float* const out[6] = {txx, tyy, tzz, txy, txz, tyz};
    return tidal_run(c, count, nullptr, bodies, true, out);
}

// ---- include/murbknn.h
namespace {
inline bool knn_k_valid(int k, int least) { return k >= least && k <= MURBKNN_KMAX; }

// the checks murbknn_of and murbdensity_of share; 1: nothing to do
int knn_of_checks(murbhip_ctx* c, int k, int least, unsigned long count, const int* bodies)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 1;
    RC_TRY(field_state(c));
    return knn_k_valid(k, least) && bodies_valid(c, count, bodies, true) ? 0 : MURBHIP_E_INVALID;
}
}  // namespace

int murbknn_of(murbhip_ctx* c, int k, unsigned long count, const int* bodies, int* idx, float* r2)
{
    const int rc = knn_of_checks(c, k, 1, count, bodies);
    if (rc != 0) return rc == 1 ? 0 : rc;
    return knn_run(c, k, count, nullptr, bodies, true, idx, r2, nullptr, false);
}

int murbknn_at(murbhip_ctx* c, int k, unsigned long count, const float* px, const float* py, const float* pz, const int* skip,
               int* idx, float* r2)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!knn_k_valid(k, 1) || !px || !py || !pz) return MURBHIP_E_INVALID;
    if (!planes_finite(count, {px, py, pz})) return MURBHIP_E_INVALID;
    if (!skips_valid(c, count, skip)) return MURBHIP_E_INVALID;
    const float* const p[3] = {px, py, pz};
    return knn_run(c, k, count, p, skip, false, idx, r2, nullptr, false);
}

int murbdensity_of(murbhip_ctx* c, int k, unsigned long count, const int* bodies, float* rho)
{
    const int rc = knn_of_checks(c, k, 2, count, bodies);
    if (rc != 0) return rc == 1 ? 0 : rc;
    if (!rho) return MURBHIP_E_INVALID;
    return knn_run(c, k, count, nullptr, bodies, true, nullptr, nullptr, rho, false);
}

int murbdensity_centre(murbhip_ctx* c, int k, double* out8)
{
    if (!c) return MURBHIP_E_INVALID;
    RC_TRY(field_state(c));
    if (!knn_k_valid(k, 2) || !out8) return MURBHIP_E_INVALID;
    return knn_centre(c, k, out8);
}

int murbknn_merge(int k, const int* idx_a, const float* r2_a, const int* idx_b, const float* r2_b, int* idx_out, float* r2_out)
{
    if (!knn_k_valid(k, 1) || !idx_a || !r2_a || !idx_b || !r2_b || !idx_out || !r2_out) return MURBHIP_E_INVALID;
    murb_knn_merge(k, idx_a, r2_a, idx_b, r2_b, idx_out, r2_out);
    return 0;
}

int murbknn_density(int k, const int* idx, const float* r2, const float* masses, float soft, float* rho_out)
{
    if (!knn_k_valid(k, 2) || !idx || !r2 || !masses || !rho_out) return MURBHIP_E_INVALID;
    *rho_out = murb_knn_density(k, idx, r2, masses, soft * soft);
    return 0;
}

// ---- include/murbbind.h
int murbbind_of(murbhip_ctx* c, unsigned long count, const int* bodies, int* partner, float* h)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!bodies_valid(c, count, bodies, true)) return MURBHIP_E_INVALID;
    return bind_run(c, count, nullptr, bodies, true, partner, h, false);
}

int murbbind_at(murbhip_ctx* c, unsigned long count, const float* px, const float* py, const float* pz, const float* pvx,
                const float* pvy, const float* pvz, const float* m, const int* skip, int* partner, float* h)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!px || !py || !pz || !all_or_none({pvx, pvy, pvz})) return MURBHIP_E_INVALID;
    if (!planes_finite(count, {px, py, pz, pvx, pvy, pvz})) return MURBHIP_E_INVALID;
    for (unsigned long i = 0; m && i < count; ++i)
        if (!std::isfinite(m[i]) || m[i] < 0.f) return MURBHIP_E_INVALID;
    if (!skips_valid(c, count, skip)) return MURBHIP_E_INVALID;
    std::vector<float> gm;
    if (m) {
        gm.resize(count);
        for (unsigned long i = 0; i < count; ++i) gm[i] = c->g * m[i];   // the upload's one fp32 multiply (pack_records)
    }
    const float* const p[7] = {px, py, pz, pvx, pvy, pvz, m ? gm.data() : nullptr};
    return bind_run(c, count, p, skip, false, partner, h, false);
}

int murbbind_pairs(murbhip_ctx* c, int* i, int* j, double* elems, unsigned long capacity, unsigned long* count, double* out8)
{
    if (!c) return MURBHIP_E_INVALID;
    RC_TRY(field_state(c));
    if (!count || !out8 || !all_or_none({i, j, elems})) return MURBHIP_E_INVALID;
    return bind_pairs(c, i, j, elems, capacity, count, out8);
}

int murbbind_elements(float g, float soft, const float* qi, const float* vi, float mi, const float* qj, const float* vj, float mj,
                      double* out6)
{
    if (!qi || !vi || !qj || !vj || !out6) return MURBHIP_E_INVALID;
    for (const float* q : {qi, vi, qj, vj})
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(q[k])) return MURBHIP_E_INVALID;
    for (const float v : {g, soft, mi, mj})
        if (!std::isfinite(v) || v < 0.f) return MURBHIP_E_INVALID;
    murb_bind_elements(soft * soft, qi, vi, g * mi, mi, qj, vj, g * mj, mj, out6);
    return 0;
}

// ---- include/murbbound.h
int murbpot_of(murbhip_ctx* c, unsigned long count, const int* bodies, const unsigned char* member, float* phi)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!phi || !bodies_valid(c, count, bodies, true)) return MURBHIP_E_INVALID;
    return pot_call(c, count, nullptr, bodies, true, member, phi);
}

int murbpot_at(murbhip_ctx* c, unsigned long count, const float* px, const float* py, const float* pz, const int* skip,
               const unsigned char* member, float* phi)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!px || !py || !pz || !phi) return MURBHIP_E_INVALID;
    if (!planes_finite(count, {px, py, pz})) return MURBHIP_E_INVALID;
    if (!skips_valid(c, count, skip)) return MURBHIP_E_INVALID;
    const float* const p[3] = {px, py, pz};
    return pot_call(c, count, p, skip, false, member, phi);
}

int murbbound_members(murbhip_ctx* c, const unsigned char* start, const double* frame_v, int max_iter, unsigned char* member, double* e,
                      double* out16)
{
    if (!c) return MURBHIP_E_INVALID;
    RC_TRY(field_state(c));
    if (!out16 || max_iter < 1 || max_iter > 4096) return MURBHIP_E_INVALID;
    for (int k = 0; frame_v && k < 3; ++k)
        if (!std::isfinite(frame_v[k])) return MURBHIP_E_INVALID;
    return bound_members(c, start, frame_v, max_iter, member, e, out16);
}

int murbbound_radii(unsigned long n, const float* qx, const float* qy, const float* qz, const float* m, const unsigned char* member,
                    const double* centre3, int nfrac, const double* frac, double* radii)
{
    if (nfrac < 0 || !centre3) return MURBHIP_E_INVALID;
    if (nfrac == 0) return 0;
    if (!frac || !radii || (n > 0 && (!qx || !qy || !qz || !m))) return MURBHIP_E_INVALID;
    for (const float* q : {qx, qy, qz, m})
        for (unsigned long i = 0; i < n; ++i)
            if (!std::isfinite(q[i]) || (q == m && q[i] < 0.f)) return MURBHIP_E_INVALID;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(centre3[k])) return MURBHIP_E_INVALID;
    for (int f = 0; f < nfrac; ++f)
        if (!(frac[f] > 0.0 && frac[f] <= 1.0)) return MURBHIP_E_INVALID;
    murb_bound_radii(n, qx, qy, qz, m, member, centre3, nfrac, frac, radii);
    return 0;
}

// ---- include/murbsep.h
int murbsep_of(murbhip_ctx* c, unsigned long count, const int* bodies, const unsigned char* member, double* sum, int lo_exp, int sub, int bins,
               unsigned long long* hist, unsigned long long* out4)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!sep_request_valid(sum, lo_exp, sub, bins, hist, out4) || !bodies_valid(c, count, bodies, true)) return MURBHIP_E_INVALID;
    return sep_call(c, count, nullptr, bodies, true, member, sum, lo_exp, sub, bins, hist, out4);
}

int murbsep_at(murbhip_ctx* c, unsigned long count, const float* px, const float* py, const float* pz, const unsigned char* member,
               double* sum, int lo_exp, int sub, int bins, unsigned long long* hist, unsigned long long* out4)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!sep_request_valid(sum, lo_exp, sub, bins, hist, out4) || !px || !py || !pz) return MURBHIP_E_INVALID;
    if (!planes_finite(count, {px, py, pz})) return MURBHIP_E_INVALID;
    const float* const p[3] = {px, py, pz};
    return sep_call(c, count, p, nullptr, false, member, sum, lo_exp, sub, bins, hist, out4);
}

int murbsep_bin(int lo_exp, int sub, int bins, float d2)
{
    if (!murb_sep_params_valid(lo_exp, sub, bins)) return MURBHIP_E_INVALID;
    return murb_sep_bin(lo_exp, sub, bins, d2);
}

int murbsep_edges(int lo_exp, int sub, int bins, float* edge2, double* edge_r)
{
    if (!murb_sep_params_valid(lo_exp, sub, bins) || (!edge2 && !edge_r)) return MURBHIP_E_INVALID;
    for (int k = 0; k <= bins; ++k) {
        const float e = murb_sep_edge2(lo_exp, sub, k);
        if (edge2) edge2[k] = e;
        if (edge_r) edge_r[k] = std::sqrt((double)e);
    }
    return 0;
}

// ---- include/murbmst.h
int murbforeign_of(murbhip_ctx* c, unsigned long count, const int* bodies, const int* label, int* partner, float* r2)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!label || !partner || !r2 || !bodies_valid(c, count, bodies, true)) return MURBHIP_E_INVALID;
    return foreign_call(c, count, bodies, label, partner, r2);
}

int murbmst_of(murbhip_ctx* c, const unsigned char* member, unsigned long capacity, int* ei, int* ej, float* er2, double* elen, int* label,
               double* out8)
{
    if (!c) return MURBHIP_E_INVALID;
    RC_TRY(field_state(c));
    if (!out8) return MURBHIP_E_INVALID;
    return mst_call(c, member, capacity, ei, ej, er2, elen, label, out8);
}

int murbmst_round(unsigned long n, int* label, const int* partner, const float* r2, int* ei, int* ej, float* er2, unsigned long capacity,
                  unsigned long* edges)
{
    if (!edges || (n > 0 && (!label || !partner || !r2))) return MURBHIP_E_INVALID;
    std::vector<int> next(label, label + n);
    std::vector<MurbMstEdge> chosen;
    if (!murb_mst_round(n, next.data(), partner, r2, chosen)) return MURBHIP_E_INVALID;
    if ((ei || ej || er2) && *edges + chosen.size() > capacity) return MURBHIP_E_INVALID;
    for (size_t e = 0; e < chosen.size(); ++e) {
        if (ei) ei[*edges + e] = chosen[e].i;
        if (ej) ej[*edges + e] = chosen[e].j;
        if (er2) er2[*edges + e] = chosen[e].r2;
    }
    std::copy(next.begin(), next.end(), label);
    *edges += chosen.size();
    return 0;
}

int murbmst_cut(unsigned long n, unsigned long edges, const int* ei, const int* ej, const float* er2, float thr, int* label)
{
    if ((n > 0 && !label) || (edges > 0 && (!ei || !ej || !er2)) || thr != thr) return MURBHIP_E_INVALID;
    return murb_mst_cut(n, edges, ei, ej, er2, thr, label) ? 0 : MURBHIP_E_INVALID;
}

// ---- include/murbnbr.h
namespace {
// the radii of a call, checked, as thresholds; false: a radius that is negative or not finite
bool nbr_thresholds(const murbhip_ctx* c, unsigned long count, const float* h, float h_all, std::vector<float>& thr)
{
    const auto valid = [](float v) { return std::isfinite(v) && v >= 0.f; };
    if (!h && !valid(h_all)) return false;
    for (unsigned long i = 0; h && i < count; ++i)
        if (!valid(h[i])) return false;
    thr.resize(count);
    for (unsigned long i = 0; i < count; ++i) thr[i] = murb_nbr_threshold(h ? h[i] : h_all, c->soft2);
    return true;
}
}  // namespace

int murbnbr_of(murbhip_ctx* c, unsigned long count, const int* bodies, const float* h, float h_all, unsigned long* offsets, int* idx,
               float* r2, unsigned long capacity)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!offsets || !bodies_valid(c, count, bodies, true)) return MURBHIP_E_INVALID;
    std::vector<float> thr;
    if (!nbr_thresholds(c, count, h, h_all, thr)) return MURBHIP_E_INVALID;
    return nbr_run(c, count, nullptr, bodies, true, thr, offsets, idx, r2, capacity);
}

int murbnbr_at(murbhip_ctx* c, unsigned long count, const float* px, const float* py, const float* pz, const int* skip, const float* h,
               float h_all, unsigned long* offsets, int* idx, float* r2, unsigned long capacity)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!px || !py || !pz || !offsets) return MURBHIP_E_INVALID;
    if (!planes_finite(count, {px, py, pz})) return MURBHIP_E_INVALID;
    if (!skips_valid(c, count, skip)) return MURBHIP_E_INVALID;
    std::vector<float> thr;
    if (!nbr_thresholds(c, count, h, h_all, thr)) return MURBHIP_E_INVALID;
    const float* const p[3] = {px, py, pz};
    return nbr_run(c, count, p, skip, false, thr, offsets, idx, r2, capacity);
}

int murbnbr_set_option(murbhip_ctx* c, const char* key, long value)
{
    if (!c || !key || std::string(key) != "list_entries" || !murb_nbr_option_valid(value)) return MURBHIP_E_INVALID;
    c->nbr_list_entries = value;   // read by the radius read-out's fill pass alone
    return 0;
}

int murbnbr_get_option(murbhip_ctx* c, const char* key, long* value)
{
    if (!c || !key || !value || std::string(key) != "list_entries") return MURBHIP_E_INVALID;
    *value = (long)murb_nbr_entries(c->nbr_list_entries);   // as resolved
    return 0;
}

int murbnbr_threshold(float h, float soft, float* thr)
{
    if (!thr || !std::isfinite(h) || h < 0.f || !std::isfinite(soft) || soft < 0.f) return MURBHIP_E_INVALID;
    *thr = murb_nbr_threshold(h, soft * soft);
    return 0;
}

int murbnbr_cut(unsigned long count, const unsigned long* offsets, unsigned long first, unsigned long entries, unsigned long* last)
{
    if (!offsets || !last || first >= count) return MURBHIP_E_INVALID;
    *last = murb_nbr_cut(count, offsets, first, entries);
    return 0;
}

// ---- include/murblist.h
int murblist_of(murbhip_ctx* c, unsigned long count, const int* bodies, const unsigned long* offsets, const int* idx, float* ax, float* ay,
                float* az, float* jx, float* jy, float* jz, float* phi)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!bodies_valid(c, count, bodies, true) || !all_or_none({ax, ay, az}) || !all_or_none({jx, jy, jz})) return MURBHIP_E_INVALID;
    if (!murb_list_valid(count, offsets, idx, c->in.n)) return MURBHIP_E_INVALID;
    float* const out[7] = {ax, ay, az, jx, jy, jz, phi};
    return list_run(c, count, nullptr, bodies, true, offsets, idx, out);
}

int murblist_at(murbhip_ctx* c, unsigned long count, const float* px, const float* py, const float* pz, const float* pvx, const float* pvy,
                const float* pvz, const unsigned long* offsets, const int* idx, float* ax, float* ay, float* az, float* jx, float* jy,
                float* jz, float* phi)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!px || !py || !pz || !all_or_none({pvx, pvy, pvz}) || !all_or_none({ax, ay, az}) || !all_or_none({jx, jy, jz})) return MURBHIP_E_INVALID;
    if (!planes_finite(count, {px, py, pz, pvx, pvy, pvz})) return MURBHIP_E_INVALID;
    if (!murb_list_valid(count, offsets, idx, c->in.n)) return MURBHIP_E_INVALID;
    const float* const p[6] = {px, py, pz, pvx, pvy, pvz};
    float* const out[7] = {ax, ay, az, jx, jy, jz, phi};
    return list_run(c, count, p, nullptr, false, offsets, idx, out);
}

int murbsplit_of(murbhip_ctx* c, unsigned long count, const int* bodies, const float* h, float h_all, unsigned long* counts, float* ax,
                 float* ay, float* az, float* jx, float* jy, float* jz, float* phi)
{
    if (!c) return MURBHIP_E_INVALID;
    if (count == 0) return 0;
    RC_TRY(field_state(c));
    if (!bodies_valid(c, count, bodies, true) || !all_or_none({ax, ay, az}) || !all_or_none({jx, jy, jz})) return MURBHIP_E_INVALID;
    std::vector<float> thr;
    if (!nbr_thresholds(c, count, h, h_all, thr)) return MURBHIP_E_INVALID;
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    RC_TRY(list_pack(c, sh));
    float* const out[7] = {ax, ay, az, jx, jy, jz, phi};
    for (float* plane : out)   // the ranges without an entry are never swept: +0
        if (plane) std::fill(plane, plane + count, 0.f);
    std::vector<unsigned long> offsets(count + 1, 0ul);
    std::vector<unsigned int> range;
    std::vector<float> results;
    // a filled range of the neighbour read-out, consumed where it is: its points packed with their velocities into records of
    // this read-out's own (the fill pass keeps the launch's points in fld_pts), its entries read from the list buffer
    const NbrConsume consume = [&](unsigned long first, unsigned long lo, unsigned long hi, size_t cap) -> int {
        const unsigned long npts = hi - lo;
        RC_TRY(grow(sh, sh.lst_pts, sh.lst_points, 2 * npts));
        const StagedPoints bodies_of_range{nullptr, (const int*)(sh.fld_in + kFieldIntPlane * cap) + lo};   // where stage_points left the launch's bodies
        RC_TRY(pack_points(c, sh, bodies_of_range, sh.lst_pts, npts, npts, 0, false));
        list_range(offsets.data() + first, lo, hi, range);
        return list_sweep(c, sh, sh.lst_pts, npts, range, out, first + lo, results);
    };
    RC_TRY(nbr_run(c, count, nullptr, bodies, true, thr, offsets.data(), nullptr, nullptr, ~0ul, &consume));
    for (unsigned long i = 0; counts && i < count; ++i) counts[i] = offsets[i + 1] - offsets[i];
    return 0;
}

// ---- include/murbac.h
int murbac_begin(murbhip_ctx* c, const float* h, float h_all, int n_irr)
{
    if (!c || !murb_ac_nirr_valid(n_irr)) return MURBHIP_E_INVALID;
    std::vector<float> thr;
    if (!nbr_thresholds(c, c->in.n, h, h_all, thr)) return MURBHIP_E_INVALID;
    RC_TRY(ac_requirements(c));
    const int rc = ac_begin(c, thr, n_irr);
    if (rc) c->ac_live = false;
    return rc;
}

int murbac_steps(murbhip_ctx* c, float dt, int steps)
{
    if (!c || !std::isfinite(dt) || !(dt > 0.f) || steps < 0) return MURBHIP_E_INVALID;
    RC_TRY(ac_requirements(c));
    if (!c->ac_live) return MURBHIP_E_STATE;
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    const int parts = hermite_parts(c->in);
    if (steps > 0) RC_TRY(ensure_hermite(c, sh, parts));
    for (int i = 0; i < steps; ++i) {
        const int rc = c->ac_m + 1 < c->ac_nirr ? ac_irregular_step(c, sh, parts, dt) : ac_regular_step(c, sh, parts, dt);
        if (rc) {   // the bodies stand at the end of the last completed step
            ac_finish(c);
            return rc;
        }
    }
    return 0;
}

int murbac_end(murbhip_ctx* c)
{
    if (!c) return MURBHIP_E_INVALID;
    ac_finish(c);
    return 0;
}

int murbac_state(murbhip_ctx* c, double out[16])
{
    if (!c || !out) return MURBHIP_E_INVALID;
    std::fill(out, out + 16, 0.0);
    if (!c->ac_live) return 0;
    const double total = (double)c->ac_offsets[c->in.n];
    const double values[9] = {(double)c->ac_nirr, (double)c->ac_m, (double)c->ac_steps, (double)c->ac_regular, total, (double)c->ac_longest,
                              (double)c->ac_empty, total / (double)c->in.n, c->ac_time};
    std::copy(values, values + 9, out);
    return 0;
}

int murbac_lists(murbhip_ctx* c, unsigned long* offsets, int* idx, unsigned long capacity)
{
    if (!c || !offsets) return MURBHIP_E_INVALID;
    if (!c->ac_live) return MURBHIP_E_STATE;
    std::copy(c->ac_offsets.begin(), c->ac_offsets.end(), offsets);
    if (!idx && capacity == 0) return 0;
    const unsigned long total = c->ac_offsets[c->in.n];
    if (!idx || total > capacity) return MURBHIP_E_INVALID;   // idx untouched: the caller sizes it from the offsets
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    if (total) HIP_TRY(hipMemcpy(idx, sh.ac_idx[c->ac_buf], total * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int murbac_forces(murbhip_ctx* c, float* irr[6], float* reg[6], float* reg2[3], float* reg3[3])
{
    if (!c) return MURBHIP_E_INVALID;
    if (!c->ac_live) return MURBHIP_E_STATE;
    const std::pair<float* const*, int> groups[4] = {{irr, 6}, {reg, 6}, {reg2, 3}, {reg3, 3}};
    for (const auto& g : groups)
        for (int k = 0; g.first && k < g.second; ++k)
            if (!g.first[k]) return MURBHIP_E_INVALID;
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    const size_t n = c->in.n;
    size_t plane = 0;   // ac_force: aI jI | aR jR | a2R | a3R, three planes each
    for (const auto& g : groups) {
        for (int k = 0; g.first && k < g.second; ++k)
            HIP_TRY(hipMemcpy(g.first[k], sh.ac_force + (plane + k) * n, n * sizeof(float), hipMemcpyDeviceToHost));
        plane += g.second;
    }
    return 0;
}

// ---- include/murbtracer.h
int murbtracer_validate(unsigned long count, const float* qx, const float* qy, const float* qz, const float* vx, const float* vy,
                        const float* vz)
{
    const float* const q[3] = {qx, qy, qz};
    const float* const v[3] = {vx, vy, vz};
    return count <= (1ul << 30) && murb_tracer_upload_valid(count, q, v) ? 0 : MURBHIP_E_INVALID;
}

int murbtracer_upload(murbhip_ctx* c, unsigned long count, const float* qx, const float* qy, const float* qz, const float* vx,
                      const float* vy, const float* vz)
{
    if (!c) return MURBHIP_E_INVALID;
    if (c->integrator != 2 || c->in.world != 1 || c->shards.size() != 1 || c->force_exchange || c->blk_open) return MURBHIP_E_STATE;
    RC_TRY(murbtracer_validate(count, qx, qy, qz, vx, vy, vz));
    if (count == 0) return murbtracer_clear(c);
    RC_TRY(murbhip_sync(c));   // enqueued steps still carry the old set
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    RC_TRY(ensure_tracers(sh, count));
    const size_t cap = sh.trc_cap;
    std::vector<float> host(6 * cap, 0.f);
    const float* const src[6] = {qx, qy, qz, vx, vy, vz};
    for (int k = 0; k < 6; ++k)
        if (src[k]) std::memcpy(host.data() + k * cap, src[k], count * sizeof(float));
    HIP_TRY(hipMemcpy(sh.trc_state, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    if (c->tracer_dt) c->herm_proposal = false;   // the retained step was proposed for another set
    c->tracers = count;
    c->trc_current = false;
    return 0;
}

int murbtracer_clear(murbhip_ctx* c)
{
    if (!c) return MURBHIP_E_INVALID;
    if (c->blk_open) return MURBHIP_E_STATE;
    if (!c->tracers) return 0;
    RC_TRY(murbhip_sync(c));
    if (c->tracer_dt) c->herm_proposal = false;
    c->tracers = 0;
    c->trc_current = false;
    return 0;
}

int murbtracer_count(murbhip_ctx* c, unsigned long* count)
{
    if (!c || !count) return MURBHIP_E_INVALID;
    *count = c->tracers;
    return 0;
}

int murbtracer_compute(murbhip_ctx* c)
{
    if (!c) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->blk_open || c->shards.size() != 1) return MURBHIP_E_STATE;
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    return enqueue_tracer_evaluation(c, sh);
}

namespace {
// planes [first, first + 6) of the tracers' state into the caller's arrays (null: not asked for)
int tracer_read(murbhip_ctx* c, int first, float* const (&out)[6])
{
    RC_TRY(murbhip_sync(c));
    if (!c->tracers) return 0;
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    const size_t cap = sh.trc_cap;
    std::vector<float> host(6 * cap);
    HIP_TRY(hipMemcpy(host.data(), sh.trc_state + (size_t)first * cap, host.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int k = 0; k < 6; ++k)
        if (out[k]) std::memcpy(out[k], host.data() + k * cap, c->tracers * sizeof(float));
    return 0;
}
}  // namespace

int murbtracer_download(murbhip_ctx* c, float* qx, float* qy, float* qz, float* vx, float* vy, float* vz)
{
    if (!c) return MURBHIP_E_INVALID;
    float* const out[6] = {qx, qy, qz, vx, vy, vz};
    return tracer_read(c, 0, out);
}

int murbtracer_download_forces(murbhip_ctx* c, float* ax, float* ay, float* az, float* jx, float* jy, float* jz)
{
    if (!c || !all_or_none({ax, ay, az}) || !all_or_none({jx, jy, jz})) return MURBHIP_E_INVALID;
    if (!c->tracers || !c->trc_current) return MURBHIP_E_STATE;
    float* const out[6] = {ax, ay, az, jx, jy, jz};
    return tracer_read(c, 6, out);
}

int murbtracer_set_option(murbhip_ctx* c, const char* key, long value)
{
    if (!c || !murb_tracer_option_valid(key, value)) return MURBHIP_E_INVALID;
    const std::string k(key);
    if (k == "tracer_dt") {
        if (c->tracers && c->tracer_dt != (int)value) c->herm_proposal = false;   // the retained step was proposed under the other rule
        c->tracer_dt = (int)value;
    } else if (k == "tracer_chunks") {
        if (c->tracer_chunks != value) c->trc_current = false;   // another cut of the row sums
        c->tracer_chunks = value;
    } else c->tracer_batch = value;
    return 0;
}

int murbtracer_get_option(murbhip_ctx* c, const char* key, long* value)
{
    if (!c || !key || !value) return MURBHIP_E_INVALID;
    const std::string k(key);
    const MurbFieldLayout l = tracer_layout(c);   // as resolved
    if (k == "tracer_chunks") *value = l.chunks;
    else if (k == "tracer_batch") *value = (long)l.batch;
    else if (k == "tracer_dt") *value = c->tracer_dt;
    else return MURBHIP_E_INVALID;
    return 0;
}

int murbhip_upload_radii(murbhip_ctx* c, const float* r)
{
    if (!c || !r) return MURBHIP_E_INVALID;
    for (unsigned long i = 0; i < c->in.n; ++i)
        if (!std::isfinite(r[i]) || r[i] < 0.f) return MURBHIP_E_INVALID;
    if (c->blk_open || c->in.world != 1 || c->shards.size() != 1) return MURBHIP_E_STATE;
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    RC_TRY(shard_alloc(sh, sh.radius, c->in.slice * sizeof(float)));
    std::vector<float> buf(c->in.slice, 0.f);
    std::copy(r, r + c->in.n, buf.begin());
    HIP_TRY(hipMemcpy(sh.radius, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
    c->trc_current = false;   // murbtracer.h: the tracers stay, their remembered evaluation goes
    if (c->contact) {
        invalidate_cached_forces(c);   // the remembered (cp, gap2) belong to the old radii
        RC_TRY(enqueue_radii_lanes(c));
    }
    return 0;
}

int murbhip_evolve(murbhip_ctx* c, double duration, double eta, double eta_start, float dt_min, float dt_max,
                   unsigned long max_steps, double* out5)
{
    if (!c || !out5) return MURBHIP_E_INVALID;
    if (!(duration > 0.0) || !std::isfinite(duration) || !(eta > 0.0) || !(eta_start > 0.0) || !std::isfinite(dt_max) ||
        !(dt_max > 0.f) || !(dt_min >= 0.f) || dt_min > dt_max || max_steps == 0)
        return MURBHIP_E_INVALID;
    if (!c->uploaded || c->integrator != 2 || c->blk_open) return MURBHIP_E_STATE;
    ac_finish(c);                         // murbac.h: these steps end a live scheme, and never start from its extrapolated total
    RC_TRY(enqueue_hermite(c, 0.f, 0));   // refuses several shards; leaves (a0, j0) of the current state remembered
    Shard& sh = c->shards[0];
    RC_TRY(enqueue_tracer_evaluation(c, sh));   // murbtracer.h: beside the bodies' starting evaluation, or alone
    RC_TRY(shard_alloc(sh, sh.herm_ctl, sizeof(MurbEvolveCtl)));
    if (!sh.herm_ctl_host) HIP_TRY(hipHostMalloc((void**)&sh.herm_ctl_host, kEvolveHead, hipHostMallocDefault));
    const int parts = hermite_parts(c->in);
    const unsigned pairs = (unsigned)(c->in.slots / 2);
    const int fresh = c->herm_proposal ? 0 : 1;
    hipLaunchKernelGGL(murb_evolve_begin_kernel, dim3(1), dim3(1), 0, sh.compute, sh.herm_ctl, duration, eta, dt_min, dt_max,
                       (unsigned long long)max_steps, fresh, encounter_threshold(c));
    RC_TRY(hip_rc(hipGetLastError()));
    c->enc_count = 0;
    if (fresh) {
        const MurbHermiteArgs a = hermite_args(c, sh, parts, 0.f, 0);
        hipLaunchKernelGGL(murb_evolve_first_kernel, dim3((pairs + 255) / 256), dim3(256), 0, sh.compute, a, sh.herm_ctl, eta_start);
        RC_TRY(hip_rc(hipGetLastError()));
        if (c->tracers && c->tracer_dt) {   // "tracer_dt" 1: the tracers' starting steps enter the same minimum
            const MurbTracerArgs ta = tracer_args(c, sh, 0.f, 0);
            hipLaunchKernelGGL(murb_tracer_first_kernel, dim3((unsigned)((ta.count + 255) / 256)), dim3(256), 0, sh.compute, ta, sh.herm_ctl, eta_start);
            RC_TRY(hip_rc(hipGetLastError()));
        }
        hipLaunchKernelGGL(murb_evolve_start_kernel, dim3(1), dim3(1), 0, sh.compute, sh.herm_ctl);
        RC_TRY(hip_rc(hipGetLastError()));
    }
    c->evolve_steps = 0;
    // Batches: as many steps as the remaining time takes at the step last seen, kEvolveBatch at the most; a step that
    // grows leaves a tail of no-op launches, one that shrinks another batch.  The first batch of a call without a
    // proposal knows no step yet and is short.
    MurbEvolveCtl& head = *sh.herm_ctl_host;
    unsigned long batch = 4;
    if (!fresh) {
        HIP_TRY(hipMemcpyAsync(&head, sh.herm_ctl, kEvolveHead, hipMemcpyDeviceToHost, sh.compute));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        batch = 0;
    }
    for (;;) {
        if (batch == 0) {   // from the head just read
            const double est = std::ceil((head.duration - head.t) / (double)std::max(head.dt, 1e-30f));
            batch = (unsigned long)std::min<double>(std::max(est, 1.0), (double)kEvolveBatch);
            batch = (unsigned long)std::min<unsigned long long>(batch, head.max_steps - head.steps);
        }
        batch = std::min<unsigned long>(batch, max_steps);
        if (c->evolve_batch > 0) batch = (unsigned long)c->evolve_batch;   // timing aid: fixed length, no-op tail and all
        int rc = 0;
        for (unsigned long k = 0; k < batch && rc == 0; ++k) rc = enqueue_hermite_adaptive(c, sh, parts);
        // the bodies changed whatever happens next; (a1, j1) of the last step taken and its proposal stay with them
        invalidate_cached_forces(c);
        c->herm_current = true;
        c->herm_in_acc_out = true;
        c->herm_proposal = true;
        c->trc_current = c->tracers != 0;   // carried through the same steps
        RC_TRY(rc);
        HIP_TRY(hipMemcpyAsync(&head, sh.herm_ctl, kEvolveHead, hipMemcpyDeviceToHost, sh.compute));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        if (c->async_error) return c->async_error;
        if (head.done) break;
        batch = 0;
    }
    c->evolve_steps = (unsigned long)head.steps;
    c->enc_count = head.enc_hits;
    c->enc_time = head.t;
    out5[0] = head.t;
    out5[1] = (double)head.steps;
    out5[2] = (double)head.used_min;
    out5[3] = (double)head.used_max;
    out5[4] = (double)head.prop;
    return 0;
}

int murbhip_evolve_dts(murbhip_ctx* c, float* dts, unsigned long capacity, unsigned long* count)
{
    if (!c || !count || (!dts && capacity)) return MURBHIP_E_INVALID;
    if (!c->uploaded) return MURBHIP_E_STATE;
    const unsigned long kept = std::min<unsigned long>(c->evolve_steps, MURB_EVOLVE_RING);
    *count = kept;
    if (!dts || kept == 0) return 0;
    if (capacity < kept) return MURBHIP_E_INVALID;
    Shard& sh = c->shards[0];
    RC_TRY(murbhip_sync(c));
    HIP_TRY(hipSetDevice(sh.device));
    std::vector<float> ring(MURB_EVOLVE_RING);
    HIP_TRY(hipMemcpy(ring.data(), sh.herm_ctl->ring, ring.size() * sizeof(float), hipMemcpyDeviceToHost));
    const unsigned long first = c->evolve_steps - kept;   // oldest step kept
    for (unsigned long k = 0; k < kept; ++k) dts[k] = ring[(first + k) % MURB_EVOLVE_RING];
    return 0;
}

int murbhip_evolve_block(murbhip_ctx* c, float dt_max, unsigned long blocks, double eta, double eta_start, int kmax,
                         unsigned long max_steps, double* out8)
{
    if (!c || !out8) return MURBHIP_E_INVALID;
    if (!std::isfinite(dt_max) || !(dt_max > 0.f) || blocks == 0 || blocks > 0xfffffffful || !(eta > 0.0) || !(eta_start > 0.0) ||
        kmax < 0 || kmax > 20 || max_steps == 0 || !std::isnormal(std::ldexp(dt_max, -kmax)))
        return MURBHIP_E_INVALID;
    if (!c->uploaded || c->integrator != 2 || c->tracers) return MURBHIP_E_STATE;   // tracers take no block steps (murbtracer.h)
    if (c->blk_open && (dt_max != c->blk_dt_max || kmax != c->blk_kmax)) return MURBHIP_E_STATE;   // the open block is another grid's
    const bool resume = c->blk_open;
    ac_finish(c);                         // murbac.h: as in murbhip_evolve
    RC_TRY(enqueue_hermite(c, 0.f, 0));   // refuses several shards; leaves (a0, j0) of the current state remembered
    Shard& sh = c->shards[0];
    RC_TRY(ensure_block(c, sh));
    const MurbBlockArgs a = block_args(c, sh);
    hipLaunchKernelGGL(murb_block_begin_kernel, dim3(1), dim3(1), 0, sh.compute, sh.blk_ctl, a, dt_max, kmax, eta, (unsigned int)blocks,
                       (unsigned long long)max_steps, block_units(c), (int)(c->in.slots / MURB_TILE_BODIES),
                       (unsigned int)std::min<size_t>(sh.blk_rows, 0xffffffffu), resume ? 1 : 0, encounter_threshold(c));
    RC_TRY(hip_rc(hipGetLastError()));
    c->enc_count = 0;
    const bool retained = c->blk_have_levels == 1 && dt_max == c->blk_dt_max && kmax == c->blk_kmax;
    const bool given = c->blk_have_levels == 2 && kmax == c->blk_kmax;
    if (!resume && !retained && !given) {
        hipLaunchKernelGGL(murb_block_start_kernel, dim3((unsigned)((sh.count + 255) / 256)), dim3(256), 0, sh.compute, a, sh.blk_ctl, eta_start);
        RC_TRY(hip_rc(hipGetLastError()));
    }
    // Batches.  The first: what the last call's blocks took, 16 steps without one; then what the remaining ticks take at the
    // rate seen so far.  A batch longer than the run needs ends in launches that find `done` set.
    MurbBlockCtl& head = *sh.blk_ctl_host;
    const double T = (double)(1u << kmax);
    double est = c->blk_steps_per_block > 0.0 ? c->blk_steps_per_block * (double)blocks : 16.0;
    for (;;) {
        unsigned long batch = (unsigned long)std::min<double>(std::max(std::ceil(est), 1.0), (double)kBlockBatch);
        if (c->evolve_batch > 0) batch = (unsigned long)c->evolve_batch;   // timing aid: fixed length, no-op tail and all
        int rc = 0;
        for (unsigned long k = 0; k < batch && rc == 0; ++k) rc = enqueue_block_step(c, sh, a);
        // the bodies changed whatever happens next; every body's (a, j) at its own time stay with them
        invalidate_cached_forces(c);
        c->herm_current = true;
        c->herm_in_acc_out = true;
        c->blk_open = true;   // until the head says otherwise
        c->blk_dt_max = dt_max;
        c->blk_kmax = kmax;
        RC_TRY(rc);
        HIP_TRY(hipMemcpyAsync(&head, sh.blk_ctl, sizeof(MurbBlockCtl), hipMemcpyDeviceToHost, sh.compute));
        HIP_TRY(hipStreamSynchronize(sh.compute));
        if (c->async_error) return c->async_error;
        if (head.done) break;
        const double left = (double)head.blocks_left * T - (double)head.clock;
        est = head.ticks_done ? (double)head.steps * left / (double)head.ticks_done : 16.0;
        est = std::min(est, (double)(head.max_steps - head.steps));
    }
    c->blk_open = head.clock != 0u;
    c->blk_have_levels = c->blk_open ? 0 : 1;
    if (head.ticks_done) c->blk_steps_per_block = (double)head.steps * T / (double)head.ticks_done;
    c->blk_info[0] = (double)head.steps;
    c->blk_info[1] = (double)head.body_steps;
    c->blk_info[2] = (double)head.clamped;
    c->blk_info[3] = (double)head.max_act;
    c->enc_count = head.enc_hits;
    c->enc_time = (double)head.ticks_done * head.tick_sec;
    out8[0] = (double)head.ticks_done * head.tick_sec;
    out8[1] = (double)head.steps;
    out8[2] = (double)head.body_steps;
    out8[3] = (double)std::ldexp(dt_max, -(int)head.k_hi);
    out8[4] = (double)std::ldexp(dt_max, -(int)head.k_lo);
    out8[5] = (double)head.clamped;
    out8[6] = (double)head.max_act;
    out8[7] = c->blk_open ? 0.0 : 1.0;
    return 0;
}

int murbhip_block_state(murbhip_ctx* c, unsigned int* ticks, int* levels)
{
    if (!c) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->shards.size() != 1 || !c->shards[0].blk_ticks) return MURBHIP_E_STATE;
    RC_TRY(murbhip_sync(c));
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    if (ticks) HIP_TRY(hipMemcpy(ticks, sh.blk_ticks, c->in.n * sizeof(unsigned int), hipMemcpyDeviceToHost));
    if (levels) HIP_TRY(hipMemcpy(levels, sh.blk_levels, c->in.n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int murbhip_block_set_levels(murbhip_ctx* c, const int* levels, int kmax)
{
    if (!c || !levels || kmax < 0 || kmax > 20) return MURBHIP_E_INVALID;
    for (unsigned long i = 0; i < c->in.n; ++i)
        if (levels[i] < 0 || levels[i] > kmax) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->integrator != 2 || c->blk_open || c->in.world != 1 || c->shards.size() != 1 || c->tracers) return MURBHIP_E_STATE;
    Shard& sh = c->shards[0];
    HIP_TRY(hipSetDevice(sh.device));
    RC_TRY(ensure_block(c, sh));
    RC_TRY(murbhip_sync(c));
    HIP_TRY(hipMemcpy(sh.blk_levels, levels, c->in.n * sizeof(int), hipMemcpyHostToDevice));
    // on the compute stream, and waited for: a fill on the null stream returns before it has run, and the compute stream
    // (non-blocking) does not wait for that stream, so the next call's first launches could still read the ticks of the last block
    HIP_TRY(hipMemsetAsync(sh.blk_ticks, 0, c->in.slots * sizeof(unsigned int), sh.compute));
    HIP_TRY(hipStreamSynchronize(sh.compute));
    c->blk_have_levels = 2;
    c->blk_kmax = kmax;
    ac_finish(c);   // murbac.h: the next steps are block steps
    return 0;
}

int murbhip_warmup(murbhip_ctx* c, double milliseconds)
{
    if (!c || !(milliseconds >= 0.0) || milliseconds > 10000.0) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->blk_open) return MURBHIP_E_STATE;
    // a COUNT fixed by n and the number of ranks, not a clock: in rank mode every evaluation carries collectives, and
    // all ranks must enqueue the same number of them
    const double per_eval_s = (double)c->in.n * (double)c->in.n / (5e12 * (double)c->in.world) + 10e-6;
    const int evaluations = (int)std::min(5000.0, std::ceil(milliseconds * 1e-3 / per_eval_s));
    for (int k = 0; k < evaluations; ++k) {
        c->acc_current = false;   // evaluate again, whatever is remembered
        RC_TRY(enqueue_iteration(c, 0.f, 0));
    }
    c->acc_current = false;       // and nothing of it is kept: the first timed step does all of its own work
    c->pe_current = false;
    return murbhip_sync(c);
}

int murbhip_step(murbhip_ctx* c, float dt)
{
    return murbhip_steps(c, dt, 1);
}

int murbhip_steps(murbhip_ctx* c, float dt, int iterations)
{
    if (!c || iterations < 0) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->blk_open) return MURBHIP_E_STATE;   // an open block (murbhip_evolve_block): the bodies sit at different times
    if (iterations > 0) ac_finish(c);   // murbac.h: these steps end a live scheme, and never start from its extrapolated total
    for (int i = 0; i < iterations; ++i) {
        if (c->integrator == 2) { RC_TRY(enqueue_hermite(c, dt, 1)); continue; }
        RC_TRY(enqueue_iteration(c, dt, 1));
        if (c->integrator == 1) { c->lf_half = true; c->lf_last_dt = dt; }
    }
    return 0;
}

int murbhip_integrate_host_acc(murbhip_ctx* c, const float* ax, const float* ay, const float* az, float dt)
{
    if (!c || !ax || !ay || !az) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->lf_half) return MURBHIP_E_STATE;   // a leapfrog run in flight has half-step velocities
    std::vector<float4> part(c->in.slice);
    for (Shard& sh : c->shards) {
        HIP_TRY(hipSetDevice(sh.device));
        if (c->gather_pending) HIP_TRY(hipStreamWaitEvent(sh.compute, sh.ev_gathered, 0));
        std::fill(part.begin(), part.end(), make_float4(0.f, 0.f, 0.f, 0.f));
        for (unsigned long k = 0; k < sh.count; ++k)
            part[k] = make_float4(ax[sh.first + k], ay[sh.first + k], az[sh.first + k], 0.f);
        RC_TRY(ensure_accp(c, sh));
        HIP_TRY(hipMemcpyAsync(sh.accp, part.data(), part.size() * sizeof(float4), hipMemcpyHostToDevice, sh.compute));
        HIP_TRY(hipStreamSynchronize(sh.compute));   // `part` is reused for the next shard
        RC_TRY(enqueue_integrate(c, sh, 1, dt, 1, nullptr, 0));
    }
    if (c->in.world > 1) {
        RC_TRY(crew_run(c, [&](Shard& sh) { return shard_exchange(c, sh, c->cur ^ 1, 0); }));
        c->gather_pending = true;
    }
    c->cur ^= 1;
    invalidate_cached_forces(c);
    return 0;
}

namespace {
// Leapfrog: the device holds v_{n-1/2}; anything that reports v_n needs a(q_n) (one force evaluation, remembered;
// a collective in one-process-per-GPU mode).
int ensure_acc_for_readout(murbhip_ctx* c)
{
    if (c->lf_half && !c->acc_current) RC_TRY(enqueue_iteration(c, 0.f, 0));
    return 0;
}

// The O(N) sums of the tracked metrics over this process's bodies (murb_metrics_kernel + the block rows added
// in index order on the host).  want_phi: the potential sweep has just been written to phi_out.  pair_sum: also add up
// the pair potentials murbhip_energy has just enqueued into the buffers' tails (then the kept sums are not enough).
int device_metrics(murbhip_ctx* c, bool want_phi, double (&sums)[MURB_METRIC_VALUES], double* pair_sum = nullptr,
                   bool phi_has_self = true)
{
    if (!pair_sum && c->metrics_serial == c->state_serial && (c->metrics_with_phi || !want_phi)) {   // same state, sums already here
        RC_TRY(murbhip_sync(c));
        for (int k = 0; k < MURB_METRIC_VALUES; ++k) sums[k] = c->metrics_sums[k];
        return 0;
    }
    const MetricsLayout l = metrics_layout(c);
    for (Shard& sh : c->shards) {
        HIP_TRY(hipSetDevice(sh.device));
        RC_TRY(shard_alloc(sh, sh.metrics, l.total * sizeof(double)));
        if (c->gather_pending) HIP_TRY(hipStreamWaitEvent(sh.compute, sh.ev_gathered, 0));
        MurbMetricsArgs a{};
        a.rec = sh.rec[c->cur];
        a.vel = sh.vel;
        a.mass = sh.mass;
        a.phi = want_phi ? sh.phi_out : nullptr;
        a.acc = sh.acc_out;
        a.out = sh.metrics;
        a.i_first_slot = (int)((unsigned long)sh.rank * c->in.slice);
        a.count = (int)sh.count;
        a.acc_stride = (unsigned int)c->in.slice;
        a.half_dt = c->lf_half ? 0.5f * c->lf_last_dt : 0.f;
        a.g_over_soft = phi_has_self ? (double)c->g / std::sqrt((double)c->soft2) : 0.0;
        hipLaunchKernelGGL(murb_metrics_kernel, dim3((unsigned)l.blocks), dim3(256), 0, sh.compute, a);
        RC_TRY(hip_rc(hipGetLastError()));
        // the read-out rides behind the kernels on the same stream, into pinned memory: one wait for everything
        if (!sh.metrics_host) HIP_TRY(hipHostMalloc((void**)&sh.metrics_host, l.total * sizeof(double), hipHostMallocDefault));
        HIP_TRY(hipMemcpyAsync(sh.metrics_host, sh.metrics, (pair_sum ? l.total : l.pe_main) * sizeof(double), hipMemcpyDeviceToHost, sh.compute));
    }
    RC_TRY(murbhip_sync(c));
    for (double& v : sums) v = 0.0;
    if (pair_sum) *pair_sum = 0.0;
    for (Shard& sh : c->shards) {
        const double* const host = sh.metrics_host;
        for (size_t b = 0; b < l.blocks; ++b)
            for (int k = 0; k < MURB_METRIC_VALUES; ++k) sums[k] += host[b * MURB_METRIC_VALUES + k];
        if (!pair_sum) continue;
        if (sh.sym_main.part) for (int k = 0; k < kPeSumBlocks; ++k) *pair_sum += host[l.pe_main + k];
        if (sh.sym_tri.part) for (int k = 0; k < kPeSumBlocks; ++k) *pair_sum += host[l.pe_tri + k];
        for (size_t b = 0; b < l.own_blocks * MURB_PE_DIAG_SPLIT; ++b) *pair_sum += host[l.pe_diag + b];
    }
    for (int k = 0; k < MURB_METRIC_VALUES; ++k) c->metrics_sums[k] = sums[k];
    c->metrics_serial = c->state_serial;
    c->metrics_with_phi = want_phi;
    return 0;
}
}  // namespace

int murbhip_energy(murbhip_ctx* c, double* kinetic, double* potential)
{
    if (!c || !kinetic || !potential) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->blk_open) return MURBHIP_E_STATE;
    const Plan main_plan = current_plan(c);
    if (main_plan.symmetric && !c->energy_sweep) {
        // Pair-symmetric plan: the potential energy comes out of a FORCE evaluation (murb_kernels_sym.h, PHI = 2: two more
        // packed instructions per 18 sum G m_i G m_j / r of every pair a wave meets, one float per group of 4 i bodies behind
        // the partial rows) — no second N^2 sweep.  The forces of that evaluation are remembered, so a step that follows only
        // launches the state update (also with several shards): a tracked iteration costs one force evaluation.  Every shard
        // sums the pairs IT evaluated off the diagonal, plus the pairs inside its own blocks (murb_sym_pe_diag_kernel: fp64,
        // no self terms).  Several passes over one shared buffer (one GPU, N > 2.4 M): the groups' sums are added up pass by
        // pass while the evaluation runs (enqueue_sym_passes).
        const MetricsLayout l = metrics_layout(c);
        for (Shard& sh : c->shards) {
            if (sh.metrics) continue;
            HIP_TRY(hipSetDevice(sh.device));
            RC_TRY(shard_alloc(sh, sh.metrics, l.total * sizeof(double)));
        }
        if (!(c->acc_current && c->pe_current)) {
            c->acc_current = false;   // forces alone are not enough: evaluate again, this time with the pair potential
            c->want_pe = true;
            const int rc = enqueue_iteration(c, 0.f, 0);
            c->want_pe = false;
            RC_TRY(rc);
        }
        for (Shard& sh : c->shards) {
            HIP_TRY(hipSetDevice(sh.device));
            const size_t at[2] = {l.pe_main, l.pe_tri};
            int k = 0;
            for (SymSet* st : {&sh.sym_main, &sh.sym_tri}) {
                const size_t off = at[k++];
                if (!st->part || st->passes.size() > 1) continue;   // several passes: summed during the evaluation
                hipLaunchKernelGGL(murb_sym_pe_sum_kernel, dim3(kPeSumBlocks), dim3(1024), 0, sh.compute, st->part + 3 * st->comp_stride,
                                   (unsigned long)(st->comp_stride / MURB_SYM_R + 1), sh.metrics + off, 0);
                RC_TRY(hip_rc(hipGetLastError()));
            }
            // the diagonal blocks (the own slice's) separately, in fp64 and without the bodies' own terms
            hipLaunchKernelGGL(murb_sym_pe_diag_kernel, dim3((unsigned)(l.own_blocks * MURB_PE_DIAG_SPLIT)), dim3(256), 0, sh.compute, sh.rec[c->cur],
                               (int)(sh.rank * l.own_blocks), c->soft2, sh.metrics + l.pe_diag);
            RC_TRY(hip_rc(hipGetLastError()));
        }
        double sums[MURB_METRIC_VALUES], pair_sum = 0.0;
        RC_TRY(device_metrics(c, false, sums, &pair_sum));   // syncs; one copy per shard
        *kinetic = sums[0];
        *potential = -pair_sum / (double)c->g;
        return 0;
    }
    // phi_i = sum_j GM_j / sqrt(r_ij^2 + soft^2), written to the x plane of phi_out: pair-symmetric sweep where the force
    // plan is pair-symmetric (one GPU: one launch; several ranks: the half-ring schedule with its reduce-scatter; over ALL
    // j, self term included and removed by the metrics kernel), the one-sided sweep otherwise (j != i: the sweep leaves
    // the self term out itself, murb_force_body)
    RC_TRY(ensure_acc_for_readout(c));   // before the sweep: it reuses the one-sided partial rows
    Plan p{};
    p.variant = kPotentialKernel;
    {
        const unsigned long tiles_local = c->in.slice / MURB_TILE_BODIES, tiles_remote = (c->in.slots - c->in.slice) / MURB_TILE_BODIES;
        p.parts_local = std::max(1, auto_parts(c->in, 1, c->in.slice, tiles_local));
        p.parts_remote = c->in.world > 1 ? std::max(1, std::min<int>(auto_parts(c->in, 1, c->in.slice, tiles_remote), kMaxParts / 2)) : 0;
    }
    // one shard on the pair-symmetric plan: the sweep is pair-symmetric too (phi_i += G m_j / r, phi_j += G m_i / r:
    // 8 packed + 2 rsq per 4 pair terms instead of 7 + 2 per 2), through the force kernel's partial rows
    const bool symmetric_sweep = main_plan.symmetric && c->in.world == 1 && !c->force_exchange;
    const bool symmetric_multi = main_plan.symmetric && !symmetric_sweep;   // several ranks: the half-ring form
    for (Shard& sh : c->shards) {
        HIP_TRY(hipSetDevice(sh.device));
        RC_TRY(shard_alloc(sh, sh.phi_out, 3 * c->in.slice * sizeof(float)));
    }
    RC_TRY(drain_for_rebuild(c, main_plan));
    if (symmetric_multi) {
        RC_TRY(crew_run(c, [&](Shard& sh) { return shard_potential_sym_multi(c, sh, main_plan); }));
        c->reduce_pending = true;
    }
    for (Shard& sh : c->shards) {
        if (symmetric_multi) break;
        HIP_TRY(hipSetDevice(sh.device));
        if (c->gather_pending) HIP_TRY(hipStreamWaitEvent(sh.compute, sh.ev_gathered, 0));
        if (symmetric_sweep) {
            RC_TRY(build_sym_schedule(c, sh, main_plan));
            if (sh.sym_main.passes.size() > 1) {
                RC_TRY(enqueue_sym_passes(c, sh, true));
                MurbIntegrateArgs a{};   // no state update: phi_out = the accumulated sums
                a.rec_in = sh.rec[c->cur]; a.rec_out = sh.rec[c->cur ^ 1]; a.vel = sh.vel;
                a.acc_out = sh.phi_out;
                a.acc64 = sh.sym_acc64; a.acc64_stride = (unsigned int)c->in.slots;
                a.count = (int)sh.count; a.acc_stride = (unsigned int)c->in.slice;
                hipLaunchKernelGGL(murb_integrate_kernel, dim3((unsigned)((c->in.slice / 2 + 255) / 256)), dim3(256), 0, sh.compute, a);
                RC_TRY(hip_rc(hipGetLastError()));
                continue;
            }
            RC_TRY(enqueue_sym_launch(c, sh, 0, sh.sym_items_total, false, nullptr, true));
            RC_TRY(enqueue_sym_rowsum(sh.sym_main, sh.phi_out, (unsigned int)c->in.slots, sh.compute));
            continue;
        }
        RC_TRY(enqueue_force(c, sh, p, 0));
        if (c->in.world > 1) RC_TRY(enqueue_force(c, sh, p, 1));
        RC_TRY(enqueue_integrate(c, sh, p.parts_local + p.parts_remote, 0.f, 0, nullptr, -1, sh.phi_out));
    }
    double sums[MURB_METRIC_VALUES];
    RC_TRY(device_metrics(c, true, sums, nullptr, main_plan.symmetric));
    *kinetic = sums[0];
    *potential = sums[1];
    return 0;
}

int murbhip_moments(murbhip_ctx* c, double* out10)
{
    if (!c || !out10) return MURBHIP_E_INVALID;
    if (!c->uploaded || c->blk_open) return MURBHIP_E_STATE;
    RC_TRY(ensure_acc_for_readout(c));
    double sums[MURB_METRIC_VALUES];
    RC_TRY(device_metrics(c, false, sums));
    std::memcpy(out10, sums + 2, 10 * sizeof(double));
    return 0;
}

int murbhip_set_option(murbhip_ctx* c, const char* key, long value)
{
    if (!c || !key) return MURBHIP_E_INVALID;
    const std::string k(key);
    if (k == "solo_shard" || k == "force_exchange") c->acc_current = false;   // what acc_out covers changes
    // A key that enters current_plan() or layout_key(): another value means another kernel, another cut of the sums or another
    // layout of the partial rows (rebuilt zeroed, the pair potentials behind them gone).  What is remembered of the force plan
    // belongs to the old value: drop it, so that results are a function of the state and of the options in force when the work
    // is done.  The kept metric sums go with them: murbhip_energy's swept potential is the plan's sweep, and under leapfrog the
    // kinetic energy takes its closing half kick from the plan's forces.  The Hermite memory, the levels and state_serial are
    // not the force plan's and stay.
    const auto plan_key = [c](auto& field, auto v) {
        if (field != v) { c->acc_current = false; c->pe_current = false; c->metrics_serial = c->state_serial - 1; }
        field = v;
    };
    if (k == "variant") { if (value < 0 || value > kNumVariants) return MURBHIP_E_INVALID; plan_key(c->in.variant, (int)value); }
    else if (k == "jsplit") { if (value < 0 || value > kMaxParts / 2) return MURBHIP_E_INVALID; plan_key(c->in.jsplit, (int)value); }
    else if (k == "xcd_order") plan_key(c->xcd_order, value ? 1 : 0);
    else if (k == "pad_aware") plan_key(c->pad_aware, value ? 1 : 0);
    else if (k == "energy_sweep") c->energy_sweep = value ? 1 : 0;
    else if (k == "sym_wide") {
        if (value < -1 || value > 1) return MURBHIP_E_INVALID;
        plan_key(c->sym_wide, (int)value);   // the other form rounds differently
    }
    else if (k == "fuse_integrate") plan_key(c->in.fuse_integrate, value ? 1 : 0);
    else if (k == "exchange_p2p") {
        if (value && (c->exchange != 1 || !rccl().Send || !rccl().Recv)) return MURBHIP_E_STATE;   // needs the RCCL exchange and ncclSend/ncclRecv
        RC_TRY(murbhip_sync(c));
        c->exchange_p2p = value ? 1 : 0;
    }
    else if (k == "tri_div") { if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return MURBHIP_E_INVALID; plan_key(c->in.tri_div, (int)value); }
    else if (k == "init_libm_fma") { if (value < -1 || value > 1) return MURBHIP_E_INVALID; c->init_libm_fma = (int)value; }
    else if (k == "tri_first_pct") { if (value < 0 || value > 100) return MURBHIP_E_INVALID; plan_key(c->tri_first_pct, (int)value); }
    else if (k == "taper") { if (value < -1 || value > 100) return MURBHIP_E_INVALID; plan_key(c->in.taper, (int)value); }
    else if (k == "sym_pass_mb") { if (value < 0) return MURBHIP_E_INVALID; plan_key(c->in.sym_pass_mb, value); }
    else if (k == "diag_tri") { if (value < -1 || value > 1) return MURBHIP_E_INVALID; plan_key(c->in.diag_tri, (int)value); }
    else if (k == "sym_red") { if (value < -1 || value > 1) return MURBHIP_E_INVALID; plan_key(c->in.sym_red, (int)value); }
    else if (k == "sym_waves") { if (value != 0 && value != 4 && value != 8) return MURBHIP_E_INVALID; plan_key(c->in.sym_waves, (int)value); }
    else if (k == "overlap") { if (value < 0 || value > 2) return MURBHIP_E_INVALID; plan_key(c->overlap, (int)value); }
    else if (k == "integrator") {
        if (value < 0 || value > 2) return MURBHIP_E_INVALID;
        if (c->lf_half && value != c->integrator) return MURBHIP_E_STATE;   // half-step velocities on the device: upload first
        if (value == 2 && (c->in.world != 1 || c->shards.size() != 1 || c->force_exchange)) return MURBHIP_E_STATE;   // Hermite: one shard, no exchange (murbhip.h)
        if (value != 2 && (c->nearest || c->contact || c->potential)) return MURBHIP_E_STATE;   // they belong to the Hermite sweeps: switch them off first
        if (value != 2 && c->tracers) return MURBHIP_E_STATE;   // the Hermite steps carry them (murbtracer.h): clear them first
        c->integrator = (int)value;
    }
    else if (k == "evolve_batch") {
        if (value < 0 || value > kEvolveBatch) return MURBHIP_E_INVALID;
        c->evolve_batch = (int)value;
    }
    else if (k == "nearest" || k == "contact" || k == "potential") RC_TRY(set_side_option(c, k, value));
    else if (k == "block_units") {
        if (value < 0 || value > kBlockMaxUnits) return MURBHIP_E_INVALID;
        c->block_units = (int)value;
    }
    else if (k == "solo_shard") c->solo_shard = (int)value;
    else if (k == "cu_reserve") {
        if (value < 0 || value > c->in.cu_count / 2) return MURBHIP_E_INVALID;
        if ((int)value != c->cu_reserve) {
            RC_TRY(murbhip_sync(c));
            for (Shard& sh : c->shards) {
                HIP_TRY(hipSetDevice(sh.device));
                HIP_TRY(hipStreamDestroy(sh.compute)); sh.compute = nullptr;
                HIP_TRY(hipStreamDestroy(sh.compute_low)); sh.compute_low = nullptr;
                RC_TRY(create_compute_streams(c, sh, (int)value));
            }
            c->cu_reserve = (int)value;
        }
    }
    else if (k == "force_exchange") {
        if (value && c->exchange == 1 && !c->shards[0].comm_rccl) return MURBHIP_E_STATE;
        if (value && c->integrator == 2) return MURBHIP_E_STATE;   // the Hermite integrator has no exchange
        c->force_exchange = value ? 1 : 0;
    }
    else if (k == "profile") {
        if (value < 0 || value > 2) return MURBHIP_E_INVALID;
        RC_TRY(murbhip_sync(c));   // spans of the previous setting may still be in flight
        c->profile = (int)value;
        for (Shard& sh : c->shards) {
            HIP_TRY(hipSetDevice(sh.device));
            if (c->profile && sh.prof.empty()) {
                sh.prof.resize(2 * kProfPairs);
                sh.prof_kind.assign(kProfPairs, 0);
                for (hipEvent_t& e : sh.prof) HIP_TRY(hipEventCreate(&e));
            }
            sh.prof_used = 0;
            sh.sym_launches = 0;
        }
    } else return MURBHIP_E_INVALID;
    return 0;
}

int murbhip_get_info(murbhip_ctx* c, const char* key, double* value)
{
    if (!c || !key || !value) return MURBHIP_E_INVALID;
    const std::string k(key);
    const Plan p = current_plan(c);
    if (k == "cu_count") *value = c->in.cu_count;
    else if (k == "clock_mhz") *value = c->clock_mhz;
    else if (k == "n") *value = (double)c->in.n;
    else if (k == "slots") *value = (double)c->in.slots;
    else if (k == "world") *value = c->in.world;
    else if (k == "cu_reserve") *value = c->cu_reserve;
    else if (k == "sym_passes") *value = c->shards[0].sym_main.passes.empty() ? 0.0 : (double)c->shards[0].sym_main.passes.size();
    else if (k == "rank") *value = c->shards[0].rank;
    else if (k == "jsplit") *value = p.symmetric ? (double)p.split
                                     : p.persistent ? (double)p.sched[0].nblocks / std::max(resident_blocks(c->in), 1)
                                                    : (double)(p.parts_local + p.parts_remote);
    else if (k == "hermite_parts") *value = hermite_parts(c->in);   // j chunks of the acceleration + jerk sweep
    else if (k == "block_units") *value = block_units(c);
    else if (k == "block_grid") *value = block_grid(c);
    else if (k == "nearest") *value = c->nearest;
    else if (k == "encounter_count") *value = c->contact ? 0.0 : (double)c->enc_count;
    else if (k == "contact") *value = c->contact;
    else if (k == "potential") *value = c->potential;
    else if (k == "contact_count") *value = c->contact ? (double)c->enc_count : 0.0;
    else if (k == "block_steps") *value = c->blk_info[0];
    else if (k == "block_body_steps") *value = c->blk_info[1];
    else if (k == "block_clamped") *value = c->blk_info[2];
    else if (k == "block_max_active") *value = c->blk_info[3];
    else if (k == "sym_waves") *value = p.symmetric ? p.waves : 0;
    else if (k == "sym_wide") *value = p.symmetric && sym_wide_chosen(c->sym_wide, c->sym_wide_needed) ? 1 : 0;
    else if (k == "taper") *value = p.symmetric ? p.taper : 0;
    else if (k == "workgroups") *value = p.persistent ? p.sched[0].nblocks + (c->in.world > 1 ? p.sched[1].nblocks : 0) : 0;
    else if (k == "variant") *value = p.variant;
    else if (k == "interactions_per_launch") *value = c->interactions_per_launch;
    else if (k == "device_bytes") { double b = 0; for (Shard& sh : c->shards) b += (double)sh.bytes; *value = b; }
    else if (k == "sym_launches") { double v = 0; for (Shard& sh : c->shards) v += (double)sh.sym_launches; *value = v; }
    else if (k == "spans_dropped") {   // 1: the event pool ran out during the profiled steps (averages cover the first part only)
        *value = 0;
        for (Shard& sh : c->shards) if (!sh.prof.empty() && sh.prof_used + 2 > sh.prof.size()) *value = 1;
    }
    else if (k == "force_launches" || k == "force_ms_avg" || k == "force_ms_total" || k.rfind("span_", 0) == 0 || k == "compute_wait_ms_per_step") {
        // Timing spans of the profiled steps ("profile"), over all shards of this process:
        //   force_*                       every force launch (one GPU: the launch; exchange pipeline: T1, R and T2 together)
        //   span_<kind>_ms_avg / _count   kind in tri1, rect, tri2, reduce_scatter, all_gather, wait_gather, wait_reduce, step, field, tidal,
        //                                 tracer, knn, nbr, bind, pot, mst, sep, list, ac_predict, ac_correct
        //   compute_wait_ms_per_step      (wait_gather + wait_reduce) per profiled step: what the exchange costs the compute stream
        static const char* const names[kProfKinds] = {"force", "tri1", "rect", "tri2", "reduce_scatter", "all_gather", "wait_gather",
                                                      "wait_reduce", "step", "field", "tidal", "tracer", "knn", "nbr", "bind", "pot",
                                                      "mst", "sep", "list", "ac_predict", "ac_correct"};
        RC_TRY(murbhip_sync(c));
        double total[kProfKinds] = {0};
        size_t count[kProfKinds] = {0};
        for (Shard& sh : c->shards) {
            HIP_TRY(hipSetDevice(sh.device));
            for (size_t i = 0; i + 1 < sh.prof_used; i += 2) {
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, sh.prof[i], sh.prof[i + 1]));
                const int kind = sh.prof_kind[i / 2];
                total[kind] += ms; ++count[kind];
            }
        }
        const double f_total = total[kProfForce] + total[kProfTri1] + total[kProfRect] + total[kProfTri2];
        const size_t f_count = count[kProfForce] + count[kProfTri1] + count[kProfRect] + count[kProfTri2];
        if (k == "force_launches") *value = (double)f_count;
        else if (k == "force_ms_total") *value = f_total;
        else if (k == "force_ms_avg") *value = f_count ? f_total / (double)f_count : 0.0;
        else if (k == "compute_wait_ms_per_step")
            *value = count[kProfStep] ? (total[kProfWaitGather] + total[kProfWaitReduce]) / (double)count[kProfStep] : 0.0;
        else {
            const bool avg = k.size() > 7 && k.compare(k.size() - 7, 7, "_ms_avg") == 0;
            const bool cnt = k.size() > 6 && k.compare(k.size() - 6, 6, "_count") == 0;
            if (!avg && !cnt) return MURBHIP_E_INVALID;
            const std::string name = k.substr(5, k.size() - 5 - (avg ? 7 : 6));
            int kind = -1;
            for (int q = 0; q < kProfKinds; ++q) if (name == names[q]) kind = q;
            if (kind < 0) return MURBHIP_E_INVALID;
            *value = avg ? (count[kind] ? total[kind] / (double)count[kind] : 0.0) : (double)count[kind];
        }
    } else return MURBHIP_E_INVALID;
    return 0;
}

}  // extern "C"
