// The context behind the C ABI (murbhip_ctx), a shard of it (Shard: one device's streams, buffers and tables), and the small
// helpers every part of murbhip.hip uses: error codes, releases, the counted allocation of a shard's device buffers.
#ifndef MURB_CTX_H_
#define MURB_CTX_H_

#include <hip/hip_runtime.h>

#include <vector>

#include "murb_choose.h"
#include "murb_crew.h"
#include "murb_kernels_block.h"     // murb_kernels_pair.h, _side.h, _hermite.h, _adaptive.h on the way
#include "murb_kernels_field.h"
#include "murb_kernels_sym.h"
#include "murb_kernels_tidal.h"   // behind the others: the kernels before it keep their places in the code object
#include "murb_kernels_tracer.h"  // likewise
#include "murb_kernels_knn.h"     // likewise
#include "murb_kernels_nbr.h"     // likewise
#include "murb_kernels_bind.h"    // likewise
#include "murb_kernels_pot.h"     // likewise
#include "murb_kernels_mst.h"     // likewise
#include "murb_kernels_sep.h"     // likewise
#include "murb_kernels_list.h"    // likewise
#include "murb_kernels_ac.h"      // likewise
#include "murb_rccl.h"

namespace {

// ------------------------------------------------------------------------------------ error codes
inline int hip_rc(hipError_t e) { return e == hipSuccess ? 0 : -(int)e; }
inline int nccl_rc(int r) { return r == 0 ? 0 : -(3000 + r); }   // disjoint from -(hipError_t), which reaches past 1000

// Teardown and error paths: a release that fails cannot be acted on (the context is going away either way).
template <typename... P> inline void release(P*... p) { ((void)hipFree((void*)p), ...); }
inline void release_event(hipEvent_t& e) { if (e) (void)hipEventDestroy(e); e = nullptr; }
inline void release_stream(hipStream_t& s) { if (s) (void)hipStreamDestroy(s); s = nullptr; }
inline void drain(hipStream_t s) { if (s) (void)hipStreamSynchronize(s); }

#define HIP_TRY(expr)                        \
    do {                                     \
        const int rc_ = hip_rc((expr));      \
        if (rc_ != 0) return rc_;            \
    } while (0)
#define RC_TRY(expr)                \
    do {                            \
        const int rc_ = (expr);     \
        if (rc_ != 0) return rc_;   \
    } while (0)

// ------------------------------------------------------------------------------------ context
// Partial rows of one group of launches (murb_kernels_sym.h): the buffer, and per block the row table its row sum reads
// (SymPass, the layout and the planner: murb_plan.h).
struct SymSet {
    float* part = nullptr;
    size_t comp_stride = 0;           // floats per component (single pass)
    MurbSymBlockRows* rows = nullptr; // device copy of the table
    int nblocks = 0;                  // entries (all passes)
    std::vector<SymPass> passes;      // more than one entry: multi-pass evaluation
};

struct Shard {
    int device = 0;
    int rank = 0;
    unsigned long first = 0, count = 0;   // global body range owned
    hipStream_t compute = nullptr, comm = nullptr;
    hipStream_t compute_low = nullptr;   // lowest priority: the own-slice triangle in "overlap" mode 2
    hipEvent_t ev_integrated = nullptr, ev_gathered = nullptr, ev_tri = nullptr;
    float4* rec[2] = {nullptr, nullptr};
    float4* vel = nullptr;
    float4* accp = nullptr;      // one-sided kernels: partial-sum rows, allocated on first use (ensure_accp)
    float* acc_out = nullptr;
    float* phi_out = nullptr;    // murbhip_energy's potential sweep (same shape as acc_out), allocated on first use
    float* mass = nullptr;       // masses of the local slice as uploaded (metrics)
    float* radius = nullptr;     // radii of the local slice: after murbhip_init_bodies or murbhip_upload_radii
    double* metrics = nullptr;   // block sums of murb_metrics_kernel, then murbhip_energy's pair potentials (metrics_doubles)
    double* metrics_host = nullptr;   // its pinned host copy: the read-out is one asynchronous copy behind the kernels
    // pair-symmetric kernel: item table and partial-row layouts (built by build_sym_schedule for one plan)
    MurbSymItem* sym_items = nullptr;
    int sym_items_own = 0, sym_items_total = 0;   // [0, own) = own-slice triangle, the rest need the gathered positions
    SymLayoutKey key;                             // what the tables were built for (sym_layout_key)
    int sym_red = 0;                              // i-side reduction of the plan (kernel template parameter; not part of the tables)
    int sym_t1 = 0;                               // items of the triangle's first launch (exchange pipeline, overlap 1)
    SymSet sym_main;             // one GPU: every item; exchange pipeline: the rectangles (-> reduce-scatter send chunks)
    SymSet sym_tri;              // exchange pipeline: the own-slice triangle (never enters the reduce-scatter)
    float* sym_send = nullptr;   // [world][3][slice]
    float* sym_recv = nullptr;   // [3][slice]
    float* sym_p2p = nullptr;    // "exchange_p2p": chunks received from the floor(W/2) ranks behind this one [floor(W/2)][3][slice]
    float* sym_tri_acc = nullptr;// row sums of sym_tri [3][slice]
    double* sym_acc64 = nullptr; // multi-pass evaluation: fp64 row sums accumulated over the passes [3][slots]
    hipEvent_t ev_rowsum = nullptr, ev_reduced = nullptr;
    rccl_comm_t comm_rccl = nullptr;
    std::vector<hipEvent_t> prof;   // pool of timing events ("profile"): two per recorded span
    size_t prof_used = 0;
    std::vector<int> prof_kind;     // what span k (events 2k, 2k+1) brackets: ProfKind
    // Hermite integrator ("integrator" 2; one shard), allocated on first use (ensure_hermite)
    float4* herm_rec = nullptr;     // predicted positions + GM, all slots
    float4* herm_vel = nullptr;     // predicted velocities
    float* herm_a0 = nullptr;       // ax | ay | az of the remembered evaluation
    float* herm_j0 = nullptr;       // jx | jy | jz of it
    float4* herm_part = nullptr;    // partial rows of the sweep: herm_rows rows of accelerations, then as many of jerks
    int herm_rows = 0;
    MurbEvolveCtl* herm_ctl = nullptr;        // murbhip_evolve's control block (device), allocated on first use
    MurbEvolveCtl* herm_ctl_host = nullptr;   // pinned copy of its head (everything in front of the ring)
    // individual block time steps (murbhip_evolve_block), allocated on first use (ensure_block)
    MurbBlockCtl* blk_ctl = nullptr;          // control block (device)
    MurbBlockCtl* blk_ctl_host = nullptr;     // pinned copy
    unsigned int* blk_ticks = nullptr;        // per body: its own time inside the block, in ticks
    int* blk_levels = nullptr;                // per body: its level
    int* blk_list = nullptr;                  // the active bodies of the step in flight
    float4* blk_rec = nullptr;                // their predicted positions and velocities by list index, pair layout
    float4* blk_vel = nullptr;
    float4* blk_part = nullptr;               // partial rows of the active sweep: blk_rows entries of accelerations, then of jerks
    size_t blk_rows = 0;
    // "nearest" (Hermite sweeps), allocated on first use (ensure_hermite)
    int* nn_idx = nullptr;                    // per slot: nearest other real body of the remembered evaluation, -1 = none
    float* nn_r2 = nullptr;                   // ... and the sweep's r2 of that pair
    MurbEncList* enc = nullptr;               // the encounter list of the last murbhip_evolve / murbhip_evolve_block
    // "potential" (Hermite sweeps), allocated on first use (ensure_hermite)
    float* herm_phi = nullptr;                // per slot: phi_i of the remembered evaluation (include/murbhip.h, "potential")
    double* pot_sums = nullptr;               // block sums of murbhip_potential_energy
    double* pot_sums_host = nullptr;          // ... and their pinned host copy
    // field read-out (murbfield_at / murbfield_of): buffers of its own, allocated on first use and grown (ensure_field); the
    // tidal read-out (murbtidal_at / murbtidal_of) uses the same ones: both are synchronous on the compute stream
    float* fld_in = nullptr;        // a launch's uploaded points: 6 planes of floats and one of ints (skip entries or bodies)
    float4* fld_pts = nullptr;      // ... packed: two records per point
    float* fld_out = nullptr;       // ... results: 7 planes
    size_t fld_points = 0;          // points the three hold
    float4* fld_part = nullptr;     // partial rows: fld_rows entries {ax, ay, az, phi}, then as many {jx, jy, jz, 0}
    size_t fld_rows = 0;
    // massless tracers (include/murbtracer.h): buffers of their own, allocated on first upload and grown (ensure_tracers).  The
    // steps that carry them are enqueue-only and the read-outs above synchronous, so the two share nothing
    float* trc_state = nullptr;     // 18 planes of trc_cap floats: q, v, (a0, j0), (a1, j1), three each
    float4* trc_pts = nullptr;      // the packed (predicted) records: two per tracer, whole groups
    size_t trc_cap = 0;             // tracers the two hold (a multiple of 16)
    float4* trc_part = nullptr;     // partial rows: trc_rows entries {ax, ay, az, 0}, then as many {jx, jy, jz, 0}
    size_t trc_rows = 0;
    // k nearest neighbours and densities (include/murbknn.h): the points go through the field read-out's fld_in / fld_pts (every
    // call of either is synchronous on the compute stream); the lists and rows are its own, allocated on first use and grown
    float* knn_part_r2 = nullptr;   // the chunks' lists: knn_part entries of r2 ...
    int* knn_part_idx = nullptr;    // ... and of indices
    size_t knn_part = 0;
    float* knn_list_r2 = nullptr;   // a launch's merged lists: knn_list entries each
    int* knn_list_idx = nullptr;
    size_t knn_list = 0;
    float* knn_rho = nullptr;       // densities: of a launch's points, or of all bodies (murbdensity_centre); knn_rhos floats
    size_t knn_rhos = 0;
    double* knn_sums = nullptr;     // block rows of murb_knn_centre_kernel: knn_blocks rows
    size_t knn_blocks = 0;
    // neighbours within a radius (include/murbnbr.h): the points go through the field read-out's fld_in / fld_pts like the knn
    // read-out's; counts, bases and the list buffer are its own, allocated on first use and grown
    unsigned int* nbr_part = nullptr;    // the chunks' counts, then their prefix sums per point: nbr_parts entries
    size_t nbr_parts = 0;
    unsigned int* nbr_counts = nullptr;  // a launch's counts per point: nbr_points entries ...
    unsigned int* nbr_base = nullptr;    // ... and a range's bases per point
    size_t nbr_points = 0;
    int* nbr_idx = nullptr;              // the list buffer ("list_entries"): nbr_list entries of indices ...
    float* nbr_r2 = nullptr;             // ... and of r2
    size_t nbr_list = 0;
    // bound pairs (include/murbbind.h): the packed points go through the field read-out's fld_pts like the knn read-out's; the
    // uploaded planes, rows and results are its own, allocated on first use and grown
    float* bnd_in = nullptr;        // a launch's uploaded points: 7 planes of floats and one of ints (skip entries or bodies)
    size_t bnd_ins = 0;             // floats it holds
    uint2* bnd_part = nullptr;      // the chunks' (key, index): bnd_parts entries
    size_t bnd_parts = 0;
    int* bnd_idx = nullptr;         // partners: of a launch's points, or of all bodies (murbbind_pairs); bnd_points entries ...
    float* bnd_h = nullptr;         // ... and their h
    size_t bnd_points = 0;
    double* bnd_elems = nullptr;    // murbbind_pairs: 6 doubles per body, bnd_elem doubles ...
    size_t bnd_elem = 0;
    int* bnd_flag = nullptr;        // ... which bodies hold a pair: bnd_flags entries ...
    size_t bnd_flags = 0;
    double* bnd_sums = nullptr;     // ... and the block rows of murb_bind_pairs_kernel: bnd_rows doubles
    size_t bnd_rows = 0;
    // potential read-out and bound members (include/murbbound.h): the packed points go through the field read-out's fld_pts like the
    // knn read-out's; the uploaded planes, the masked records, rows and results are its own, allocated on first use and grown
    float* pot_in = nullptr;        // a launch's uploaded points: 3 planes of floats and one of ints (skip entries or bodies)
    size_t pot_ins = 0;             // floats it holds
    float4* pot_rec = nullptr;      // the masked copy of the position + G m records: pot_recs records
    size_t pot_recs = 0;
    unsigned char* pot_member = nullptr;   // the mask, one byte per body: pot_members bytes
    size_t pot_members = 0;
    float* pot_part = nullptr;      // the chunks' rows: pot_parts floats
    size_t pot_parts = 0;
    float* pot_phi = nullptr;       // phi: of a launch's points, or of all bodies (murbbound_members); pot_phis floats
    size_t pot_phis = 0;
    double* pot_e = nullptr;        // murbbound_members: e per body, pot_es doubles ...
    size_t pot_es = 0;
    double* pot_rows = nullptr;     // ... and the block rows of its two kernels: pot_row doubles
    size_t pot_row = 0;
    // nearest body of another label and the spanning tree (include/murbmst.h): the packed points go through the field read-out's
    // fld_pts like the knn read-out's; the labels, the labelled records, the listed bodies, rows and results are its own,
    // allocated on first use and grown
    int* mst_label = nullptr;       // the labels, one int per body: mst_labels entries
    size_t mst_labels = 0;
    float4* mst_rec = nullptr;      // the labelled copy of the position + G m records: mst_recs records
    size_t mst_recs = 0;
    int* mst_in = nullptr;          // a launch's listed bodies: mst_ins entries
    size_t mst_ins = 0;
    uint2* mst_part = nullptr;      // the chunks' (r2 bits, index): mst_parts entries
    size_t mst_parts = 0;
    int* mst_idx = nullptr;         // a launch's partners: mst_points entries ...
    float* mst_r2 = nullptr;        // ... and their r2
    size_t mst_points = 0;
    // pair separations (include/murbsep.h): the packed points go through the field read-out's fld_pts like the knn read-out's; the
    // uploaded planes, the mask, the masked records, rows and results are its own, allocated on first use and grown
    float* sep_in = nullptr;        // a launch's uploaded points: 3 planes of floats and one of ints (the listed bodies)
    size_t sep_ins = 0;             // floats it holds
    unsigned char* sep_member = nullptr;   // the mask, one byte per body: sep_members bytes
    size_t sep_members = 0;
    float4* sep_rec = nullptr;      // the masked copy of the position records: sep_recs records
    size_t sep_recs = 0;
    float* sep_part = nullptr;      // the chunks' rows: sep_parts floats
    size_t sep_parts = 0;
    double* sep_sum = nullptr;      // a launch's sums: sep_sums doubles
    size_t sep_sums = 0;
    unsigned int* sep_rows = nullptr;        // the workgroups' counter rows of a launch: sep_row entries ...
    size_t sep_row = 0;
    unsigned long long* sep_total = nullptr; // ... and the call's 64-bit totals: sep_totals entries
    size_t sep_totals = 0;
    // the field of listed bodies (include/murblist.h): murblist_of / murblist_at pack their points through the field read-out's
    // fld_in / fld_pts and stage their entries in the neighbour read-out's list buffer (nbr_idx); murbsplit_of runs inside the
    // neighbour read-out's fill pass, whose points occupy fld_pts, so its points have records of their own.  All three write fld_out
    float4* lst_src = nullptr;      // the gather copy of the bodies, two records per body: lst_srcs records
    size_t lst_srcs = 0;
    unsigned int* lst_range = nullptr;   // a range's list starts, then its list lengths: lst_ranges entries
    size_t lst_ranges = 0;
    float4* lst_pts = nullptr;      // murbsplit_of: a range's packed points: lst_points records
    size_t lst_points = 0;
    // the Ahmad-Cohen scheme (include/murbac.h): everything it keeps between steps and everything its steps write is its own, so
    // that the read-outs above (synchronous, on buffers of theirs) stay observers; of the Hermite integrator it uses the predicted
    // records, the partial rows and the remembered (a0, j0)
    float4* ac_src = nullptr;       // the predicted bodies in gather form, two records per body: ac_srcs records
    size_t ac_srcs = 0;
    float* ac_in = nullptr;         // the rebuild's points as murb_nbr_pack_kernel reads them: n thresholds, then the n bodies: ac_ins floats
    size_t ac_ins = 0;
    float4* ac_pts = nullptr;       // ... packed, whole groups: ac_ptss records
    size_t ac_ptss = 0;
    unsigned int* ac_part = nullptr;   // the chunks' counts, then their prefix sums per point: ac_parts entries
    size_t ac_parts = 0;
    unsigned int* ac_begin[2] = {nullptr, nullptr};   // the two list buffers alternate (old and new lists exist together): per body
    unsigned int* ac_len[2] = {nullptr, nullptr};     // where its list starts and its length: ac_points entries each ...
    size_t ac_points[2] = {0, 0};
    int* ac_idx[2] = {nullptr, nullptr};              // ... and the entries: ac_cap entries
    size_t ac_cap[2] = {0, 0};
    float* ac_r2 = nullptr;         // the fill sweep's r2, written and never read: ac_r2s floats
    size_t ac_r2s = 0;
    float* ac_out = nullptr;        // two list sweeps' results, seven planes of n each: ac_outs floats
    size_t ac_outs = 0;
    float* ac_force = nullptr;      // (aI, jI): 6 planes of n, then (aR, jR, a2R, a3R): 12 planes: ac_forces floats
    size_t ac_forces = 0;
    unsigned long sym_launches = 0; // pair-symmetric launches of any form since "profile" was last set (force, potential sweep)
    size_t bytes = 0;
};

// Device buffers of a shard, allocated on first use and counted in Shard::bytes (info "device_bytes").  `zero_on`: a fresh
// buffer is also cleared, on that stream.
template <typename T>
int shard_alloc(Shard& sh, T*& p, size_t bytes, hipStream_t zero_on = nullptr)
{
    if (p) return 0;
    HIP_TRY(hipMalloc((void**)&p, bytes));
    sh.bytes += bytes;
    if (zero_on) HIP_TRY(hipMemsetAsync(p, 0, bytes, zero_on));
    return 0;
}
template <typename T>
void shard_free(Shard& sh, T*& p, size_t bytes)
{
    if (!p) return;
    release(p);
    p = nullptr;
    sh.bytes -= bytes;
}

constexpr int kPeSumBlocks = 256;      // workgroups of murb_sym_pe_sum_kernel
constexpr size_t kProfPairs = 4096;

// What a pair of timing events brackets.  "profile" 1: the force launches only (two event records per launch);
// 2: also the collectives on the exchange stream, the compute stream's waits for them (= the EXPOSED part of the
// exchange) and the compute stream's whole step.
enum ProfKind {
    kProfForce = 0,       // a force launch outside the exchange pipeline (one GPU; the one-sided kernels)
    kProfTri1,            // exchange pipeline: first part of the own-slice triangle (runs under the position gather)
    kProfRect,            // ... rectangles against the other slices
    kProfTri2,            // ... rest of the own-slice triangle (runs under the reduce-scatter)
    kProfReduceScatter,   // exchange stream: from "my send chunks are ready" to "my reduced share has arrived"
    kProfAllGather,       // exchange stream: from "my slice is integrated" to "all slices have arrived"
    kProfWaitGather,      // compute stream: idle in front of the rectangles, waiting for the gathered positions
    kProfWaitReduce,      // compute stream: idle in front of the state update, waiting for the reduced share
    kProfStep,            // compute stream: first launch of a step to the end of its state update
    kProfField,           // compute stream: a sweep launch of the field read-out (murbfield.h); never part of the force figures
    kProfTidal,           // compute stream: a sweep launch of the tidal read-out (murbtidal.h); never part of the force figures
    kProfTracer,          // compute stream: a sweep launch of the tracers (murbtracer.h); never part of the force figures
    kProfKnn,             // compute stream: a sweep launch of the neighbour read-out (murbknn.h); never part of the force figures
    kProfNbr,             // compute stream: a count or fill sweep launch of the radius read-out (murbnbr.h); never part of the force figures
    kProfBind,            // compute stream: a sweep launch of the bound-pair read-out (murbbind.h); never part of the force figures
    kProfPot,             // compute stream: a sweep launch of the potential read-out (murbbound.h); never part of the force figures
    kProfMst,             // compute stream: a sweep launch of the foreign-nearest read-out (murbmst.h); never part of the force figures
    kProfSep,             // compute stream: a sweep launch of the pair-separation read-out (murbsep.h); never part of the force figures
    kProfList,            // compute stream: a sweep launch of the listed-source read-out (murblist.h); never part of the force figures
    kProfAcPredict,       // compute stream: the predictor launch of an irregular step of the Ahmad-Cohen scheme (murbac.h)
    kProfAcCorrect,       // compute stream: the corrector launch of an irregular step, or the last launch of a regular one (murbac.h)
    kProfKinds
};

}  // namespace

struct murbhip_ctx {
    PlanInputs in;             // n, world, slice, slots, the device facts and every option the plan choice reads (murb_choose.h)
    float soft2 = 0.f, g = 0.f;
    int exchange = 0;          // 0 peer copies, 1 RCCL
    bool rank_mode = false;    // one shard here, the others live in other processes
    std::vector<Shard> shards;
    ShardCrew* crew = nullptr; // one host thread per shard when this process drives several
    int cur = 0;               // record buffer holding the current positions
    bool uploaded = false;
    bool gather_pending = false;   // an exchange into rec[cur] is in flight on the comm streams
    bool reduce_pending = false;   // peers may still be reading this context's reduce-scatter send buffers
    // options
    int profile = 0, overlap = 1;
    int tri_first_pct = 50;   // overlap 1: share of the own-slice triangle launched BEFORE the rectangles (under the
                              // position gather); the rest runs under the reduce-scatter
    int xcd_order = 0;        // pair-symmetric kernel: 1 = item table interleaved into one run per XCD (measured worse)
    int evolve_batch = 0;     // murbhip_evolve: steps per batch; 0 = from the remaining time over the step last seen
    int integrator = 0;       // 0 the reference's update (Bodies.cpp:260-278), 1 kick-drift-kick leapfrog, 2 4th-order Hermite
    bool herm_current = false;// Hermite: herm_a0 / herm_j0 hold the evaluation the next step starts from
    bool herm_in_acc_out = false;   // ... and acc_out still holds its accelerations (no force evaluation has run since)
    bool herm_proposal = false;     // ... and the control block's `raw` is the step murbhip_evolve's criterion proposes from it
    unsigned long evolve_steps = 0; // steps of the last murbhip_evolve (what murbhip_evolve_dts reads from the ring)
    // individual block time steps (murbhip_evolve_block)
    int block_units = 0;            // "block_units": (group, chunk) units the active sweep is cut into at least; 0 = default
    bool blk_open = false;          // a call ended inside a block (max_steps): bodies sit at their own times
    int blk_have_levels = 0;        // 1: the device's levels were left by a call that ended synchronised, for (blk_dt_max, blk_kmax);
                                    // 2: murbhip_block_set_levels put them there, for blk_kmax
    float blk_dt_max = 0.f;
    int blk_kmax = 0;
    double blk_steps_per_block = 0; // block steps a block took in the last call (sizes the first batch of the next)
    double blk_info[4] = {0, 0, 0, 0};   // last call: block steps, body-steps, clamped steps, largest active set
    // nearest neighbours and the encounter stop (Hermite sweeps)
    int nearest = 0;                // "nearest": the sweeps keep every body's nearest neighbour beside (a, j)
    float enc_radius = 0.f;         // murbhip_set_encounter; 0 = off
    unsigned long enc_count = 0;    // hits of the step that ended the last evolve call (0: it ended otherwise)
    double enc_time = 0.0;          // ... and the model time advanced in that call when they were seen
    // contact by radii (Hermite sweeps); shares the per-slot arrays, the hit list and the counters above with "nearest"
    int contact = 0;                // "contact": 1 the sweeps keep every body's (cp, gap2) beside (a, j), 2 also the contact stop
    int potential = 0;              // "potential": the sweeps keep every body's phi_i beside (a, j); excludes "nearest" and "contact"
    long field_chunks = 0;          // "field_chunks": j chunks of the field read-out; 0 = default (murb_field.h)
    long field_batch = 0;           // "field_batch": its points per launch; 0 = default
    long nbr_list_entries = 0;      // "list_entries" (murbnbr.h): the device list buffer's entries; 0 = default (murb_nbr.h)
    // massless tracers (include/murbtracer.h)
    unsigned long tracers = 0;      // resident tracers; 0 = none, and then nothing of the context differs from a build without them
    bool trc_current = false;       // their (a0, j0) are those of the tracers' and the bodies' current state
    long tracer_chunks = 0;         // "tracer_chunks", "tracer_batch": the field options' meaning (murb_field.h)
    long tracer_batch = 0;
    // the Ahmad-Cohen scheme (include/murbac.h)
    bool ac_live = false;           // murbac_begin has run and nothing has changed the bodies another way since
    int ac_nirr = 0, ac_m = 0;      // regular steps are every ac_nirr-th; ac_m steps since the last one
    int ac_buf = 0;                 // which of the two list buffers holds the resident lists
    unsigned long ac_steps = 0, ac_regular = 0;
    double ac_time = 0.0;           // the fp64 sum of the steps' dt since murbac_begin
    std::vector<unsigned long> ac_offsets;   // the resident lists' offsets: n + 1 entries
    unsigned long ac_longest = 0, ac_empty = 0;
    int tracer_dt = 0;              // "tracer_dt": 1 = the tracers' Aarseth steps enter murbhip_evolve's step-size minimum
    bool lf_half = false;     // leapfrog: device velocities lag the positions by half a step of lf_last_dt
    // acceleration cache: murbhip_compute_acc / a leapfrog read-out evaluated the forces at the CURRENT positions
    bool acc_current = false;        // acc_out holds them (a second evaluation would be bit-identical: skip it)
    unsigned long state_serial = 1;  // counts the changes of the body state (upload, device initialisation, every update)
    unsigned long metrics_serial = 0;// the state the cached metric sums below belong to (murbhip_energy and murbhip_moments of one
    bool metrics_with_phi = false;   // tracked iteration share one pass of the metrics kernel and one read-back)
    double metrics_sums[MURB_METRIC_VALUES] = {0};
    bool want_pe = false;            // the force launches being enqueued also sum the pair potential (murbhip_energy)
    bool pe_current = false;         // ... and the partial-row buffers hold it for the current positions
    float lf_last_dt = 0.f;
    int force_exchange = 0;   // run the exchange even with one rank (self-test of the RCCL binding)
    int init_libm_fma = -1;   // murbhip_init_bodies: which build of glibc's sincosf to reproduce (-1 = what this host's libm picks)
    int sym_wide = -1;        // pair-symmetric kernel: the range-safe pair factor (G m inv) inv^2; -1 = where the last upload needs it
    bool sym_wide_needed = false;   // ... what murbhip_upload found (csrc/murb_choose.h, sym_wide_needed); device-made bodies: false
    int energy_sweep = 0;     // murbhip_energy on a pair-symmetric plan: 1 = the separate potential sweep of rounds 1-2 (kept for the A/B)
    int exchange_p2p = 0;     // RCCL exchange by grouped ncclSend/ncclRecv instead of ncclReduceScatter / ncclAllGather
    int pad_aware = 1;        // pair-symmetric kernel: 1: padding slots are not walked (murb_schedule.h, sym_orient); 0: every block as if full (A/B)
    int cu_reserve = 0;       // CUs masked out of the compute streams (left free for the collectives' kernels)
    int solo_shard = -1;      // >= 0: only this shard computes (timing aid: one rank's isolated timeline
                              // when W shards share one GPU; results are then meaningless)
    // facts
    int clock_mhz = 0;
    double interactions_per_launch = 0;
    int async_error = 0;
};

#endif
