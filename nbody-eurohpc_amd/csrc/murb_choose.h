// Which kernel runs at every N and rank count: the force plan (make_plan) and the rules behind it, as pure functions of
// PlanInputs — no HIP in here and no context.  murbhip.hip keeps one PlanInputs inside its context ("set_option" writes
// the options into it) and calls make_plan per step; tests/helpers/plan_selftest.cpp sweeps the same functions on the CPU,
// under AddressSanitizer / UBSan, and pushes every pair-symmetric choice through the layout checks.
#ifndef MURB_CHOOSE_H_
#define MURB_CHOOSE_H_

#include <algorithm>
#include <cstddef>

#include "murb_layout.h"
#include "murb_plan.h"

namespace {

// Everything the plan choice reads.
struct PlanInputs {
    // facts
    unsigned long n = 0;
    int world = 1;
    unsigned long slice = 0;   // slots per rank
    unsigned long slots = 0;   // world * slice
    int cu_count = 0;
    size_t device_mem = 0;     // bytes of HBM on the first device
    int resident_per_cu = 0;   // workgroups of the persistent kernel resident on a CU (an occupancy query: murbhip.hip fills it
                               // in the first time a persistent plan is asked for; 0 = not asked yet)
    // options
    int variant = 0, jsplit = 0;
    int sym_waves = 0;        // pair-symmetric kernel: waves per workgroup, 0 = auto, 4 or 8
    int taper = -1;           // ... % of each launch cut into finer items (-1 = the plan's default)
    int diag_tri = -1;        // ... diagonal blocks as triangular pieces (-1 = the plan's default)
    int sym_red = -1;         // ... i-side reduction in registers (0) or through LDS (1) (-1 = the plan's default)
    int fuse_integrate = 1;   // "fuse_integrate": one-sided plan, the state update in the tail of the step's last force launch
    long sym_pass_mb = 0;     // ... one GPU: budget (MiB) for the partial rows of one pass; 0 = a quarter of the device memory
    int tri_div = 0;          // ... exchange pipeline: the own-slice triangle's items cut into this many parts more (0 = the plan's choice)
};

constexpr int kMaxParts = 64;          // rows of the partial-sum buffer
constexpr int kNumVariants = 8;
constexpr int kOneSidedVariant = 1;     // the persistent schedule (7) measured no faster: DESIGN.md §4.1
constexpr int kOneSidedFewBodies = 2;   // 4 i bodies per wave instead of 8: twice the workgroups for a rank's small slice (tools/solo_rank.py,
                                        // round 3, one rank alone: N = 30 000 W = 2/4/8 148 -> 138, 92 -> 86, 69 -> 63 us per step; N = 16 000
                                        // W = 4: 54 -> 43; N = 45 000 W = 8: 108 -> 99; equal from ~20 000 bodies per rank)
constexpr int kPersistentVariant = 7;   // murb_force_persistent<8, 4, 4>
constexpr int kSymmetricVariant = 8;    // murb_force_sym_kernel<4, 4 or 8>
constexpr unsigned long kSymmetricMinBodies = 2049;    // below this (one or two blocks) the one-sided kernel wins; round 2: 10 240 —
                                                       // with items of 64-128 bodies the pair-symmetric kernel is 1.2-1.4x faster
                                                       // from 3 blocks up (tools/small_plan_table.py: N = 3584 14.4 vs 20.5 us per step)
constexpr int kRowsPerLaunch = kMaxParts / 2;

struct Plan {
    int variant;   // resolved
    int parts_local, parts_remote;   // 2-D grid variants: j chunks of the own-slice launch and of the rest
    bool persistent;                 // balanced persistent schedule (murb_force_persistent)
    bool symmetric;                  // pair-symmetric kernel (murb_force_sym_kernel)
    int split;                       // its i-side sub-blocks per block (1, 2, 4, 8, 16)
    int waves;                       // ... and its waves per workgroup (4 or 8)
    int taper;                       // ... and the share (%) of each launch whose items are cut finer ("taper")
    bool diag_tri;                   // ... diagonal blocks in triangular pieces ("diag_tri")
    int red;                         // ... i-side reduction: 0 registers, 1 LDS teams ("sym_red")
    MurbSchedule sched[2];           // [0] own slice (or everything), [1] the rest
};

// "sym_wide": which form of its pair factor the pair-symmetric kernel takes (csrc/murb_kernels_sym.h, murb_interact_sym).  The
// fast form cubes 1 / sqrt(r^2 + soft^2) before G m comes in: the cube is a normal fp32 number for 2^-42 <= r <= 2^42.
// `reach` bounds the largest r of the uploaded bodies (the diagonal of their bounding box and the softening, added in
// quadrature); the fast form is kept where the system may still grow 2^8-fold, and where the softening — the smallest r, a
// body against itself — leaves the cube two binades and more below the largest fp32 number.  Anything that is not a number
// takes the wide form.
constexpr double kSymFastMaxReach = 0x1p34;
constexpr double kSymFastMinSoft = 0x1p-40;
inline bool sym_wide_needed(double reach, double soft) { return !(reach <= kSymFastMaxReach && soft >= kSymFastMinSoft); }
inline bool sym_wide_chosen(int option, bool needed) { return option < 0 ? needed : option != 0; }   // -1 automatic, 0 / 1 forced

// Workgroups of the persistent kernel that fit on the chip at once.
inline int resident_blocks(const PlanInputs& in) { return std::max(in.resident_per_cu, 1) * std::max(in.cu_count, 1); }

// Cut groups x tiles units into equal runs: `rounds` runs per resident slot (so that a slot lost to
// another process or to the profiler costs 1/rounds, not 2x), at least ~8 tiles per run (the
// end-of-run reduction is ~1 % of that), and few enough runs that a group spans < kRowsPerLaunch rows.
inline MurbSchedule make_schedule(const PlanInputs& in, long groups, long tiles, int row_base)
{
    MurbSchedule sc{(int)groups, (int)tiles, 1, row_base};
    const long units = groups * tiles;
    if (units <= 0) { sc.nblocks = 0; return sc; }
    const long slots = resident_blocks(in);
    long rounds = in.jsplit > 0 ? in.jsplit : std::min<long>(8, std::max<long>(1, units / (slots * 8)));
    long nb = std::min(units, slots * rounds);
    nb = std::min(nb, std::max<long>(1, (kRowsPerLaunch - 2) * groups));
    sc.nblocks = (int)std::max<long>(nb, 1);
    return sc;
}

inline int variant_group(int variant)   // bodies per workgroup = waves * R
{
    switch (variant) {
        case kPersistentVariant: return 32;
        case kSymmetricVariant: return 32;
        case 2: case 6: return 16;
        case 5: return 64;
        default: return 32;
    }
}

// How many j chunks: enough workgroups for ~24 scheduling rounds of the chip, but chunks of at
// least 8 tiles (4096 bodies) so the end-of-sweep reduction stays well under 1 % of the sweep.
inline int auto_parts(const PlanInputs& in, int variant, unsigned long i_slots, unsigned long tiles)
{
    if (tiles == 0) return 0;
    const unsigned long groups = (i_slots + variant_group(variant) - 1) / variant_group(variant);
    const unsigned long want_blocks = (unsigned long)std::max(in.cu_count, 1) * 6ul * 24ul;
    unsigned long parts = (want_blocks + groups - 1) / groups;
    parts = std::min(parts, std::max(tiles / 8ul, 1ul));
    parts = std::max(parts, 1ul);
    return (int)std::min<unsigned long>(parts, kMaxParts / 2);
}

// Block pairs a rank evaluates under the (half-ring) pair-symmetric schedule with whole-block items.
inline long sym_items_per_rank(const PlanInputs& in)
{
    const long tb = (long)(in.slice / MURB_SYM_BLOCK), w = in.world;
    return tb * (tb + 1) / 2 + ((w - 1) / 2) * tb * tb + (w > 1 && w % 2 == 0 ? tb * ((tb + 1) / 2) : 0);
}

// One GPU: what the partial rows of one pass may take.  Problems whose rows exceed it are evaluated in several passes
// over ranges of j columns (the rows of N = 1M take 12 GB, of 3.5M 144 GB: half of the HBM).
inline size_t sym_pass_budget(const PlanInputs& in)
{
    if (in.sym_pass_mb > 0) return (size_t)in.sym_pass_mb << 20;
    return in.device_mem ? in.device_mem / 4 : 0;
}

// Bytes of the partial rows of the pair-symmetric kernel on one rank for uniform items of 1024/split bodies
// (12 B per row slot: three components).  One GPU: block b has split*b j rows and T-b i rows.  A rank of W: its
// triangle (tb blocks) plus the rectangles against floor(W/2) slices: tb i rows per own block and split*tb j rows per
// far block at most.
inline size_t sym_row_bytes(const PlanInputs& in, int split)
{
    const size_t tb = in.slice / MURB_SYM_BLOCK, w = (size_t)in.world, far = w / 2;
    size_t rows = tb * tb + (size_t)(split - 1) * tb * (tb - 1) / 2;
    if (w > 1) rows += tb * far * tb + far * tb * (size_t)split * tb;
    return rows * MURB_SYM_BLOCK * 3 * sizeof(float);
}

// One GPU, few bodies: the one-sided kernel with the state update in its tail (murb_force_integrate_kernel: ONE launch per
// step, 2 i bodies per wave) against the pair-symmetric plan's two launches (force, row sum + update), by block count —
// tools/rate_curve.py, us per step, round 3: N = 2 049: 8.9 vs 14.0; 3 000: 9.4 vs 13.9; 3 584: 11.2 vs 14.4; 4 097 (5 blocks):
// 14.2 vs 14.9, 5 000: 15.0 vs 15.1 (a tie: the pair-symmetric plan stays); 6 000 (6 blocks, where the pair-symmetric items
// fall badly on the workgroup slots): 16.2 vs 19.8; 7 000: 21.9 vs 20.2; 8 193: 37 vs 27.
inline bool fused_one_sided_wins(const PlanInputs& in)
{
    const unsigned long T = in.slots / MURB_SYM_BLOCK;
    return in.fuse_integrate && in.jsplit == 0 && (T <= 4 || T == 6);
}

inline Plan make_plan(const PlanInputs& in)
{
    Plan p{};
    // variant 0 = auto: pair-symmetric when a GPU gets enough block pairs and its partial rows fit comfortably
    // (they grow as N^2/1024 on one GPU: 0.5 GB at 200k, 12 GB at 1M; a rank of W holds ~1/W of that), else one-sided
    // (one GPU: rows beyond the budget are handled in passes, so only a rank of several has to fit them whole)
    const auto fits = [&](int split) { return in.world == 1 || in.device_mem == 0 || sym_row_bytes(in, split) < in.device_mem / 2; };
    if (in.variant >= 1 && in.variant <= kNumVariants) p.variant = in.variant;
    else if (in.world == 1) p.variant = (in.n >= kSymmetricMinBodies && !fused_one_sided_wins(in) && fits(1)) ? kSymmetricVariant : kOneSidedVariant;
    else p.variant = (sym_items_per_rank(in) >= 400 && fits(1)) ? kSymmetricVariant : (in.slice <= 16384 ? kOneSidedFewBodies : kOneSidedVariant);
    p.symmetric = p.variant == kSymmetricVariant;
    if (p.symmetric) {
        // finer items (i side cut in 2 or 4) until a GPU has ~8 scheduling rounds of them; ~16 in the
        // multi-rank pipeline, whose three force launches per step each end in a tail (measured with
        // tools/solo_profile.py: N=200k, W=2/4/8 -> split 2/4/4 is best)
        const long items = sym_items_per_rank(in);
        const long want = (in.world > 1 ? 16L : 8L) * 4 * std::max(in.cu_count, 1);
        // ... and with few block pairs per rank finer still, so that each of the three launches of a step gets its round of
        // workgroups (tools/solo_rank.py, round 3: N=100k W=8, 689 block pairs: split 8 beats 4 by 3 %; N=60k W=4, 465: by 4.6 %;
        // N=30k W=2, 240: split 16 beats 4 by 5.5 %; from ~1000 block pairs up 4 is best: N=100k W=4, N=200k W=8)
        p.split = (in.jsplit == 1 || in.jsplit == 2 || in.jsplit == 4 || in.jsplit == 8 || in.jsplit == 16)
                      ? in.jsplit
                      : (items >= want ? 1 : (2 * items >= want ? 2 : (in.world == 1 || items >= 1000 ? 4 : (items >= 400 ? 8 : 16))));
        // Rounds 1-2, one GPU below 45 000 bodies (BASELINE's N = 30 000: 465 block pairs for 1024 workgroup slots): 8-wave
        // workgroups (2 per SIMD, 2 workgroups per CU: a CU's last workgroup still has two waves per SIMD to interleave),
        // quarter-block items with the last 30 % of the launch cut finer, diagonal blocks as triangular pieces.
        // tools/ab.py, interleaved, N = 30 000, wall per step: 8 waves / split 8 (round 1) 174.5 us, 8 / 4 / taper 30 /
        // triangular diagonal 170.5, 8 / 2 / taper 60 171.4; 4 waves never better.
        // Round 3 (tools/small_plan_table.py: five plans interleaved for every block count T = 10 ... 44; padding-aware
        // items, measurement without the profiling events): from T = 28 blocks up (N > 27 648) the plan of the larger
        // problems — 4 waves, quarter blocks, 5 % taper, plain diagonal — is the fastest or within 1 % of it (N = 30 000:
        // +3.6 % over the 8-wave plan, interleaved).  Below, the winner follows how the item count falls on the 1024
        // (4 waves) or 512 (8 waves) workgroup slots of the chip, block count by block count, with up to 27 % between the
        // plans at T = 10-16: a table (measured on the 256 CUs of an MI355X; any other CU count keeps the 8-wave plan).
        struct SmallPlan { int waves, split, taper; bool diag_tri; };
        static const SmallPlan kSmallPlans[5] = {{8, 4, 30, true}, {4, 4, 5, false}, {4, 8, 5, false}, {8, 8, 30, true}, {4, 16, 5, false}};
        static const signed char kSmallPlanOfBlocks[25] = {4, 4, 4, 3, 3, 3, 4,                                      // T = 3 ... 9
                                                           3, 3, 0, 2, 2, 1, 3, 0, 2, 1, 2, 0, 1, 2, 0, 1, 0, 2};   // T = 10 ... 27
        const int T = (int)(in.slots / MURB_SYM_BLOCK);
        const bool small = in.world == 1 && T <= 27;
        const SmallPlan sp = kSmallPlans[(small && in.cu_count == 256 && T >= 3) ? kSmallPlanOfBlocks[T - 3] : (T < 10 ? 3 : 0)];
        p.waves = (in.sym_waves == 4 || in.sym_waves == 8) ? in.sym_waves : (small ? sp.waves : 4);
        if (in.jsplit == 0 && in.sym_waves == 0 && small) p.split = sp.split;
        while (p.split > 1 && MURB_SYM_BLOCK / p.split < 16 * p.waves) p.split /= 2;   // an item is at least one group per wave
        while (p.split > 1 && !fits(p.split)) p.split /= 2;   // the rows of the split actually used must fit, too
        // the tail of a launch in finer items (murb_schedule.h): +1.2-1.4 % on the force launch at N = 200 000 with 5 %,
        // nothing at 1M (the tail is 0.3 % of the launch there), and nothing on the wall clock of a rank of 8, whose three
        // short launches gain what their row sums lose to the extra rows
        p.taper = in.taper >= 0 ? in.taper : (in.world > 1 ? 0 : (small ? sp.taper : (in.n <= 600000 ? 5 : 0)));
        p.diag_tri = in.diag_tri >= 0 ? in.diag_tri != 0 : (small && sp.diag_tri);
        // i-side sums through LDS: 599 instead of 616 VALU instructions per group; +0.8-1.3 % at N = 200 000, +1.7 % for
        // a rank of 8 (tools/ab.py)
        p.red = in.sym_red >= 0 ? in.sym_red : 1;
        p.persistent = false;
        p.parts_local = p.parts_remote = 0;
        return p;
    }
    const unsigned long tiles_local = in.slice / MURB_TILE_BODIES;
    const unsigned long tiles_remote = (in.slots - in.slice) / MURB_TILE_BODIES;
    p.persistent = p.variant == kPersistentVariant;
    if (p.persistent) {
        // every shard sweeps the same number of i groups: the largest slice count decides
        unsigned long first, count;
        partition(in.n, in.world, 0, &first, &count);
        const long groups = (long)((count + 31) / 32);
        p.sched[0] = make_schedule(in, groups, (long)tiles_local, 0);
        p.sched[1] = make_schedule(in, groups, (long)tiles_remote, kRowsPerLaunch);
        p.parts_local = p.parts_remote = 0;
        return p;
    }
    if (in.world == 1) {
        p.parts_local = in.jsplit > 0 ? std::min<int>(in.jsplit, (int)std::min<unsigned long>(tiles_local, kMaxParts))
                                      : auto_parts(in, p.variant, in.slice, tiles_local);
        // up to 6 blocks the default one-sided launch keeps all j in one chunk: its workgroups then need nothing from each
        // other and take the state update along (murb_force_integrate_kernel)
        if (in.jsplit == 0 && in.fuse_integrate && p.variant == kOneSidedVariant && in.slots / MURB_SYM_BLOCK <= 6) p.parts_local = 1;
        p.parts_remote = 0;
    } else {
        // split the requested/auto chunk count between the two launches in proportion to their tiles
        const unsigned long tiles_all = tiles_local + tiles_remote;
        int total = in.jsplit > 0 ? in.jsplit : auto_parts(in, p.variant, in.slice, tiles_all);
        total = std::max(total, 2);
        int loc = (int)std::max<unsigned long>(1ul, (unsigned long)total * tiles_local / tiles_all);
        int rem = std::max(1, total - loc);
        p.parts_local = (int)std::min<unsigned long>((unsigned long)loc, std::min<unsigned long>(tiles_local, kMaxParts / 2));
        p.parts_remote = (int)std::min<unsigned long>((unsigned long)rem, std::min<unsigned long>(tiles_remote, kMaxParts / 2));
    }
    return p;
}

// Exchange pipeline: the own-slice triangle is T_s (T_s + 1) / 2 block pairs in TWO launches (one under each collective); with
// few blocks per slice neither fills the chip's 4 x CUs workgroup slots and both run at a fraction of the issue rate.
// Their items (and only theirs) are cut finer until each launch has ~2 rounds of them ("tri_div" overrides).
inline int plan_tri_div(const PlanInputs& in, const Plan& p)
{
    if (in.tri_div > 0) return in.tri_div;
    if (in.world == 1) return 1;
    const long tb = (long)(in.slice / MURB_SYM_BLOCK);
    const long items = tb * (tb + 1) / 2 * p.split / 2;             // per triangle launch
    const long slots = 4L * std::max(in.cu_count, 1) * 4 / p.waves;  // resident workgroups
    int div = 1;
    while (div < 4 && items * div < 2 * slots && MURB_SYM_BLOCK / (p.split * div * 2) >= 16 * p.waves) div *= 2;
    return div;
}

// The key of the pair-symmetric tables a shard needs for plan `p` (murb_plan.h).  `overlap` and `tri_first_pct` only place launch
// boundaries inside the exchange pipeline's triangle: outside that mode the layout ignores them, and so does the key.
inline SymLayoutKey sym_layout_key(const PlanInputs& in, const Plan& p, bool exchange_mode, int overlap, int tri_first_pct, bool xcd_order,
                                   bool pad_aware)
{
    SymLayoutKey k;
    k.split = p.split; k.waves = p.waves; k.taper = p.taper; k.diag_tri = p.diag_tri;
    k.exchange_mode = exchange_mode;
    k.overlap = exchange_mode ? overlap : 0;
    k.tri_first_pct = exchange_mode ? tri_first_pct : 0;
    k.xcd_order = xcd_order;
    k.budget_floats = sym_pass_budget(in) / (3 * sizeof(float));
    k.tri_div = plan_tri_div(in, p);
    k.pad_aware = pad_aware;
    return k;
}

// j chunks of the sweep: the one-sided kernels' rule ("jsplit" overrides), for i groups of 16 bodies
inline int hermite_parts(const PlanInputs& in)
{
    const unsigned long tiles = in.slots / MURB_TILE_BODIES;
    if (in.jsplit > 0) return (int)std::min<unsigned long>((unsigned long)in.jsplit, std::min<unsigned long>(tiles, kMaxParts / 2));
    return auto_parts(in, kOneSidedFewBodies, in.slots, tiles);
}

}  // namespace

#endif
