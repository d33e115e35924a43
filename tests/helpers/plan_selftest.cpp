// TEST INFRASTRUCTURE: the host-side planner of the pair-symmetric launches (csrc/murb_plan.h + murb_schedule.h, no HIP in
// them) compiled with g++ under AddressSanitizer and UBSan and swept over many (n, ranks, split, waves, taper, ...) plans:
// every item's two outputs lie inside the buffer the plan asks for, no partial-row cell has two writers, the row tables cover
// exactly the rows the items write, the passes partition the items — and the sanitizers see every index the planner computes.
// The plan choice (csrc/murb_choose.h: make_plan and its rules) runs in the same binary: the fused one-launch step, the small-plan
// table, the multi-rank thresholds and the forced options give the plans the comments there promise, and every pair-symmetric
// choice is chained through sym_layout_key into the same layout checks.
// The sweep has two parts: seven sizes from 1 to 60 001 bodies on 1-8 ranks, and 26 residues of a ragged last block (1 ... 1023
// real bodies, both sides of every length it can be cut to) at 1 + rem and 3 + rem blocks on one rank and two blocks a slice on
// 2-4 ranks (check_ragged_residues: 87 048 layouts).  About 93 000 layouts in all; under the sanitizers the run takes about
// 30 s on one core, 14 s before the residues came (all 1024 residues would take a quarter of an hour and more: do not).
//   plan_selftest        prints "ok <plans checked>" and exits 0
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <set>
#include <vector>

#include "murb_choose.h"

#define FAIL(...) do { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } while (0)
#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "n=%lu W=%d r=%d split=%d waves=%d taper=%d tri=%d ex=%d div=%d xcd=%d budget=%zu: ", n, W, r, key.split, key.waves, key.taper, (int)key.diag_tri, (int)key.exchange_mode, key.tri_div, (int)key.xcd_order, key.budget_floats); \
    FAIL(__VA_ARGS__); } } while (0)

// one bit per cell of a partial-row buffer (the rows of N = 1 000 000 on one GPU are 2.4e9 cells), handled a word at a time
struct Cells {
    std::vector<unsigned long long> w;
    explicit Cells(size_t n) : w((n + 63) / 64, 0ull) {}
    // false if a cell of [first, first + len) was set already (claim) / is not set (covers); claim sets them all
    template <bool CLAIM> bool walk(size_t first, size_t len)
    {
        bool ok = true;
        for (size_t k = first, end = first + len; k < end;) {
            const size_t bit = k % 64, n = std::min<size_t>(64 - bit, end - k);
            const unsigned long long mask = (n == 64 ? ~0ull : ((1ull << n) - 1)) << bit;
            unsigned long long& word = w[k / 64];
            if (CLAIM) { ok = ok && !(word & mask); word |= mask; }
            else ok = ok && (word & mask) == mask;
            k += n;
        }
        return ok;
    }
    bool claim(size_t first, size_t len) { return walk<true>(first, len); }
    bool covers(size_t first, size_t len) { return walk<false>(first, len); }
};

static int check_set(const std::vector<MurbSymItem>& items, size_t first, size_t end, const std::vector<MurbSymBlockRows>& table, size_t floats,
                     int waves, const char** what)
{
    Cells writers(floats), in_table(floats);
    for (const MurbSymBlockRows& br : table) {
        if (br.base_j + (size_t)br.nj * MURB_SYM_BLOCK > floats || br.base_i + (size_t)br.ni * MURB_SYM_BLOCK > floats) { *what = "row table outside the buffer"; return 1; }
        if (!in_table.claim(br.base_j, (size_t)br.nj * MURB_SYM_BLOCK) || !in_table.claim(br.base_i, (size_t)br.ni * MURB_SYM_BLOCK)) { *what = "two table entries share a row"; return 1; }
    }
    for (size_t k = first; k < end; ++k) {
        const MurbSymItem& it = items[k];
        const size_t len = (size_t)it.ngroups * waves * MURB_SYM_R;
        if (it.ngroups < 1 || it.i_slot0 % (waves * MURB_SYM_R) != 0 || it.i_slot0 / MURB_SYM_BLOCK != (int)((it.i_slot0 + len - 1) / MURB_SYM_BLOCK)) { *what = "i range leaves its block"; return 1; }
        if (it.ioff + len > floats) { *what = "i-side output outside the buffer"; return 1; }
        if (!writers.claim(it.ioff, len)) { *what = "two writers for an i-row cell"; return 1; }
        if (!in_table.covers(it.ioff, len)) { *what = "an item writes outside the row tables"; return 1; }
        if (!(it.flags & 1)) {
            if (it.joff + MURB_SYM_BLOCK > floats) { *what = "j-side output outside the buffer"; return 1; }
            if (!writers.claim(it.joff, MURB_SYM_BLOCK)) { *what = "two writers for a j-row cell"; return 1; }
            if (!in_table.covers(it.joff, MURB_SYM_BLOCK)) { *what = "an item writes outside the row tables"; return 1; }
        }
    }
    return 0;
}

// The layout of rank r for `key`: item counts, every set (or pass) through check_set, the passes a partition of the items.
static int check_layout(unsigned long n, int W, int r, const SymLayoutKey& key)
{
    const SymFill fill = sym_fill(n, W, key.pad_aware);
    SymHostLayout L;
    plan_sym_layout(W, r, fill, key, L);
    CHECK(!L.items.empty() && L.own >= 0 && (size_t)L.own <= L.items.size() && L.t1 >= 0 && L.t1 <= L.own, "item counts");
    const char* what = "";
    if (key.exchange_mode) {
        CHECK(L.passes.size() == 1, "the exchange pipeline has one pass");
        CHECK(!check_set(L.items, 0, (size_t)L.own, L.table_tri, L.floats_tri, key.waves, &what), "triangle set: %s", what);
        CHECK(!check_set(L.items, (size_t)L.own, L.items.size(), L.table_main, L.floats_main, key.waves, &what), "main set: %s", what);
        CHECK((int)L.table_tri.size() == fill.tb, "the triangle's table has %zu entries for %d blocks", L.table_tri.size(), fill.tb);
        return 0;
    }
    size_t next = 0;
    CHECK(key.budget_floats || L.passes.size() == 1, "passes without a budget");
    for (const SymPass& ps : L.passes) {
        CHECK((size_t)ps.item_first == next && ps.item_count > 0 && ps.floats <= L.floats_main, "passes do not partition the items");
        next += (size_t)ps.item_count;
        const std::vector<MurbSymBlockRows> table(L.table_main.begin() + ps.table_first, L.table_main.begin() + ps.table_first + ps.table_count);
        CHECK(!check_set(L.items, (size_t)ps.item_first, next, table, ps.floats, key.waves, &what), "pass: %s", what);
    }
    CHECK(next == L.items.size(), "passes do not partition the items");
    if (L.passes.size() == 1) CHECK((int)L.table_main.size() == fill.tb, "one GPU: a table entry per block");
    return 0;
}

// ---- the plan choice (murb_choose.h) --------------------------------------------------------------------------------------
// A context of n bodies on W ranks as the library sets it up: the HBM of an MI355X, default options.
static PlanInputs inputs(unsigned long n, int W, int cu_count)
{
    PlanInputs in;
    in.n = n;
    in.world = W;
    in.slice = slice_slots(n, W);
    in.slots = in.slice * (unsigned long)W;
    in.cu_count = cu_count;
    in.device_mem = (size_t)288 << 30;
    in.resident_per_cu = 2;
    return in;
}

// (e) a pair-symmetric choice chained to the layout the library would build for it (default options; every rank up to 4,
// ranks 0, 3, 6 of 8); a layout already checked is not checked again
static long g_plans = 0;
static int chain_to_layout(const PlanInputs& in, const Plan& p)
{
    static std::set<std::vector<long>> seen;
    const SymLayoutKey key = sym_layout_key(in, p, in.world > 1, 1, 50, false, true);
    for (int r = 0; r < in.world; r += (in.world > 4 ? 3 : 1)) {
        if (!seen.insert({(long)in.n, in.world, r, key.split, key.waves, key.taper, key.diag_tri, key.tri_div, (long)key.budget_floats}).second) continue;
        if (check_layout(in.n, in.world, r, key)) return 1;
        ++g_plans;
    }
    return 0;
}

#define EXPECT(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "choice, n=%lu W=%d cu=%d variant=%d jsplit=%d sym_waves=%d -> variant %d parts %d+%d split %d waves %d taper %d tri %d: ", \
    in.n, in.world, in.cu_count, in.variant, in.jsplit, in.sym_waves, p.variant, p.parts_local, p.parts_remote, p.split, p.waves, p.taper, (int)p.diag_tri); FAIL(__VA_ARGS__); } } while (0)

// (a), (b): one rank, T = 1 ... 30 blocks: full, 37 bodies short of full, 65 bodies and one body in the last block
static int check_block_sweep(int cu_count)
{
    std::set<int> variants, waves, splits, tapers;
    for (int T = 1; T <= 30; ++T) {
        std::vector<unsigned long> sizes = {1024ul * T, 1024ul * T - 37};
        if (T >= 2) { sizes.push_back(1024ul * (T - 1) + 65); sizes.push_back(1024ul * (T - 1) + 1); }   // a truly cut item; a one-body block
        for (unsigned long n : sizes) {
            const PlanInputs in = inputs(n, 1, cu_count);
            const Plan p = make_plan(in);
            variants.insert(p.variant);
            if (T <= 4 || T == 6) {   // the fused one-launch step (fused_one_sided_wins)
                EXPECT(p.variant == 1 && p.parts_local == 1 && p.parts_remote == 0, "expected the one-sided plan in one chunk");
                continue;
            }
            EXPECT(p.variant == 8 && p.symmetric && p.parts_local == 0, "expected the pair-symmetric plan");
            waves.insert(p.waves); splits.insert(p.split); tapers.insert(p.taper);
            if (T >= 28 && cu_count == 256) EXPECT(p.waves == 4 && p.split == 4 && p.taper == 5 && !p.diag_tri, "expected the plan of the larger problems");
            if (T <= 27 && cu_count != 256)   // the table was measured on 256 CUs: any other count keeps the 8-wave plan
                EXPECT(p.waves == 8 && p.split == (T < 10 ? 8 : 4) && p.taper == 30 && p.diag_tri, "expected the 8-wave plan");
            if (chain_to_layout(in, p)) return 1;
        }
    }
    if (cu_count != 256) return 0;
    // what tests/test_pair_coverage.py::test_block_count_sweep_reached_every_plan asserts on the GPU
    const bool reached = variants.count(1) && variants.count(8) && waves.count(4) && waves.count(8) && splits.count(4) && splits.count(8) &&
                         splits.count(16) && tapers.count(5) && tapers.count(30);
    if (!reached) FAIL("the block-count sweep no longer reaches every plan of the table");
    return 0;
}

// (c) forced options win
static int check_forced_options()
{
    for (int W : {1, 4})
        for (int jsplit : {1, 2, 4, 8, 16})
            for (int sym_waves : {4, 8}) {
                PlanInputs in = inputs(200000, W, 256);
                in.jsplit = jsplit;
                in.sym_waves = sym_waves;
                const Plan p = make_plan(in);
                int split = jsplit;
                while (split > 1 && MURB_SYM_BLOCK / split < 16 * sym_waves) split /= 2;   // an item is at least one group per wave
                while (split > 1 && in.world > 1 && sym_row_bytes(in, split) >= in.device_mem / 2) split /= 2;   // and its rows fit
                EXPECT(p.variant == 8 && p.split == split && p.waves == sym_waves, "expected split %d", split);
            }
    for (int taper : {0, 17, 100})
        for (int diag_tri : {0, 1})
            for (int sym_red : {0, 1}) {
                PlanInputs in = inputs(30000, 1, 256);
                in.taper = taper; in.diag_tri = diag_tri; in.sym_red = sym_red;
                const Plan p = make_plan(in);
                EXPECT(p.variant == 8 && p.taper == taper && p.diag_tri == (diag_tri != 0) && p.red == sym_red, "forced taper / diag_tri / sym_red");
            }
    return 0;
}

// (d) what holds for every choice
static int check_invariants(unsigned long n, int W, int variant)
{
    PlanInputs in = inputs(n, W, 256);
    in.variant = variant;
    const Plan p = make_plan(in);
    EXPECT(p.variant >= 1 && p.variant <= kNumVariants && (variant == 0 || p.variant == variant), "resolved variant");
    const unsigned long tiles_local = in.slice / MURB_TILE_BODIES, tiles_remote = (in.slots - in.slice) / MURB_TILE_BODIES;
    if (variant == 0 && W > 1) {
        const bool fits = sym_row_bytes(in, 1) < in.device_mem / 2;
        const int want = sym_items_per_rank(in) >= 400 && fits ? 8 : (in.slice <= 16384 ? 2 : 1);
        EXPECT(p.variant == want, "multi-rank default: expected variant %d", want);
    }
    if (p.symmetric) {
        EXPECT(p.split == 1 || p.split == 2 || p.split == 4 || p.split == 8 || p.split == 16, "split");
        EXPECT((p.waves == 4 || p.waves == 8) && MURB_SYM_BLOCK / p.split >= 16 * p.waves, "an item is at least one group per wave");
        const int div = plan_tri_div(in, p);
        EXPECT((div == 1 || div == 2 || div == 4) && (W > 1 || div == 1), "tri_div %d", div);
        return chain_to_layout(in, p);
    }
    if (p.persistent) {
        unsigned long first, count;
        partition(n, W, 0, &first, &count);
        const long groups = (long)((count + 31) / 32);
        for (int k = 0; k < (W > 1 ? 2 : 1); ++k)
            EXPECT(p.sched[k].nblocks >= 1 && p.sched[k].nblocks <= (kRowsPerLaunch - 2) * groups, "schedule %d: %d workgroups for %ld groups", k, p.sched[k].nblocks, groups);
        return 0;
    }
    EXPECT((tiles_local == 0 || p.parts_local >= 1) && (tiles_remote == 0 || p.parts_remote >= 1), "a launch with tiles has no chunk");
    EXPECT(p.parts_local <= kMaxParts / 2 && p.parts_remote <= kMaxParts / 2 && p.parts_local + p.parts_remote <= kMaxParts, "more chunks than rows");
    return 0;
}

// (e) j chunks of the Hermite sweep (hermite_parts, read back as info("hermite_parts")): "jsplit" clamped to the layout tiles and
// to kMaxParts / 2, so that no chunk of murb_force_jerk_sweep's rule [tiles c / parts, tiles (c + 1) / parts) is empty
static int check_hermite_parts()
{
    for (unsigned long n : {1ul, 2ul, 17ul, 513ul, 1025ul, 2049ul, 3035ul, 12001ul, 30000ul, 200000ul})
        for (int jsplit = 0; jsplit <= kMaxParts / 2; ++jsplit) {
            PlanInputs in = inputs(n, 1, 256);
            in.jsplit = jsplit;
            const long tiles = (long)(in.slots / MURB_TILE_BODIES);
            const int parts = hermite_parts(in);
            const Plan p = make_plan(in);   // for EXPECT's message
            const long most = std::min<long>(tiles, kMaxParts / 2);
            EXPECT(parts >= 1 && parts <= most && (jsplit == 0 || parts == std::min<long>(jsplit, most)), "hermite_parts %d of %ld tiles", parts, tiles);
            if (jsplit == 0 && n == 30000) EXPECT(parts > 1, "the default sweep at N = 30 000 is chunked");
            for (int c = 0; c < parts; ++c)
                EXPECT(tiles * c / parts < tiles * (c + 1) / parts, "chunk %d of %d is empty", c, parts);
        }
    return 0;
}

// (f) "sym_wide": which form of the pair factor an upload selects (sym_wide_needed) and how the option overrides it
static int check_sym_wide()
{
    struct Case { double reach, soft; bool wide; const char* what; };
    const Case cases[] = {
        {6.9e8, 2e8, false, "the galaxy scheme"}, {1.95e9, 2e8, false, "the random scheme"}, {2e11, 1e3, true, "1e11 m binaries"},
        {12.0, 1e-3, false, "Henon units"}, {2.4e5, 10.0, false, "AU, a cluster of 2e4 AU"}, {1.2e14, 1e9, true, "SI at 1e13 m"},
        {1.2e16, 1e11, true, "SI at 1e15 m"}, {3.7e17, 1e13, true, "SI at 1 pc"}, {1.1e-8, 0x1p-40, false, "G = 1 at 2^-30"},
        {0x1p34, 1.0, false, "the last reach of the fast form"}, {0x1.000002p34, 1.0, true, "one step beyond it"},
        {1.0, 0x1p-40, false, "the smallest softening of the fast form"}, {1.0, 0x1.fffffep-41, true, "one step below it"},
        {1.0, 0.0, true, "no softening"}, {HUGE_VAL, 1.0, true, "an infinite extent"}, {std::nan(""), 1.0, true, "a NaN extent"},
        {1.0, std::nan(""), true, "a NaN softening"},
    };
    for (const Case& c : cases)
        if (sym_wide_needed(c.reach, c.soft) != c.wide) FAIL("sym_wide_needed(%g, %g) is not %d: %s", c.reach, c.soft, (int)c.wide, c.what);
    // the fast form's cube of 1 / r stays a normal fp32 number with 2^8 to spare at the far end and 2^7 below the largest at the near one
    if (std::pow(kSymFastMaxReach * 256.0, -3.0) < (double)FLT_MIN) FAIL("the far threshold leaves less than 2^8 of headroom");
    if (std::pow(kSymFastMinSoft, -3.0) * 128.0 > (double)FLT_MAX) FAIL("the near threshold lets the cube of 1 / soft overflow");
    for (int needed = 0; needed <= 1; ++needed)
        if (sym_wide_chosen(-1, needed) != (needed != 0) || sym_wide_chosen(0, needed) || !sym_wide_chosen(1, needed))
            FAIL("sym_wide_chosen: -1 follows the upload, 0 and 1 are forced");
    return 0;
}

// The layouts of n bodies on W ranks under every key of the sweep: splits x waves x tapers x (plain | triangular diagonals | XCD
// order | several passes | the exchange pipeline | its triangle launches cut in 4)
static int sweep_keys(unsigned long n, int W, std::initializer_list<int> tapers)
{
    for (int split : {1, 4, 8, 16})
        for (int waves : {4, 8}) {
            if (MURB_SYM_BLOCK / split < 16 * waves || (split == 8 && waves == 4)) continue;   // 8 x 4 lies between 4 x 4 and 16 x 4
            for (int taper : tapers)
                for (int variant = 0; variant < 6; ++variant) {
                    SymLayoutKey key;
                    key.split = split; key.waves = waves; key.taper = taper;
                    key.diag_tri = variant & 1;
                    key.exchange_mode = W > 1 || variant >= 4;
                    key.overlap = 1; key.tri_first_pct = 50;
                    key.xcd_order = variant == 2;
                    key.tri_div = (key.exchange_mode && variant == 5) ? 4 : 1;
                    key.budget_floats = (!key.exchange_mode && variant == 3) ? (size_t)40 * MURB_SYM_BLOCK : 0;
                    for (int r = 0; r < W; r += (W > 4 ? 3 : 1)) {
                        if (check_layout(n, W, r, key)) return 1;
                        ++g_plans;
                    }
                }
        }
    return 0;
}

// `rem` real bodies in a slice's last block, on both sides of every length the work list can cut that block to (the list of
// tests/helpers/ragged.py): one rank with 1 and 3 full blocks before it; 2, 3 and 4 ranks of two blocks a slice whose last
// blocks hold rem and rem - 1 bodies in every mix (rem = 1: a wholly empty block, which counts as holding one body)
static int check_ragged_residues()
{
    const int rems[] = {1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 193, 255, 257, 383, 385, 511, 513, 767, 769, 895, 897, 959, 961, 1023};
    for (int rem : rems) {
        for (int B : {1, 3})
            if (sweep_keys(1024ul * B + rem, 1, {0, 30, 100})) return 1;
        for (int W : {2, 3, 4})
            for (int k = 0; k < W; ++k)
                if (sweep_keys((unsigned long)W * (1024 + rem) - k, W, {0, 30, 100})) return 1;
    }
    return 0;
}

int main()
{
    const unsigned long sizes[] = {1, 250, 1025, 2049, 9001, 30000, 60001};
    for (unsigned long n : sizes)
        for (int W : {1, 2, 3, 4, 8})
            if ((unsigned long)W <= n && sweep_keys(n, W, {0, 40})) return 1;
    if (check_ragged_residues()) return 1;
    for (int cu_count : {256, 304, 128})
        if (check_block_sweep(cu_count)) return 1;
    if (check_forced_options()) return 1;
    if (check_hermite_parts()) return 1;
    if (check_sym_wide()) return 1;
    for (unsigned long n : {1ul, 250ul, 1025ul, 2049ul, 9001ul, 30000ul, 60001ul, 100000ul, 200000ul, 1000000ul})
        for (int W : {1, 2, 3, 4, 8})
            for (int variant : {0, 1, 2, 7, 8})
                if ((unsigned long)W <= n && check_invariants(n, W, variant)) return 1;
    std::printf("ok %ld\n", g_plans);
    return 0;
}
