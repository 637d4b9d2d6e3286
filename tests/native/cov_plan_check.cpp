// cov_plan_check.cpp -- the coverage pass's host-side decisions (pantax_amd/csrc/cov_plan.hpp) at their edges.  A program of its own: tests/test_cov_plan.py
// compiles it with cov_plan.cpp by the host compiler under -fsanitize=address,undefined and runs it; it returns non-zero at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cov_plan.hpp"

using namespace ptx;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "cov_plan_check:%d: %s\n", __LINE__, #cond);     \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

static bool fast_is(const CovFastShape &s, int u, int p, int w) { return s.u == u && s.passes == p && s.win == w; }
static bool long_is(const CovLongShape &s, int u, int w, uint32_t groups, uint32_t back) { return s.u == u && s.win == w && s.chunk_groups == groups && s.win_back == back; }
static bool step_is(const CovStepShape &s, int u, int p) { return s.u == u && s.passes == p; }
using U32s = std::vector<uint32_t>;
using I64s = std::vector<int64_t>;

// a plan of the default options over reads of this shape
static CovPlan plan_of(uint64_t T_pad, uint32_t n_long, uint32_t n_slots, uint32_t n_items, uint64_t R, bool general = false, const char *cov_long = "",
                       int covf = -1, int covl = -1, int covs = -1, int xcd = 0) {
    return cov_plan(T_pad, n_long, n_slots, n_items, R, general, cov_long, covf, covl, covs, xcd);
}

static void fast_codes() {
    const struct { int code, u, p, w; } table[] = {{182, 1, 8, 2048},  {242, 2, 4, 2048},  {282, 2, 8, 2048},  {283, 2, 8, 3072},  {284, 2, 8, 4096},
                                                   {243, 2, 4, 3072},  {2823, 2, 8, 2304}, {2825, 2, 8, 2560}, {2423, 2, 4, 2304}, {2425, 2, 4, 2560},
                                                   {1823, 1, 8, 2304}, {4423, 4, 4, 2304}, {442, 4, 4, 2048},  {443, 4, 4, 3072}};
    for (const auto &t : table) {
        CHECK(fast_is(cov_fast_shape(t.code), t.u, t.p, t.w));
        CHECK(fast_is(plan_of(1 << 20, 0, 10, 3, 10, false, "", t.code).fast, t.u, t.p, t.w));   // the option overrides the default
    }
    CHECK(fast_is(cov_fast_shape(999), 2, 4, 2048));    // an unknown code
    CHECK(fast_is(plan_of((1ull << 28) - 64, 0, 10, 3, 10).fast, 2, 4, 2304));      // 2423 below 2^28 steps
    CHECK(fast_is(plan_of(1ull << 28, 0, 10, 3, 10).fast, 2, 8, 2304));             // 2823 from there
    CHECK(fast_is(plan_of(1ull << 28, 0, 10, 3, 10, false, "", 0).fast, 2, 8, 2304));   // 0 is "no option"
}

static void long_codes() {
    CHECK(long_is(cov_long_shape(1120), 1, 2048, 8, 0));
    CHECK(long_is(cov_long_shape(1222), 1, 2048, 16, 512));
    CHECK(long_is(cov_long_shape(1232), 1, 3072, 16, 512));
    CHECK(long_is(cov_long_shape(2242), 2, 4096, 16, 512));
    CHECK(long_is(cov_long_shape(2448), 2, 4096, 32, 2048));
    CHECK(long_is(cov_long_shape(2848), 2, 4096, 64, 2048));
    CHECK(long_is(cov_long_shape(2834), 2, 3072, 64, 1024));
    CHECK(long_is(plan_of(1 << 20, 5, 10, 3, 10).lng, 2, 3072, 64, 1024));          // the default: 64 groups, window 3072, back 1024
    CHECK(long_is(plan_of(1 << 20, 5, 10, 3, 10, false, "", -1, 1222).lng, 1, 2048, 16, 512));
    CHECK(long_is(cov_long_shape(21224), 2, 2048, 96, 1024));                       // five digits: <U><GG><W><B>
    CHECK(long_is(cov_long_shape(11631), 1, 3072, 128, 256));
    CHECK(long_is(cov_long_shape(1030), 1, 3072, 8, 0));                            // G = 0 still gives a workgroup 8 groups
    CHECK(long_is(cov_long_shape(3252), 2, 3072, 16, 512));                         // any other <U><W>: (2, 3072)
    CHECK(long_is(cov_long_shape(2212), 2, 3072, 16, 512));
}

static void step_codes() {
    CHECK(step_is(cov_step_shape(22), 2, 2));
    CHECK(step_is(cov_step_shape(21), 2, 1));
    CHECK(step_is(cov_step_shape(41), 4, 1));
    CHECK(step_is(cov_step_shape(42), 4, 2));
    CHECK(step_is(cov_step_shape(18), 1, 8));
    CHECK(step_is(cov_step_shape(14), 1, 4));
    CHECK(step_is(cov_step_shape(77), 1, 4));
    CHECK(step_is(plan_of((1ull << 25) - 64, 5, 10, 3, 10, false, "step").step, 1, 4));   // 14 below 2^25 steps
    CHECK(step_is(plan_of(1ull << 25, 5, 10, 3, 10, false, "step").step, 1, 8));          // 18 from there
    CHECK(step_is(plan_of(1ull << 25, 5, 10, 3, 10, false, "step", -1, -1, 42).step, 4, 2));
    CHECK(plan_of(1 << 20, 5, 10, 3, 10, false, "step", -1, -1, -1, 1).xcd_map == 1u);
    CHECK(plan_of(1 << 20, 5, 10, 3, 10, false, "step").xcd_map == 0u);
}

static bool runs(const CovPlan &p, bool fast, bool lng, bool step) { return p.run_fast == fast && p.run_long == lng && p.run_step == step; }
static void run_conditions() {
    CHECK(runs(plan_of(1 << 20, 0, 10, 3, 10), true, false, false));                       // short reads only
    CHECK(runs(plan_of(1 << 20, 10, 10, 3, 10), false, true, false));                      // long reads only
    CHECK(runs(plan_of(1 << 20, 4, 10, 3, 10), true, true, false));                        // mixed
    CHECK(plan_of(1 << 20, 4, 10, 3, 10).only_long);
    const CovPlan g = plan_of(1 << 20, 0, 10, 3, 10, true);                                // cov_general: every group through the long kernel
    CHECK(runs(g, false, true, false) && !g.only_long);
    CHECK(runs(plan_of(1 << 20, 4, 10, 3, 10, true), false, true, false));
    CHECK(runs(plan_of(1 << 20, 4, 10, 3, 10, false, "step"), true, false, true));         // cov_long=step
    CHECK(runs(plan_of(1 << 20, 0, 10, 3, 10, false, "step"), true, false, false));
    const CovPlan gs = plan_of(1 << 20, 0, 10, 3, 10, true, "step");
    CHECK(runs(gs, false, false, true) && !gs.only_long);
    CHECK(runs(plan_of(0, 0, 0, 0, 0), false, false, false));                              // R = 0
    CHECK(runs(plan_of(1 << 20, 4, 10, 3, 0), false, false, false));
    CHECK(runs(plan_of(0, 0, 0, 0, 10), false, false, false));                             // reads with empty walks only
    CHECK(runs(plan_of(1 << 20, 0, 10, 0, 10), false, false, false));                      // n_items = 0
    CHECK(runs(plan_of(1 << 20, 4, 10, 0, 10), false, true, false));
}

static void item_selection() {
    const U32s blocks = {0, 0, 1, 3, 3, 4, 7};
    CovItemSel s = cov_item_select(blocks, 11, I64s{6149}, I64s{8202});                    // blocks 3 .. 4, and the item in front
    CHECK(s.on && s.n_sel == 4 && s.sel == (U32s{2, 3, 4, 5}));
    s = cov_item_select(blocks, 11, I64s{6149, 0}, I64s{8202, 100});
    CHECK(s.on && s.n_sel == 6 && s.sel == (U32s{0, 1, 2, 3, 4, 5}));
    s = cov_item_select(blocks, 11, I64s{0}, I64s{16383});                                 // every id: the list is not worth it
    CHECK(!s.on && s.n_sel == 7 && s.sel.empty());
    s = cov_item_select(blocks, 11, I64s{10300}, I64s{14000});                             // inside blocks 5 .. 6, which open no item: the one-back item
    CHECK(s.on && s.n_sel == 1 && s.sel == (U32s{5}));
    s = cov_item_select(U32s{2, 3}, 11, I64s{10}, I64s{2000});                             // inside block 0, in front of every item
    CHECK(s.on && s.n_sel == 0 && s.sel.empty());
    // two overlapping ranges never list an item twice
    const U32s many = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19};
    s = cov_item_select(many, 11, I64s{4096, 6144, 4096}, I64s{10239, 12287, 5000});
    CHECK(s.on && s.n_sel == 5 && s.sel == (U32s{1, 2, 3, 4, 5}));
    // 8 of 9 items would be listed: 8 + 8 / 8 is not below 9
    s = cov_item_select(U32s{0, 1, 2, 3, 4, 5, 6, 7, 8}, 11, I64s{0}, I64s{8 * 2048 - 1});
    CHECK(!s.on && s.n_sel == 9);
    s = cov_item_select(U32s{0, 1, 2, 3, 4, 5, 6, 7, 8}, 11, I64s{0}, I64s{7 * 2048 - 1});
    CHECK(s.on && s.n_sel == 7);
    // a negative range start counts as id 0, an end beyond 32 bits as the last id
    s = cov_item_select(many, 11, I64s{-5}, I64s{100});
    CHECK(s.on && s.sel == (U32s{0}));
    s = cov_item_select(many, 11, I64s{18 * 2048}, I64s{1ll << 40});
    CHECK(s.on && s.sel == (U32s{17, 18, 19}));
}

static void arena_layout_of(uint64_t V, uint64_t U, uint64_t L) {
    const CovArenaLayout a = cov_arena_layout(V, U, L);
    const uint64_t words = (L + 31) / 32 + 1, fwords = (V + 4096 + 63) / 32 + 2, n_trio = U ? U : 1;
    CHECK(a.words == words && a.fwords == fwords && a.n_trio == n_trio);
    CHECK(a.off_trio == V * 8);
    CHECK(a.off_abort == V * 8 + n_trio * 8);
    CHECK(a.off_bm == (a.off_abort + 8 + 15) / 16 * 16 && a.off_bm % 16 == 0 && a.off_bm >= a.off_abort + 8);
    CHECK(a.off_full == a.off_bm + words * 4);
    CHECK(a.total == a.off_full + fwords * 4);
    CHECK(fwords * 32 >= V + 4096);           // a flag for every node of a window that begins at the last node
}
static void arena_layouts() {
    arena_layout_of(1000, 0, 50000);
    arena_layout_of(1000, 77, 50001);
    const CovArenaLayout a = cov_arena_layout(1000, 0, 50000), b = cov_arena_layout(1000, 77, 50001);
    CHECK(a.off_abort == 8008 && a.off_bm == 8016 && a.words == 1564 && a.off_full == 8016 + 6256 && a.fwords == 163 && a.total == 8016 + 6256 + 652);
    CHECK(b.off_abort == 8000 + 616 && b.off_bm == 8624 && b.words == 1564);
}

static void long_nodes() {
    CHECK(!long_node_shape(47 * 1000 + 999, 1000, 48, false));     // L / V = 47
    CHECK(long_node_shape(48 * 1000, 1000, 48, false));            // 48
    CHECK(!long_node_shape(48 * 1000, 1000, 48, true));            // ncs_no_prefix
    CHECK(!long_node_shape(48 * 1000, 1000, 49, false));
    CHECK(!long_node_shape(0, 0, 48, false));                      // an empty graph
}

int main() {
    fast_codes();
    long_codes();
    step_codes();
    run_conditions();
    item_selection();
    arena_layouts();
    long_nodes();
    std::puts("cov_plan_check: ok");
    return 0;
}
