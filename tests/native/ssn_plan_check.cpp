// ssn_plan_check.cpp -- geometry and workspace layout of the node-order row sort (pantax_amd/csrc/ssn_plan.hpp) at their edges.  A program of its
// own: tests/test_ssn_plan.py compiles it with ssn_plan.cpp by the host compiler under -fsanitize=address,undefined and runs it; it returns non-zero
// at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include "ssn_plan.hpp"

using namespace ptx;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "ssn_plan_check:%d: %s\n", __LINE__, #cond);    \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

// The numbers below are worked out by hand from the formula the entry point used before there was a plan: nt = max(1, ceil(seg / 2048)) tiles,
// per = clamp(ceil(nt S / 8192), 1, nt), G = ceil(nt / per); the tie grid is ceil(seg / 8192).  They hold for the default tile of 2048 nodes.
static void geometry() {
    static_assert(SN_TILE == 2048 && SN_TARGET_WGS == 8192 && SN_TIE_ROWS == 8192, "the literals below are for the default build");
    struct Case { uint32_t S; uint64_t seg; uint32_t per, G, tie; };
    const Case cases[] = {
        {1, 1, 1, 1, 1},                          // nt 1
        {22, 3000000, 4, 367, 367},               // nt 1465, nt S = 32230 -> ceil 4.93.. is 4 by the integer formula (32230 + 8191) / 8192
        {4101, 6000, 2, 2, 1},                    // nt 3, nt S = 12303 -> 2; the second workgroup's range [2, 4) is clamped to the 3 tiles
        {65535, 1ull << 26, 32768, 1, 8192},      // nt 32768, nt S / 8192 = 262140 > nt: one workgroup walks the whole segment
        {2048, 8192, 1, 4, 1},                    // nt 4, nt S = 8192 exactly: still one tile per workgroup
        {2731, 4097, 2, 2, 1},                    // nt 3, nt S = 8193: the first product that takes two
    };
    for (const Case &c : cases) {
        const SsnPlan p = ssn_plan(c.S, c.seg, c.seg * c.S);
        CHECK(p.per == c.per);
        CHECK(p.G == c.G);
        CHECK(p.tie_grid == c.tie);
    }
}

static void layout() {
    const uint32_t Ss[] = {1, 2, 3, 7, 22, 4101, 65535};
    const uint64_t segs[] = {1, 2048, 2049, 4097, 6000, 3000000};
    for (const uint32_t S : Ss)
        for (const uint64_t seg : segs)
            for (uint64_t par = 0; par < 2; ++par) {
                const uint64_t V = seg + S + par;           // (the layout takes any V; both parities)
                const SsnPlan p = ssn_plan(S, seg, V);
                const uint64_t nt = (seg + SN_TILE - 1) / SN_TILE;
                CHECK(p.per >= 1 && p.per <= nt && (uint64_t)p.G * p.per >= nt);
                CHECK(p.tie_grid == (seg + SN_TIE_ROWS - 1) / SN_TIE_ROWS);
                const size_t SG = (size_t)S * p.G;
                // the regions in order, with the words their users index: S per-segment blocks; a count matrix row and a staged-row count per
                // (segment, workgroup); a double (two words) per (segment, workgroup); seg_n[S]; seg_out[S + 1] (ssn_segscan_kernel writes
                // seg_out[S]); sub_k[S][SN_NWH]; a u16 per node; a NodePartial per (segment, workgroup)
                const size_t off[] = {p.ws, p.cntm, p.stage_cnt, p.c0p, p.seg_n, p.seg_out, p.sub_k, p.ids, p.npart, p.total_words};
                const size_t need[] = {(size_t)S * SN_WS_WORDS, SG * SN_NBUCKET, SG, 2 * SG, S, (size_t)S + 1, (size_t)S * SN_NWH, (size_t)((2 * V + 3) / 4),
                                       SG * SN_NODE_PARTIAL_WORDS};
                CHECK(p.ws == 0);
                for (int i = 0; i < 9; ++i) {
                    CHECK(need[i] > 0);
                    CHECK(off[i] + need[i] <= off[i + 1]);  // in today's order, and so pairwise disjoint; each at least as large as its user indexes
                }
                CHECK(p.c0p % 2 == 0 && p.npart % 2 == 0);   // 8-byte elements from a base that is 8-byte aligned
                CHECK(p.ws % 4 == 0 && p.cntm % 4 == 0);     // 16-byte tree nodes and 16-byte steps over the matrix
                // what sample_sort_nodes_ws_elems() returned before the plan: no allocation grows
                const size_t parent = (size_t)S * SN_WS_WORDS + (size_t)S * p.G * (SN_NBUCKET + 1 + 2) + (V + 1) / 2 + (2 + (size_t)SN_NWH) * (size_t)S + 20 +
                                      (size_t)S * p.G * (32 / 4) + 4;
                CHECK(p.total_words <= parent);
            }
}

int main() {
    static_assert(SN_WS_WORDS % 4 == 0 && SN_NBUCKET % 4 == 0, "16-byte steps");
    geometry();
    layout();
    std::printf("ssn_plan_check: ok\n");
    return 0;
}
