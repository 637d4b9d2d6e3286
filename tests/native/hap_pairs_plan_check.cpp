// hap_pairs_plan_check.cpp -- the host decisions of pantax_hip_db_hap_pairs (pantax_amd/csrc/hap_pairs_plan.hpp) at their edges.  A program of its own:
// tests/test_hap_pairs_plan.py compiles it with hap_pairs_plan.cpp by the host compiler under -fsanitize=address,undefined and runs it; it returns
// non-zero at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
#include "hap_pairs_plan.hpp"

using namespace ptx;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "hap_pairs_plan_check:%d: %s\n", __LINE__, #cond);   \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static void tiles() {
    // the block-pair table of nw = 1 .. 4 words, written out: row-major over the upper triangle
    const std::vector<std::vector<std::pair<uint32_t, uint32_t>>> want = {
        {{0, 0}},
        {{0, 0}, {0, 1}, {1, 1}},
        {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}},
        {{0, 0}, {0, 1}, {0, 2}, {0, 3}, {1, 1}, {1, 2}, {1, 3}, {2, 2}, {2, 3}, {3, 3}}};
    for (uint32_t nw = 1; nw <= 4; ++nw) {
        CHECK(hap_pairs_tiles(nw) == want[nw - 1].size() && hap_pairs_tiles(nw) == nw * (nw + 1) / 2);
        std::set<std::pair<uint32_t, uint32_t>> seen;
        for (uint32_t t = 0; t < hap_pairs_tiles(nw); ++t) {
            const HapPairsTile bp = hap_pairs_tile(nw, t);
            CHECK(bp.wa == want[nw - 1][t].first && bp.wb == want[nw - 1][t].second);
            CHECK(bp.wa <= bp.wb && bp.wb < nw);                      // the upper triangle ...
            CHECK(seen.insert({bp.wa, bp.wb}).second);                // ... every block pair once ...
        }
        CHECK(seen.size() == (size_t)nw * (nw + 1) / 2);              // ... and all of it: a bijection
    }
    CHECK(hap_pairs_tiles(0) == 0u);
    // the mapping beyond the served widths stays a bijection (nothing in it knows the limit)
    for (const uint32_t nw : {5u, 9u}) {
        std::set<std::pair<uint32_t, uint32_t>> seen;
        for (uint32_t t = 0; t < hap_pairs_tiles(nw); ++t) { const HapPairsTile bp = hap_pairs_tile(nw, t); CHECK(bp.wa <= bp.wb && bp.wb < nw && seen.insert({bp.wa, bp.wb}).second); }
    }
}

static void sizing() {
    // K = 0, 1, 64, 65, 256 in one selection
    const uint64_t off[] = {0, 0, 1, 65, 130, 386};
    uint64_t pair_off[6];
    for (uint64_t &x : pair_off) x = 77;
    CHECK(hap_pairs_offsets(5, off, pair_off) == 5u);
    CHECK(pair_off[0] == 0 && pair_off[1] == 0 && pair_off[2] == 1 && pair_off[3] == 1 + 64 * 64 && pair_off[4] == 1 + 4096 + 65 * 65 && pair_off[5] == 1 + 4096 + 4225 + 256 * 256);
    CHECK(HAP_PAIRS_MAX_K == 256);
    // K = 257 is refused, the species named; the offsets are written whole all the same
    const uint64_t wide[] = {0, 3, 260, 262, 600};
    uint64_t po[5];
    CHECK(hap_pairs_offsets(4, wide, po) == 1u);
    CHECK(po[0] == 0 && po[1] == 9 && po[2] == 9 + 257 * 257 && po[3] == po[2] + 4 && po[4] == po[3] + 338ull * 338ull);
    const uint64_t edge[] = {0, 256, 513};
    uint64_t pe[3];
    CHECK(hap_pairs_offsets(2, edge, pe) == 1u && hap_pairs_offsets(1, edge, pe) == 1u && pe[1] == 65536);
    uint64_t p0[1] = {5};
    CHECK(hap_pairs_offsets(0, edge, p0) == 0u && p0[0] == 0);      // no species: nothing to refuse
    // live bits of a word on route 2, and the words the plan implies
    CHECK(hap_pairs_live(0, 0) == 0ull && hap_pairs_live(1, 0) == 1ull && hap_pairs_live(64, 0) == ~0ull && hap_pairs_live(64, 1) == 0ull);
    CHECK(hap_pairs_live(65, 0) == ~0ull && hap_pairs_live(65, 1) == 1ull && hap_pairs_live(130, 2) == 3ull && hap_pairs_live(256, 3) == ~0ull && hap_pairs_live(256, 4) == 0ull);
}

static void chunks_and_columns() {
    CHECK(hap_pairs_chunk(0, 0, 0) == 1024u && hap_pairs_chunk(1, 1, 0) == 1024u && hap_pairs_chunk(5, 6, 0) == 1024u);   // 32 * 30 = 960: the floor
    CHECK(hap_pairs_chunk(6, 6, 0) == 1152u && hap_pairs_chunk(16, 16, 0) == 8192u && hap_pairs_chunk(32, 32, 0) == 32768u && hap_pairs_chunk(64, 64, 0) == 32768u);
    CHECK(hap_pairs_chunk(64, 1, 0) == 2048u);
    CHECK(hap_pairs_chunk(64, 64, 1) == 64u && hap_pairs_chunk(3, 3, 64) == 64u && hap_pairs_chunk(3, 3, 65) == 128u && hap_pairs_chunk(3, 3, 1 << 30) == 32768u);
    CHECK(HAP_PAIRS_CHUNK_MAX < (1u << 16));                          // n_nodes of a chunk fits the 16 bits above a packed counter's length
    CHECK(hap_pairs_cols(0ull) == 0u && hap_pairs_cols(1ull) == 8u && hap_pairs_cols(0x80ull) == 8u && hap_pairs_cols(0x100ull) == 16u && hap_pairs_cols(0xFFFFull) == 16u);
    CHECK(hap_pairs_cols(0x10000ull) == 32u && hap_pairs_cols(0xFFFFFFFFull) == 32u && hap_pairs_cols(1ull << 32) == 64u && hap_pairs_cols(~0ull) == 64u && hap_pairs_cols(1ull << 63) == 64u);
}

static void mirror() {
    // K = 130: entries [a][b] of the block pairs wa <= wb are given, the rest zero; the mirror fills [b][a] for a / 64 < b / 64 and nothing else
    const uint64_t K = 130;
    std::vector<uint64_t> m(K * K * 2, 0);
    const auto val = [](uint64_t a, uint64_t b, int q) { return (a * 1000 + b) * 2 + (uint64_t)q + 1; };
    for (uint64_t a = 0; a < K; ++a)
        for (uint64_t b = 0; b < K; ++b)
            if (a / 64 <= b / 64) { m[(a * K + b) * 2] = val(a, b, 0); m[(a * K + b) * 2 + 1] = val(a, b, 1); }
    hap_pairs_mirror(m.data(), K);
    for (uint64_t a = 0; a < K; ++a)
        for (uint64_t b = 0; b < K; ++b) {
            const bool given = a / 64 <= b / 64;
            CHECK(m[(a * K + b) * 2] == (given ? val(a, b, 0) : val(b, a, 0)) && m[(a * K + b) * 2 + 1] == (given ? val(a, b, 1) : val(b, a, 1)));
        }
    std::vector<uint64_t> one(64 * 64 * 2, 9);                         // one word: nothing to mirror
    hap_pairs_mirror(one.data(), 64);
    for (uint64_t x : one) CHECK(x == 9);
    hap_pairs_mirror(nullptr, 0);
}

int main() {
    tiles();
    sizing();
    chunks_and_columns();
    mirror();
    std::printf("hap_pairs_plan_check: ok\n");
    return 0;
}
