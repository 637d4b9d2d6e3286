// member_plan_check.cpp -- the strain reports' membership decisions (pantax_amd/csrc/member_plan.hpp) at their edges.  A program of its own:
// tests/test_member_plan.py compiles it with member_plan.cpp by the host compiler under -fsanitize=address,undefined and runs it; it returns non-zero
// at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "member_plan.hpp"

using namespace ptx;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "member_plan_check:%d: %s\n", __LINE__, #cond);    \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

static std::vector<uint32_t> iota(uint64_t n) {
    std::vector<uint32_t> v(n);
    std::iota(v.begin(), v.end(), 0u);
    return v;
}

static void routes() {
    // is route 1 open: node -> haplotype words built, and the option is not "walk"; any other value is the default
    CHECK(member_by_node(true, "") && member_by_node(true, "node") && member_by_node(true, "Walk") && member_by_node(true, "walk "));
    CHECK(!member_by_node(true, "walk") && !member_by_node(false, "") && !member_by_node(false, "walk") && !member_by_node(false, "node"));
    const std::vector<uint32_t> h = iota(200);
    for (const bool open : {true, false})
        for (const uint64_t nh : {1ull, 6ull, 64ull, 65ull, 200ull}) {   // nothing chosen: route 0, no words, whatever the species
            const MemberRow r = member_row(open, nh, 77u, h.data(), 0);
            CHECK(r.route == 0u && r.nw == 0u && r.K == 0u && r.bits == 0ull && r.mask_base == 0ull && r.node_base == 77u);
        }
    {   // the border, route 1 open
        const MemberRow a = member_row(true, 64, 5u, h.data(), 3), b = member_row(true, 65, 5u, h.data(), 3);
        CHECK(a.route == 1u && a.nw == 1u && a.K == 3u && a.bits == 7ull && a.node_base == 5u && a.mask_base == 0ull);
        CHECK(b.route == 2u && b.nw == 1u && b.K == 3u && b.bits == 0ull && b.node_base == 5u && b.mask_base == 0ull);
    }
    // route 1 closed (nh_built false; nh_built true under "walk"): route 2 for every nh
    for (const bool closed_open : {member_by_node(false, ""), member_by_node(true, "walk")})
        for (const uint64_t nh : {1ull, 6ull, 64ull, 65ull, 200ull}) {
            const MemberRow r = member_row(closed_open, nh, 0u, h.data(), 1);
            CHECK(r.route == 2u && r.nw == 1u && r.bits == 0ull);
        }
    // an option that is neither empty nor "walk" behaves as the default
    for (const uint64_t nh : {64ull, 65ull}) {
        const MemberRow d = member_row(member_by_node(true, ""), nh, 0u, h.data(), 2), o = member_row(member_by_node(true, "words"), nh, 0u, h.data(), 2);
        CHECK(d.route == o.route && d.nw == o.nw && d.bits == o.bits && d.route == (nh <= 64 ? 1u : 2u));
    }
    // words per node on route 2
    const uint64_t Ks[] = {1, 64, 65, 128, 129};
    const uint32_t nws[] = {1, 1, 2, 2, 3};
    for (int i = 0; i < 5; ++i) {
        CHECK(member_row(true, 200, 0u, h.data(), Ks[i]).nw == nws[i] && member_row(false, 30, 0u, h.data(), Ks[i]).nw == nws[i]);
        CHECK(member_words(Ks[i]) == nws[i] && member_words((uint32_t)Ks[i]) == nws[i]);
    }
    CHECK(member_words(0u) == 0u);
    CHECK(member_row(true, 64, 0u, h.data(), 64).nw == 1u && member_row(true, 64, 0u, h.data(), 64).bits == ~0ull);   // route 1: one word, all of it
    // route-1 bits of a shuffled selection that holds haplotype 63
    const uint32_t sel[] = {40, 63, 0, 7, 31, 32};
    const MemberRow r = member_row(true, 64, 9u, sel, 6);
    CHECK(r.route == 1u && r.K == 6u);
    CHECK(r.bits == ((1ull << 63) | (1ull << 40) | (1ull << 32) | (1ull << 31) | (1ull << 7) | 1ull));
    CHECK(member_bits(sel, 6) == r.bits && member_bits(sel, 0) == 0ull);
}

struct Pos { uint64_t i; uint32_t word, bit; };
// the layout of (K, J) on `route`, and through the filing helper the word (counted from w0) and bit of every candidate
static void layout_is(uint64_t K, uint64_t J, uint32_t route, uint32_t nw, uint32_t w0, uint32_t cwn, const std::vector<uint32_t> &haps, const std::vector<Pos> &spot) {
    const NearMissLayout l = near_miss_layout(K, J, route);
    CHECK(l.nw == nw && l.w0 == w0 && l.cwn == cwn);
    std::vector<uint64_t> at(J, ~0ull);
    member_file_bits(route, haps.data(), J, l.cand0, [&](uint64_t bit, uint64_t i) { CHECK(i < J && at[i] == ~0ull); at[i] = bit; });
    for (uint64_t i = 0; i < J; ++i) {
        CHECK(at[i] < 64ull * cwn);                                        // inside the species' stretch of bit_entry
        if (route == 2u) CHECK(64ull * w0 + at[i] == K + i);               // position K + i of the list Sel ++ Cand
        else CHECK(at[i] == haps[i]);
    }
    for (const Pos &p : spot) CHECK(at[p.i] / 64 == p.word && at[p.i] % 64 == p.bit);
}

static void near_miss() {
    const std::vector<uint32_t> h = iota(256);
    layout_is(0, 0, 0, 0, 0, 0, h, {});                                    // (0, 0): route 0 is the only one a launcher sees there
    layout_is(0, 0, 2, 0, 0, 0, h, {});
    CHECK(near_miss_layout(5, 9, 0).nw == 0u && near_miss_layout(5, 9, 0).cwn == 0u);
    // route 2
    layout_is(0, 1, 2, 1, 0, 1, h, {{0, 0, 0}});
    layout_is(3, 0, 2, 1, 0, 0, h, {});
    layout_is(63, 2, 2, 2, 0, 2, h, {{0, 0, 63}, {1, 1, 0}});              // word 0 is shared: Sel's bits 0 .. 62, the first candidate at bit 63
    layout_is(64, 1, 2, 2, 1, 1, h, {{0, 0, 0}});                          // Sel fills word 0: no shared word
    layout_is(64, 64, 2, 2, 1, 1, h, {{0, 0, 0}, {63, 0, 63}});
    layout_is(10, 250, 2, 5, 0, 5, h, {{0, 0, 10}, {53, 0, 63}, {54, 1, 0}, {117, 1, 63}, {118, 2, 0}, {245, 3, 63}, {246, 4, 0}, {249, 4, 3}});
    layout_is(128, 1, 2, 3, 2, 1, h, {{0, 0, 0}});
    // route 1: one word, bit = haplotype index
    const std::vector<uint32_t> c = {63, 2, 40};
    layout_is(0, 1, 1, 1, 0, 1, c, {{0, 0, 63}});
    layout_is(3, 0, 1, 1, 0, 0, c, {});
    layout_is(61, 3, 1, 1, 0, 1, c, {{0, 0, 63}, {1, 0, 2}, {2, 0, 40}});
    // the layout's nw is the row's over the list Sel ++ Cand
    const uint64_t KJ[][2] = {{0, 1}, {3, 0}, {63, 2}, {64, 1}, {64, 64}, {10, 250}};
    for (const auto &kj : KJ) CHECK(near_miss_layout(kj[0], kj[1], 2).nw == member_row(false, 300, 0u, h.data(), kj[0] + kj[1]).nw);
}

static void filing() {
    const uint32_t N = MEMBER_NO_ENTRY;
    // a db of H = 10 haplotypes in two species (hap_off 0, 6, 10) and C = 5 entries (off 0, 3, 5): per-bit arrays of H + C + 1 entries
    const uint64_t H = 10, C = 5, hap_off[] = {0, 6, 10}, off[] = {0, 3, 5};
    const uint32_t haps[] = {4, 0, 5, /* species 1 */ 3, 1};
    for (const int route1_species : {0, 1, 2}) {   // how many of the two species take route 1 (species 0 first)
        std::vector<uint32_t> got(H + C + 1, N);
        for (uint32_t s = 0; s < 2; ++s) {
            const MemberRow r = member_row((int)s < route1_species, hap_off[s + 1] - hap_off[s], 0u, haps + off[s], off[s + 1] - off[s]);
            const uint32_t base = member_bit_base(r.route, hap_off[s], H, off[s]);
            member_file_bits(r.route, haps + off[s], r.K, 0, [&](uint64_t bit, uint64_t k) { CHECK(got[base + bit] == N); got[base + bit] = (uint32_t)(off[s] + k); });
        }
        //                                  haplotypes of species 0   of species 1    entries 0 .. 4    spare
        const std::vector<uint32_t> both1 = {1, N, N, N, 0, 2,        N, 4, N, 3,     N, N, N, N, N,    N};
        const std::vector<uint32_t> first1 = {1, N, N, N, 0, 2,       N, N, N, N,     N, N, N, 3, 4,    N};
        const std::vector<uint32_t> none1 = {N, N, N, N, N, N,        N, N, N, N,     0, 1, 2, 3, 4,    N};
        CHECK(got == (route1_species == 2 ? both1 : route1_species == 1 ? first1 : none1));
    }
    CHECK(member_bit_base(0, 6, H, 3) == 0u && member_bit_base(1, 6, H, 3) == 6u && member_bit_base(2, 6, H, 3) == 13u);
    // bits ahead of the list (near miss: Sel's): position first + k
    std::vector<uint64_t> at;
    member_file_bits(2, haps, 3, 62, [&](uint64_t bit, uint64_t) { at.push_back(bit); });
    CHECK((at == std::vector<uint64_t>{62, 63, 64}));
}

static void chunks() {
    const uint32_t chunk = 1024;
    // species of 0, chunk - 1, chunk, chunk + 1 and 3 chunk + 5 nodes, one after the other from global node 100
    const uint64_t sizes[] = {0, chunk - 1, chunk, chunk + 1, 3ull * chunk + 5};
    const uint64_t per_tile[] = {0, 1, 1, 2, 4};
    for (const uint64_t tiles : {1ull, 3ull, 0ull}) {
        std::vector<MemberChunk> out;
        uint64_t v0 = 100;
        for (uint32_t s = 0; s < 5; ++s) {
            const size_t before = out.size();
            member_chunks_add(out, s, v0, v0 + sizes[s], chunk, tiles);
            CHECK(out.size() - before == per_tile[s] * tiles);
            size_t i = before;
            for (uint64_t t = 0; t < tiles; ++t) {   // tile-major: all chunks of tile 0, then of tile 1 ...
                uint64_t v = v0;
                for (uint64_t c = 0; c < per_tile[s]; ++c, ++i) {
                    const MemberChunk &m = out[i];
                    CHECK(m.first == v && m.species == s && m.tile == t && m.n >= 1u && m.n <= chunk);
                    CHECK(m.n == (c + 1 < per_tile[s] ? chunk : (uint32_t)(v0 + sizes[s] - v)));
                    v += m.n;
                }
                CHECK(v == v0 + sizes[s]);
            }
            v0 += sizes[s];
        }
        if (tiles == 0) CHECK(out.empty());
    }
    // appending keeps what is there, and a species may have tiles where its neighbour has none
    std::vector<MemberChunk> out;
    member_chunks_add(out, 0, 0, 10, 2048, 2);
    member_chunks_add(out, 1, 10, 30, 2048, 0);
    member_chunks_add(out, 2, 30, 2079, 2048, 1);
    CHECK(out.size() == 4 && out[1].first == 0u && out[1].n == 10u && out[1].tile == 1u && out[2].first == 30u && out[2].n == 2048u && out[3].first == 2078u && out[3].n == 1u && out[3].species == 2u);
}

int main() {
    routes();
    near_miss();
    filing();
    chunks();
    std::printf("member_plan_check: ok\n");
    return 0;
}
