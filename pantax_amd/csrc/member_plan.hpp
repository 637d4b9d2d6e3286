// member_plan.hpp -- "which of the chosen haplotypes of this species walk node v?", the question of the six strain reports (read strains, read support,
// node evidence, depth, near miss, model fit), of the db's pair sums (hap pairs) and of the own-node windows of the replication index (growth: eight users), decided once on the host as pure functions of plain values:
//   route 0 -- nothing chosen;
//   route 1 -- a species of <= 64 haplotypes whose node -> haplotype words were built at upload (Db::d_node_haps), the call's *_route option not "walk":
//              word(v) = node_haps[v] & bits, bit = haplotype index; no array of its own;
//   route 2 -- every other species: ceil(K / 64) words per node over the K chosen haplotypes only, bit = position in the chosen list (WalkMasks, member_device.hpp).
// The launchers of the eight users follow it; nothing else decodes a *_route option, spells the route predicate or sizes a node's words.  Standard
// headers only: tests/native/member_plan_check.cpp compiles this with the host compiler alone; MemberRow is also what the kernels read.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace ptx {

constexpr uint32_t MEMBER_NO_ENTRY = 0xFFFFFFFFu;   // a position of the per-bit arrays that stands for no chosen haplotype
// the species row the kernels read; a stage's own row embeds it and adds what is its own
struct MemberRow {
    unsigned long long bits;   // route 1: bit j = haplotype j is chosen
    uint64_t mask_base;        // route 2: first word of the species' node masks in the arena (the caller's, from WalkMasks::add_species)
    uint32_t node_base;        // first global node index of the species
    uint32_t route;            // 0, 1, 2 as above
    uint32_t nw;               // mask words per node (route 1: 1; route 0: 0)
    uint32_t K;                // chosen haplotypes
};
template <class T> constexpr T member_words(T K) { return (K + 63) / 64; }   // words that hold K bits
// route 1 is open: `route_opt` is the call's read_strain_route / evidence_route / depth_route / near_miss_route / hap_pairs_route / fit_route / growth_route (any value but "walk":
// the default)
bool member_by_node(bool nh_built, const std::string &route_opt);
unsigned long long member_bits(const uint32_t *haps, uint64_t K);   // bit haps[k] for every k (haplotype indices < 64)
// the row of a species of `nh` haplotypes of which haps[0 .. K) are chosen; mask_base is left 0
MemberRow member_row(bool by_node, uint64_t nh, uint32_t node_base, const uint32_t *haps, uint64_t K);

// Bit -> entry filing: per_bit(bit, k) for the k-th chosen haplotype, which sits at bit haps[k] on route 1 and at bit first + k on route 2 (`first`: the bits
// of the row ahead of the list).  The per-bit arrays of the read passes, of node evidence and of the model fit hold H + C + 1 entries, a species' bits from member_bit_base on.
template <class PerBit> inline void member_file_bits(uint32_t route, const uint32_t *haps, uint64_t K, uint64_t first, PerBit &&per_bit) {
    for (uint64_t k = 0; k < K; ++k) per_bit(route == 1u ? (uint64_t)haps[k] : first + k, k);
}
inline uint32_t member_bit_base(uint32_t route, uint64_t hap_off_s, uint64_t H, uint64_t entry_off_s) { return (uint32_t)(route == 1u ? hap_off_s : route == 2u ? H + entry_off_s : 0); }
// Near miss: the row is over the LIST Sel ++ Cand (K + J entries).  Route 2: Sel ends at bit K, in the middle of word K / 64, which then serves both sets;
// a node's candidate words are w0 .. w0 + cwn - 1 and candidate i is bit cand0 + i counted from word w0.  Route 1: one word, bit = haplotype index.
struct NearMissLayout { uint32_t nw = 0, w0 = 0, cwn = 0, cand0 = 0; };
NearMissLayout near_miss_layout(uint64_t K, uint64_t J, uint32_t route);
// The nodes [node_begin, node_end) of species s cut into chunks of `chunk` nodes, once per tile, tile-major; appended to `out` (hap pairs: a tile is a
// block pair of mask words, hap_pairs_plan.hpp)
struct MemberChunk { uint32_t first, n, species, tile; };   // global nodes [first, first + n), n <= chunk
void member_chunks_add(std::vector<MemberChunk> &out, uint32_t s, uint64_t node_begin, uint64_t node_end, uint32_t chunk, uint64_t tiles);

}  // namespace ptx
