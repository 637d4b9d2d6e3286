// hap_pairs_plan.hpp -- the host decisions of pantax_hip_db_hap_pairs and pantax_hip_strain_pair_evidence (stage_hap_pairs.hip) as pure functions of plain values: the sizing of pair_off, the
// block pairs of a species' mask words and their tile numbers, the nodes a wave takes per chunk, the columns a wave keeps in registers, the mirror of the
// lower triangle.  The work is C = B^T diag(Q) B over the 0/1 membership rows B of a species; its unit is a BLOCK PAIR (wa, wb), wa <= wb: the 64 haplotypes
// of mask word wa against the 64 of word wb.  A species of nw words has nw (nw + 1) / 2 of them, numbered row-major over the upper triangle; that number is
// the `tile` of member_chunks_add (member_plan.hpp).  Standard headers only: tests/native/hap_pairs_plan_check.cpp compiles this with the host compiler alone.
#pragma once
#include <cstdint>

namespace ptx {

constexpr uint64_t HAP_PAIRS_MAX_K = 256;      // selected haplotypes of a species the call serves: the four words of the wide LAD path and of the near-miss candidates
constexpr uint32_t HAP_PAIRS_CHUNK_MIN = 1024; // nodes per chunk (one wave), smallest and largest: a wave's packed counters hold { n_nodes < 2^16, len < 2^48 }
constexpr uint32_t HAP_PAIRS_CHUNK_MAX = 32768;

// pair_off[s + 1] = pair_off[s] + K_s^2 from sel_off [S + 1].  Returns S when every K_s <= HAP_PAIRS_MAX_K, else the first species beyond it (pair_off_out
// is written whole either way).  Decreasing offsets are the caller's to refuse before.
uint32_t hap_pairs_offsets(uint32_t S, const uint64_t *sel_off, uint64_t *pair_off_out);

struct HapPairsTile { uint32_t wa, wb; };      // the block pair: mask words of the rows and of the columns, wa <= wb
constexpr uint32_t hap_pairs_tiles(uint32_t nw) { return nw * (nw + 1u) / 2u; }
// tile t of a species of nw words: (0,0) (0,1) .. (0,nw-1) (1,1) .. (nw-1,nw-1).  The same expression runs in the kernel.
#if defined(__HIP__)
__host__ __device__
#endif
inline HapPairsTile hap_pairs_tile(uint32_t nw, uint32_t t) {
    uint32_t wa = 0;
    while (t >= nw - wa) { t -= nw - wa; ++wa; }
    return HapPairsTile{wa, wa + t};
}
// bits of word w that stand for a selected haplotype on route 2 (K selected: bit = position in the list); route 1 has the row's bits
#if defined(__HIP__)
__host__ __device__
#endif
inline unsigned long long hap_pairs_live(uint64_t K, uint32_t w) {
    const uint64_t lo = 64ull * w;
    return K <= lo ? 0ull : (K - lo >= 64 ? ~0ull : (1ull << (K - lo)) - 1ull);
}
// Nodes per chunk of a block pair with ka live rows and kb live columns.  A chunk ends in one flush of up to 2 ka kb 64-bit atomics, against 12 to 20 bytes
// loaded per node: 32 ka kb nodes keep the flush at one atomic per 16 nodes (half a byte of atomics per byte loaded at the most); never under 1024 nodes
// (the evidence pass's chunk: small species still spread over the CUs), never over 32768 (the packed counters).  `opt` > 0 (option hap_pairs_chunk;
// tests): that many nodes, rounded up to whole waves of 64 and cut to the same maximum.
uint32_t hap_pairs_chunk(uint32_t ka, uint32_t kb, int opt);
// Columns a wave keeps in registers for a block pair whose live column bits are `live_b`: the smallest of 8, 16, 32, 64 above its highest bit (0: none)
uint32_t hap_pairs_cols(unsigned long long live_b);
// The K x K block of a species as the kernel leaves it (entries [a][b] of the block pairs wa <= wb; a diagonal block pair is whole): entries of `cols`
// u64, { n, len } of pantax_hip_db_hap_pairs or { n, len, covered, bases } of pantax_hip_strain_pair_evidence.  Fills [b][a] = [a][b] for a / 64 < b / 64.
void hap_pairs_mirror(uint64_t *block /*[K][K][cols]*/, uint64_t K, uint32_t cols = 2);

}  // namespace ptx
