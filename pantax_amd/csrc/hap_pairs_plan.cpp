// hap_pairs_plan.cpp -- the host decisions of pantax_hip_db_hap_pairs (hap_pairs_plan.hpp).  Nothing here touches the device.
#include "hap_pairs_plan.hpp"
#include <algorithm>

namespace ptx {

uint32_t hap_pairs_offsets(uint32_t S, const uint64_t *sel_off, uint64_t *pair_off_out) {
    uint32_t bad = S;
    pair_off_out[0] = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = sel_off[s + 1] - sel_off[s];
        if (K > HAP_PAIRS_MAX_K && bad == S) bad = s;
        pair_off_out[s + 1] = pair_off_out[s] + K * K;
    }
    return bad;
}

uint32_t hap_pairs_chunk(uint32_t ka, uint32_t kb, int opt) {
    const uint64_t want = opt > 0 ? ((uint64_t)opt + 63) / 64 * 64 : std::max<uint64_t>(HAP_PAIRS_CHUNK_MIN, 32ull * ka * kb);
    return (uint32_t)std::min<uint64_t>(want, HAP_PAIRS_CHUNK_MAX);
}

uint32_t hap_pairs_cols(unsigned long long live_b) {
    if (!live_b) return 0;
    const uint32_t top = 63u - (uint32_t)__builtin_clzll(live_b);
    return top < 8 ? 8u : top < 16 ? 16u : top < 32 ? 32u : 64u;
}

void hap_pairs_mirror(uint64_t *block, uint64_t K, uint32_t cols) {
    for (uint64_t b = 64; b < K; ++b)
        for (uint64_t a = 0; a < b / 64 * 64; ++a)
            for (uint32_t q = 0; q < cols; ++q) block[(b * K + a) * cols + q] = block[(a * K + b) * cols + q];
}

}  // namespace ptx
