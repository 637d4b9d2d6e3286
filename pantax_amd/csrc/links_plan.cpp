// links_plan.cpp -- the host helpers of the contract of pantax_hip_strain_links (links_plan.hpp).  Nothing here touches the device.
#include "links_plan.hpp"
#include <algorithm>
#include <vector>
#include "../../include/pantax_hip.h"

extern "C" {

int pantax_hip_link_crossings(uint64_t n, const uint64_t *masks, const uint8_t *known, uint32_t K, uint64_t *out) {
    if (!masks || !out || n == 0 || (n > 1 && !known)) return PANTAX_HIP_E_INVALID;
    if (K > ptx::LINKS_MAX_LIST) return PANTAX_HIP_E_INVALID;
    const uint64_t all = K == 64 ? ~0ull : (1ull << K) - 1ull;
    uint64_t cnt[ptx::LNK_N_SPECIES] = {};
    for (uint64_t i = 0; i + 1 < n; ++i)
        ++cnt[known[i] ? ptx::LNK_KNOWN : ptx::link_unknown_class(masks[i] & all, masks[i + 1] & all)];
    out[0] = cnt[ptx::LNK_KNOWN]; out[1] = cnt[ptx::LNK_SKIP]; out[2] = cnt[ptx::LNK_SWITCH]; out[3] = cnt[ptx::LNK_FOREIGN];
    return 0;
}

int pantax_hip_link_top(uint64_t n, const uint64_t *flank, const uint64_t *start, uint64_t top, uint64_t *idx_out, uint64_t *n_out) {
    if (!idx_out || !n_out || (n && (!flank || !start))) return PANTAX_HIP_E_INVALID;
    std::vector<uint64_t> ord(n);
    for (uint64_t i = 0; i < n; ++i) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) {
        if (flank[a] != flank[b]) return flank[a] > flank[b];
        return start[a] != start[b] ? start[a] < start[b] : a < b;
    });
    if (top && ord.size() > top) ord.resize((size_t)top);
    std::copy(ord.begin(), ord.end(), idx_out);
    *n_out = ord.size();
    return 0;
}

}  // extern "C"
