// mosaic_plan.cpp -- the host decisions of pantax_hip_strain_mosaic and the host helpers of its contract (mosaic_plan.hpp).  Nothing here touches the device.
#include "mosaic_plan.hpp"
#include <algorithm>
#include <numeric>
#include "../../include/pantax_hip.h"

namespace ptx {

void mosaic_junctions(std::vector<MosaicBreak> &recs, std::vector<MosaicBreak> &distinct, std::vector<uint64_t> &count) {
    std::sort(recs.begin(), recs.end());
    distinct.clear();
    count.clear();
    for (const MosaicBreak &r : recs) {
        if (!distinct.empty() && distinct.back() == r) ++count.back();
        else { distinct.push_back(r); count.push_back(1); }
    }
}

}  // namespace ptx

extern "C" {

int pantax_hip_mosaic_walk(uint64_t n, const uint64_t *masks, uint32_t K, const double *w, const uint32_t *hap, uint64_t *seg_end_out, uint32_t *seg_pos_out,
                           uint64_t cap, uint64_t *k_out, uint64_t *foreign_steps_out) {
    if (!k_out || !foreign_steps_out || !w || !hap || (n && !masks) || (cap && (!seg_end_out || !seg_pos_out))) return PANTAX_HIP_E_INVALID;
    if (K == 0 || K > ptx::MOSAIC_MAX_K) return PANTAX_HIP_E_INVALID;
    // the positions in ascending haplotype index: the order of the argmax (the first of equal weights wins; a set whose weights are all NaN or -inf keeps
    // its smallest haplotype index, as on the device)
    uint32_t order[ptx::MOSAIC_MAX_K];
    std::iota(order, order + K, 0u);
    std::sort(order, order + K, [&](uint32_t a, uint32_t b) { return hap[a] < hap[b]; });
    for (uint32_t i = 1; i < K; ++i)
        if (hap[order[i]] == hap[order[i - 1]]) return PANTAX_HIP_E_INVALID;
    const uint64_t all = K == 64 ? ~0ull : (1ull << K) - 1ull;
    uint64_t foreign = 0;
    for (uint64_t i = 0; i < n; ++i) foreign += (masks[i] & all) == 0 ? 1 : 0;
    *foreign_steps_out = foreign;
    *k_out = 0;
    if (foreign || n == 0) return 0;
    const auto assigned = [&](uint64_t a) {
        uint32_t best = K;
        double bw = 0.0;
        for (uint32_t i = 0; i < K; ++i) {
            const uint32_t p = order[i];
            if (!((a >> p) & 1ull)) continue;
            if (best == K) { best = p; bw = -__builtin_inf(); }
            if (w[p] > bw) { bw = w[p]; best = p; }
        }
        return best;
    };
    uint64_t k = 0, run = masks[0] & all;
    const auto close = [&](uint64_t end) {
        if (k < cap) { seg_end_out[k] = end; seg_pos_out[k] = assigned(run); }
        ++k;
    };
    for (uint64_t i = 1; i < n; ++i) {
        const uint64_t m = masks[i] & all;
        if ((run & m) == 0) { close(i); run = m; }   // step i would empty the intersection: it opens the next segment
        else run &= m;
    }
    close(n);
    *k_out = k;
    return k > cap ? PANTAX_HIP_E_LIMIT : 0;
}

int pantax_hip_mosaic_top(uint64_t n, const uint32_t *node_a, const uint32_t *node_b, const uint64_t *count, uint64_t top, uint64_t *idx_out, uint64_t *n_out) {
    if (!n_out || (n && (!node_a || !node_b || !count)) || (n && top && !idx_out)) return PANTAX_HIP_E_INVALID;
    std::vector<uint64_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0ull);
    const auto before = [&](uint64_t x, uint64_t y) {
        if (count[x] != count[y]) return count[x] > count[y];
        if (node_a[x] != node_a[y]) return node_a[x] < node_a[y];
        if (node_b[x] != node_b[y]) return node_b[x] < node_b[y];
        return x < y;
    };
    const uint64_t m = std::min(n, top);
    std::partial_sort(idx.begin(), idx.begin() + m, idx.end(), before);
    for (uint64_t i = 0; i < m; ++i) idx_out[i] = idx[i];
    *n_out = m;
    return 0;
}

}  // extern "C"
