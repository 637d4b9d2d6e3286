// rescue_plan.cpp -- the host decisions of pantax_hip_strain_read_rescue and the host helpers of its contract (rescue_plan.hpp).  Nothing here touches the
// device.
#include "rescue_plan.hpp"
#include <algorithm>
#include "../../include/pantax_hip.h"

namespace ptx {

std::vector<uint32_t> rescue_candidates(uint64_t K, uint32_t n_cand, const uint32_t *cand_hap, const uint32_t *ranked, uint32_t n_ranked) {
    std::vector<uint32_t> out;
    if (K >= RESCUE_MAX_LIST || n_cand == 0) return out;
    std::vector<uint8_t> taken(n_cand, 0);
    for (uint32_t i = 0; i < n_ranked; ++i)
        if (ranked[i] < n_cand && !taken[ranked[i]]) { taken[ranked[i]] = 1; out.push_back(ranked[i]); }
    std::vector<uint32_t> rest;
    for (uint32_t c = 0; c < n_cand; ++c)
        if (!taken[c]) rest.push_back(c);
    std::sort(rest.begin(), rest.end(), [&](uint32_t a, uint32_t b) { return cand_hap[a] != cand_hap[b] ? cand_hap[a] < cand_hap[b] : a < b; });
    out.insert(out.end(), rest.begin(), rest.end());
    if (out.size() > RESCUE_MAX_LIST - K) out.resize((size_t)(RESCUE_MAX_LIST - K));
    return out;
}

}  // namespace ptx

extern "C" {

int pantax_hip_rescue_walk(uint64_t n, const uint64_t *sel_masks, const uint64_t *cand_masks, uint32_t K, uint32_t J, uint32_t *class_out, uint64_t *d_out,
                           uint64_t *steps_out) {
    if (!sel_masks || !cand_masks || !class_out || !d_out || !steps_out || n == 0) return PANTAX_HIP_E_INVALID;
    if ((uint64_t)K + J > ptx::RESCUE_MAX_LIST) return PANTAX_HIP_E_INVALID;
    const uint64_t sel_all = K == 64 ? ~0ull : (1ull << K) - 1ull, cand_all = J == 64 ? ~0ull : (1ull << J) - 1ull;
    uint64_t c = sel_all, d = cand_all, foreign = 0, novel = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t m = sel_masks[i] & sel_all, x = cand_masks[i] & cand_all;
        c &= m; d &= x;
        if (m == 0) { ++foreign; if (x == 0) ++novel; }
    }
    steps_out[0] = foreign; steps_out[1] = foreign - novel; steps_out[2] = novel;
    *d_out = d;
    if (c) *class_out = PANTAX_HIP_RESCUE_COMPATIBLE;
    else if (foreign) *class_out = d ? PANTAX_HIP_RESCUE_FOREIGN_RESCUED : novel ? PANTAX_HIP_RESCUE_FOREIGN_NOVEL : PANTAX_HIP_RESCUE_FOREIGN_PATCHWORK;
    else *class_out = d ? PANTAX_HIP_RESCUE_MOSAIC_RESCUED : PANTAX_HIP_RESCUE_MOSAIC_UNRESCUED;
    return 0;
}

int pantax_hip_rescue_rank(uint32_t n_cand, const uint32_t *cand_hap, const uint64_t *cand_out, uint32_t top, uint32_t *rank_out, uint32_t *n_out) {
    if (!cand_hap || !cand_out || !rank_out || !n_out) return PANTAX_HIP_E_INVALID;
    std::vector<uint32_t> ord;
    for (uint32_t c = 0; c < n_cand; ++c)
        if (cand_out[9 * (size_t)c]) ord.push_back(c);   // rescued.n_reads > 0
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t *qa = cand_out + 9 * (size_t)a, *qb = cand_out + 9 * (size_t)b;   // rescued {n_reads, n_steps, span}
        if (qa[2] != qb[2]) return qa[2] > qb[2];
        if (qa[0] != qb[0]) return qa[0] > qb[0];
        return cand_hap[a] != cand_hap[b] ? cand_hap[a] < cand_hap[b] : a < b;
    });
    if (top && ord.size() > top) ord.resize(top);
    std::copy(ord.begin(), ord.end(), rank_out);
    *n_out = (uint32_t)ord.size();
    return 0;
}

}  // extern "C"
