// segments_plan.cpp -- the host decisions of pantax_hip_strain_segments and the host helper of its contract (segments_plan.hpp).  Nothing here touches the device.
#include "segments_plan.hpp"
#include <algorithm>
#include "../../include/pantax_hip.h"

namespace ptx {

namespace {
// a run that is still open at a tile border
struct OpenRun { bool have = false; uint32_t cls = 0; uint64_t step = 0, start = 0, len = 0, bases = 0, n_steps = 0; };
}  // namespace

void segments_plan(uint64_t C, const uint64_t *tile_first, const uint32_t *tile_steps, const SegTileSum *sums, uint64_t min_len, uint64_t *seg_off,
                   uint64_t *hap_len, uint64_t *n_runs, uint64_t *run_len, uint64_t *run_max, SegPlan &plan) {
    plan.place.assign(tile_first[C], SegTilePlace{0, 0, 0});
    plan.border.clear();
    uint64_t slot = 0;
    seg_off[0] = 0;
    for (uint64_t c = 0; c < C; ++c) {
        for (int k = 0; k < 2; ++k) n_runs[2 * c + k] = run_len[2 * c + k] = run_max[2 * c + k] = 0;
        const auto count = [&](uint32_t cls, uint64_t n, uint64_t len, uint64_t longest) {
            n_runs[2 * c + cls - 1] += n; run_len[2 * c + cls - 1] += len; run_max[2 * c + cls - 1] = std::max(run_max[2 * c + cls - 1], longest);
        };
        OpenRun cur;
        const auto close = [&]() {
            if (cur.have && (cur.cls == SEG_GAP || cur.cls == SEG_PEAK)) {
                count(cur.cls, 1, cur.len, cur.len);
                if (cur.len >= min_len) plan.border.push_back(SegBorder{slot++, cur.step, cur.start, cur.len, cur.bases, (uint32_t)cur.n_steps, (uint8_t)cur.cls});
            }
            cur.have = false;
        };
        const auto open = [&](const SegPiece &p, uint64_t step, uint64_t start) {
            cur.have = true; cur.cls = p.cls; cur.step = step; cur.start = start; cur.len = p.len; cur.bases = p.bases; cur.n_steps = p.n_steps;
        };
        uint64_t base = 0, step0 = 0;
        for (uint64_t t = tile_first[c]; t < tile_first[c + 1]; ++t) {
            const SegTileSum &s = sums[t];
            if (cur.have && cur.cls == s.lead.cls) { cur.len += s.lead.len; cur.bases += s.lead.bases; cur.n_steps += s.lead.n_steps; }   // the run goes on over the border
            else { close(); open(s.lead, step0, base); }                                                                                 // a class change at the border ends it
            if (!s.whole) {
                close();   // the lead run ends inside the tile
                plan.place[t] = SegTilePlace{base, slot, step0};
                slot += s.n_keep;
                for (uint32_t k = 0; k < 2; ++k) if (s.n[k]) count(k + 1, s.n[k], s.len[k], s.max[k]);
                open(s.trail, step0 + tile_steps[t] - s.trail.n_steps, base + s.sum_len - s.trail.len);
            } else plan.place[t] = SegTilePlace{base, slot, step0};   // (no interior run: out0 is not used)
            base += s.sum_len;
            step0 += tile_steps[t];
        }
        close();
        hap_len[c] = base;
        seg_off[c + 1] = slot;
    }
}

}  // namespace ptx

extern "C" {

int pantax_hip_segment_chain(uint64_t n, const uint8_t *seg_class, const uint64_t *seg_start, const uint64_t *seg_len, const uint32_t *seg_n_steps,
                             const uint64_t *seg_bases, uint64_t bridge, uint64_t min_span, uint64_t *n_chains_out, uint8_t *chain_class, uint64_t *chain_first,
                             uint64_t *chain_last, uint64_t *chain_q) {
    if (!n_chains_out) return PANTAX_HIP_E_INVALID;
    if (n && (!seg_class || !seg_start || !seg_len || !seg_n_steps || !seg_bases || !chain_class || !chain_first || !chain_last || !chain_q)) return PANTAX_HIP_E_INVALID;
    for (uint64_t i = 0; i < n; ++i) {
        if (seg_class[i] != ptx::SEG_GAP && seg_class[i] != ptx::SEG_PEAK) return PANTAX_HIP_E_INVALID;
        if (seg_start[i] + seg_len[i] < seg_start[i]) return PANTAX_HIP_E_INVALID;                       // wraps
        if (i && seg_start[i] < seg_start[i - 1] + seg_len[i - 1]) return PANTAX_HIP_E_INVALID;          // not ascending, or overlapping
    }
    struct Chain { uint8_t cls; uint64_t first, last, q[PANTAX_HIP_SEGMENT_CHAIN_N]; };
    std::vector<Chain> chains;
    int64_t at[2] = {-1, -1};   // the open chain of either class
    for (uint64_t i = 0; i < n; ++i) {
        const int k = seg_class[i] - 1;
        const uint64_t end = seg_start[i] + seg_len[i];
        if (at[k] >= 0 && seg_start[i] - chains[at[k]].q[1] <= bridge) {
            Chain &ch = chains[at[k]];
            ch.last = i; ch.q[1] = end; ch.q[2] = end - ch.q[0]; ch.q[3] += seg_len[i]; ch.q[4] += 1; ch.q[5] += seg_n_steps[i]; ch.q[6] += seg_bases[i];
        } else {
            at[k] = (int64_t)chains.size();
            chains.push_back(Chain{seg_class[i], i, i, {seg_start[i], end, seg_len[i], seg_len[i], 1, seg_n_steps[i], seg_bases[i]}});
        }
    }
    // (a chain opens at its first member and members ascend: the chains stand in ascending start already)
    uint64_t m = 0;
    for (const Chain &ch : chains) {
        if (ch.q[2] < min_span) continue;
        chain_class[m] = ch.cls; chain_first[m] = ch.first; chain_last[m] = ch.last;
        for (int j = 0; j < PANTAX_HIP_SEGMENT_CHAIN_N; ++j) chain_q[PANTAX_HIP_SEGMENT_CHAIN_N * m + j] = ch.q[j];
        ++m;
    }
    *n_chains_out = m;
    return 0;
}

}  // extern "C"
