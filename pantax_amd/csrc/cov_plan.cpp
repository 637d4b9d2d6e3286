// cov_plan.cpp -- the coverage pass's host-side decisions (cov_plan.hpp).  Nothing here touches the device.
#include "cov_plan.hpp"
#include <algorithm>
#include <utility>

namespace ptx {

CovFastShape cov_fast_shape(int code) {
    switch (code) {
        case 182: return {1, 8, 2048};
        case 242: return {2, 4, 2048};
        case 282: return {2, 8, 2048};
        case 283: return {2, 8, 3072};
        case 284: return {2, 8, 4096};
        case 243: return {2, 4, 3072};
        case 2823: return {2, 8, 2304};
        case 2825: return {2, 8, 2560};
        case 2423: return {2, 4, 2304};
        case 2425: return {2, 4, 2560};
        case 1823: return {1, 8, 2304};
        case 4423: return {4, 4, 2304};
        case 442: return {4, 4, 2048};
        case 443: return {4, 4, 3072};
        default: return {2, 4, 2048};
    }
}

CovLongShape cov_long_shape(int code) {
    const bool five = code >= 10000;
    const int su = five ? code / 10000 : code / 1000, sg = five ? code / 100 % 100 : code / 100 % 10, sw = code / 10 % 10, sb = code % 10;
    CovLongShape s{2, 3072, (uint32_t)std::max(1, sg) * 8u, (uint32_t)sb * 256u};
    switch (su * 10 + sw) {
        case 12: s.u = 1; s.win = 2048; break;
        case 13: s.u = 1; s.win = 3072; break;
        case 14: s.u = 1; s.win = 4096; break;
        case 22: s.u = 2; s.win = 2048; break;
        case 24: s.u = 2; s.win = 4096; break;
        default: break;
    }
    return s;
}

CovStepShape cov_step_shape(int code) {
    switch (code) {
        case 22: return {2, 2};
        case 21: return {2, 1};
        case 41: return {4, 1};
        case 42: return {4, 2};
        case 18: return {1, 8};
        default: return {1, 4};   // (14 among them)
    }
}

CovPlan cov_plan(uint64_t T_pad, uint32_t n_long, uint32_t n_slots, uint32_t n_items, uint64_t R, bool cov_general, const std::string &cov_long,
                 int covf_shape, int covl_shape, int cov_shape, int cov_xcd) {
    CovPlan p;
    p.only_long = !cov_general;
    p.xcd_map = (uint32_t)cov_xcd;
    p.fast = cov_fast_shape(covf_shape > 0 ? covf_shape : T_pad >= (1ull << 28) ? COVF_SHAPE_DEFAULT_BIG : COVF_SHAPE_DEFAULT);
    p.lng = cov_long_shape(covl_shape > 0 ? covl_shape : COVL_SHAPE_DEFAULT);
    p.step = cov_step_shape(cov_shape > 0 ? cov_shape : T_pad >= (1ull << 25) ? COVS_SHAPE_DEFAULT_BIG : COVS_SHAPE_DEFAULT);
    if (R == 0 || T_pad == 0) return p;
    // walks of <= 64 steps: the short-read kernel; skipped when every walk is longer
    p.run_fast = n_long < n_slots && n_items && !cov_general;
    // groups that hold steps of longer walks (cov_general: every group): the select-only body over plain cuts of the stream, or round 5's kernel
    const bool longer = n_long || cov_general, by_step = cov_long == "step";
    p.run_long = longer && !by_step;
    p.run_step = longer && by_step;
    return p;
}

CovItemSel cov_item_select(const std::vector<uint32_t> &item_block, int blk_shift, const std::vector<int64_t> &range_start, const std::vector<int64_t> &range_end) {
    const uint32_t n_items = (uint32_t)item_block.size();
    std::vector<std::pair<uint32_t, uint32_t>> rg;       // item ranges of the species, then merged
    for (size_t s = 0; s < range_start.size() && s < range_end.size(); ++s) {
        const uint32_t b_lo = (uint32_t)std::max<int64_t>(range_start[s], 0) >> blk_shift;
        const uint32_t b_hi = (uint32_t)std::min<int64_t>(std::max<int64_t>(range_end[s], 0), 0xFFFFFFFFll) >> blk_shift;
        uint32_t i_lo = (uint32_t)(std::lower_bound(item_block.begin(), item_block.end(), b_lo) - item_block.begin());
        // An item carries the block of the FIRST read of its groups; the last group of the item in front may run on into this block (a group is
        // 64 steps of consecutive reads, and where reads are sparse a layout unit spans several blocks): its reads of block b_lo are this
        // species' too.  One item back is enough -- the next group already begins with a read of b_lo and opens an item of that block.
        if (i_lo > 0) --i_lo;
        const uint32_t i_hi = (uint32_t)(std::upper_bound(item_block.begin(), item_block.end(), b_hi) - item_block.begin());
        if (i_hi > i_lo) rg.emplace_back(i_lo, i_hi);
    }
    std::sort(rg.begin(), rg.end());
    CovItemSel r;
    uint32_t done = 0;
    for (const auto &g : rg) for (uint32_t i = std::max(g.first, done); i < g.second; ++i) { r.sel.push_back(i); done = i + 1; }
    if (r.sel.size() + r.sel.size() / 8 < n_items) {     // (worth the indirection)
        r.n_sel = (uint32_t)r.sel.size();
        r.on = true;
    } else {
        r.n_sel = n_items;
        r.sel.clear();
    }
    return r;
}

CovArenaLayout cov_arena_layout(uint64_t V, uint64_t U, uint64_t L) {
    CovArenaLayout a;
    a.words = (L + 31) / 32 + 1;
    a.fwords = (V + 4096 + 63) / 32 + 2;     // padded by the largest LDS window
    a.n_trio = U ? U : 1;
    a.off_trio = (size_t)(V * 8);
    a.off_abort = a.off_trio + (size_t)(a.n_trio * 8);
    a.off_bm = (a.off_abort + 8 + 15) & ~(size_t)15;   // (16-byte loads of the bit vector)
    a.off_full = a.off_bm + (size_t)(a.words * 4);
    a.total = a.off_full + (size_t)(a.fwords * 4);
    return a;
}

}  // namespace ptx
