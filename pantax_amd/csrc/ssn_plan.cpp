// ssn_plan.cpp -- geometry and workspace layout of the node-order row sort (ssn_plan.hpp).  Nothing here touches the device.
#include "ssn_plan.hpp"
#include <algorithm>
#include <cstring>

namespace ptx {

SsnPlan ssn_plan(uint32_t S, uint64_t seg_bound, uint64_t V) {
    SsnPlan p;
    // about SN_TARGET_WGS partition workgroups over all segments: each walks `per` tiles of its segment behind one LDS histogram
    const uint64_t nt = std::max<uint64_t>(1, (seg_bound + SN_TILE - 1) / SN_TILE);   // tiles of the largest segment
    const uint64_t target = SN_TARGET_WGS;
    uint64_t per = (nt * S + target - 1) / target;
    if (per < 1) per = 1;
    if (per > nt) per = nt;
    p.per = (uint32_t)per;
    p.G = (uint32_t)((nt + per - 1) / per);
    p.tie_grid = (uint32_t)((seg_bound + SN_TIE_ROWS - 1) / SN_TIE_ROWS);

    const size_t SG = (size_t)S * p.G;
    size_t at = 0;
    auto take = [&at](size_t words, bool even = false) {
        if (even) at += at & 1u;
        const size_t off = at;
        at += words;
        return off;
    };
    p.ws = take((size_t)S * SN_WS_WORDS);
    p.cntm = take(SG * SN_NBUCKET);
    p.stage_cnt = take(SG);
    p.c0p = take(2 * SG, true);
    p.seg_n = take(S);
    p.seg_out = take((size_t)S + 1);
    p.sub_k = take((size_t)SN_NWH * S);
    p.ids = take((size_t)((V + 1) / 2));
    p.npart = take(SN_NODE_PARTIAL_WORDS * SG, true);
    p.total_words = at;
    return p;
}

int ssn_keys_all(const char *option, bool has_patterns) {
    if (!option || !*option || std::strcmp(option, "auto") == 0) return has_patterns ? 0 : 1;
    if (std::strcmp(option, "all") == 0) return 1;
    if (std::strcmp(option, "needed") == 0) return has_patterns ? 0 : -1;
    return -1;
}

int ssn_node_bits(const char *option, int words) {
    if (words < 0 || words > 2) return -1;
    if (!option || !*option || std::strcmp(option, "range") == 0) return words ? words : SSN_NODE_BITS_WORDS;
    if (std::strcmp(option, "gather") == 0) return 0;
    return -1;
}

bool ssn_ties_async(int option, bool clocked, bool on_side_stream, bool have_side_stream) {
    if (clocked || on_side_stream || !have_side_stream) return false;
    return option > 0 || (option < 0 && SSN_TIES_ASYNC_AUTO);
}

}  // namespace ptx
