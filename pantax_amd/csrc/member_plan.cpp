// member_plan.cpp -- the strain reports' membership decisions (member_plan.hpp).  Nothing here touches the device.
#include "member_plan.hpp"
#include <algorithm>

namespace ptx {

bool member_by_node(bool nh_built, const std::string &route_opt) { return nh_built && route_opt != "walk"; }

unsigned long long member_bits(const uint32_t *haps, uint64_t K) {
    unsigned long long bits = 0ull;
    for (uint64_t k = 0; k < K; ++k) bits |= 1ull << haps[k];
    return bits;
}

MemberRow member_row(bool by_node, uint64_t nh, uint32_t node_base, const uint32_t *haps, uint64_t K) {
    MemberRow r{0ull, 0ull, node_base, 0u, 0u, (uint32_t)K};
    if (K == 0) return r;
    if (by_node && nh <= 64) { r.route = 1; r.nw = 1; r.bits = member_bits(haps, K); }
    else { r.route = 2; r.nw = (uint32_t)member_words(K); }
    return r;
}

NearMissLayout near_miss_layout(uint64_t K, uint64_t J, uint32_t route) {
    NearMissLayout l;
    if (route == 1u) { l.nw = 1; l.cwn = J ? 1u : 0u; }
    else if (route == 2u) {
        l.nw = (uint32_t)member_words(K + J); l.w0 = (uint32_t)(K / 64); l.cand0 = (uint32_t)(K % 64);
        l.cwn = J ? (uint32_t)((K + J - 1) / 64) - l.w0 + 1u : 0u;
    }
    return l;
}

void member_chunks_add(std::vector<MemberChunk> &out, uint32_t s, uint64_t node_begin, uint64_t node_end, uint32_t chunk, uint64_t tiles) {
    for (uint64_t t = 0; t < tiles; ++t)
        for (uint64_t v = node_begin; v < node_end; v += chunk)
            out.push_back(MemberChunk{(uint32_t)v, (uint32_t)std::min<uint64_t>(chunk, node_end - v), s, (uint32_t)t});
}

}  // namespace ptx
