// depth_device.hpp -- the depth of a node and its histogram bin (include/pantax_hip.h, "per-strain depth distribution"), one source text for the
// kernel of stage_depth.hip and for the host helpers pantax_hip_depth_bin / _bin_range / _quantile (api_host.cpp).  Integers only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTX_DEPTH_HD __host__ __device__
#else
#define PTX_DEPTH_HD
#endif

namespace ptx {

constexpr uint32_t DEPTH_BINS = 96;    // = PANTAX_HIP_DEPTH_BINS
constexpr uint32_t DEPTH_EXACT = 32;   // bins 0 .. 31 hold one depth each

// d(v) = bases_per_node[v] / node_len[v] in u64 integer division, 0 for a node without bases of length
PTX_DEPTH_HD inline uint64_t node_depth(uint64_t bases, uint32_t len) {
    if (len == 0u) return 0ull;
    if ((bases >> 32) == 0ull) return (uint64_t)((uint32_t)bases / len);   // (the common case: a 32-bit division)
    return bases / (uint64_t)len;
}

// d < 32: the bin is d.  From 2^5 up four bins per octave: e = floor(log2 d), the two bits under the leading one pick the quarter; bin 95 also takes
// everything from 2^21 up.
PTX_DEPTH_HD inline uint32_t depth_bin(uint64_t d) {
    if (d < (uint64_t)DEPTH_EXACT) return (uint32_t)d;
    const uint32_t e = 63u - (uint32_t)__builtin_clzll((unsigned long long)d);   // >= 5
    const uint32_t b = DEPTH_EXACT + 4u * (e - 5u) + (uint32_t)((d >> (e - 2u)) & 3ull);
    return b < DEPTH_BINS - 1u ? b : DEPTH_BINS - 1u;
}

// the smallest depth of bin b (b < DEPTH_BINS, and b = DEPTH_BINS for the bound above bin 95 in the regular grid: 2^21)
PTX_DEPTH_HD inline uint64_t depth_bin_lo(uint32_t b) {
    if (b < DEPTH_EXACT) return (uint64_t)b;
    return (uint64_t)(4u + (b - DEPTH_EXACT) % 4u) << (3u + (b - DEPTH_EXACT) / 4u);
}

}  // namespace ptx
