// bootstrap_weight.hpp -- the weight of a row in a bootstrap replicate (pantax_hip_strain_bootstrap; include/pantax_hip.h "Bootstrap of the strain fit"),
// the ONE definition the weight kernel (stage_bootstrap.hip) and the host helper pantax_hip_bootstrap_weight (bootstrap_plan.cpp) both compile, as
// depth_bin is.  Plain integer arithmetic: the same bits on either side.  Standard headers only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTX_BOOT_HD __host__ __device__
#else
#define PTX_BOOT_HD
#endif

namespace ptx {

constexpr int BOOT_W_MAX = 16;   // the cap of a weight
// T[j] = floor(2^64 * sum_{i <= j} e^-1 / i!), j = 0 .. 15: the Poisson(1) distribution function in 64-bit fixed point.  Computed with Python's decimal at
// 80 significant digits (e^-1 = 1 / Decimal(1).exp(), the partial sums kept as Decimal, times 2^64, ROUND_FLOOR); tests/bootstrap_ref.py recomputes
// them that way and tests/test_bootstrap_ref.py compares the weights.  1 - T[15] / 2^64 = 1.9e-14: the mass the cap puts on 16.
PTX_BOOT_HD inline uint32_t boot_weight_of(uint64_t r) {
    constexpr uint64_t T[BOOT_W_MAX] = {
        0x5E2D58D8B3BCDF1Aull, 0xBC5AB1B16779BE35ull, 0xEB715E1DC1582DC2ull, 0xFB23979734A252F1ull, 0xFF1025F59174DC3Dull, 0xFFD90F3BA4055E19ull,
        0xFFFA8B71FC72C913ull, 0xFFFF540C0914B3C9ull, 0xFFFFED1F4AA8F120ull, 0xFFFFFE216E641462ull, 0xFFFFFFD4D85D3183ull, 0xFFFFFFFC6DA262B4ull,
        0xFFFFFFFFBA12D178ull, 0xFFFFFFFFFB07C64Cull, 0xFFFFFFFFFFAB8EA5ull, 0xFFFFFFFFFFFABE22ull};
    uint32_t w = 0;
    for (int j = 0; j < BOOT_W_MAX; ++j) w += r >= T[j] ? 1u : 0u;
    return w;
}
PTX_BOOT_HD inline uint64_t boot_sm(uint64_t x) {   // splitmix64's output function
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the part of the hash that is the same for every row of a species: sm(seed ^ sm(sp_key))
PTX_BOOT_HD inline uint64_t boot_species_hash(uint64_t seed, uint64_t sp_key) { return boot_sm(seed ^ boot_sm(sp_key)); }
// w of row v_local in replicate b from the species' hash; replicate 0 is the plain refit
PTX_BOOT_HD inline uint32_t boot_weight_hashed(uint64_t species_hash, uint64_t b, uint64_t v_local) {
    if (b == 0) return 1u;
    return boot_weight_of(boot_sm(species_hash + (b << 40) + v_local));
}

}  // namespace ptx
