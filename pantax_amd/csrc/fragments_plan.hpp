// fragments_plan.hpp -- the host side of the fragment support (pantax_hip_fragment_mates, pantax_hip_strain_fragments; stage_fragments.hip) as pure
// functions of plain values: the fragment key of a read id (pantax_hip_fragment_key: the stem's id hash and the mate tag) and the order of the classes
// in the outputs.  pantax_hip.h and standard headers only: tests/native/fragments_plan_check.cpp compiles this with the host compiler alone.
#pragma once
#include <cstdint>

namespace ptx {

constexpr uint32_t FRAG_MAX_LIST = 64;   // K_s of a served species: C(r) is one u64
// the species classes of pantax_hip_strain_fragments, in the order of species_out
enum FragSpeciesClass { FRG_COUNTED, FRG_PAIRED, FRG_CONCORDANT, FRG_DISCORDANT, FRG_HALF, FRG_UNEXPLAINED, FRG_SINGLE, FRG_MULTI, FRG_ELSEWHERE, FRG_N_CLASSES };
// the sums of a candidate entry, in the order of hap_out
enum FragHapClass { FRG_COMPATIBLE, FRG_UNIQUE, FRG_UNIQUE_BY_PAIR, FRG_ASSIGNED, FRG_N_HAP };

// the id hash of both GAF tokenizers (pantax_hip_gaf_ids): FNV-1a-64 over the bytes, then the avalanche
inline uint64_t fragment_id_hash(const char *p, uint64_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint64_t i = 0; i < n; ++i) { h ^= (unsigned char)p[i]; h *= 0x100000001b3ull; }
    h ^= h >> 32; h *= 0xd6e8feb86659fd93ull; h ^= h >> 32;
    return h;
}
// stem and tag of an id: "<stem>/1" and "<stem>/2" (a stem of at least one byte) carry tag 1 and 2; every other id is its own stem, tag 0
inline void fragment_key(const char *id, uint64_t len, uint64_t &key, uint8_t &tag) {
    const bool suffixed = len >= 3 && id[len - 2] == '/' && (id[len - 1] == '1' || id[len - 1] == '2');
    tag = suffixed ? (uint8_t)(id[len - 1] - '0') : (uint8_t)0;
    key = fragment_id_hash(id, suffixed ? len - 2 : len);
}

}  // namespace ptx
