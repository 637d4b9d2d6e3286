// dropout_plan.hpp -- the host decisions of pantax_hip_strain_dropout (stage_dropout.hip) as pure functions of plain values: where an entry and its x
// block sit in the outputs, how many rounds of leave-one-out LPs go through the solver at once, the default of the cap on the replicated patterns in
// flight, and how a species' sorted rows are cut into the slices of the objective pass.  The host helper of the contract
// (pantax_hip_dropout_substitute) is defined in dropout_plan.cpp beside them.  pantax_hip.h and standard headers only:
// tests/native/dropout_plan_check.cpp compiles this with the host compiler alone.
#pragma once
#include <cstdint>
#include <string>

namespace ptx {

// Species s of K_s selected haplotypes has E_s = K_s + 1 entries (0: the plain refit; k + 1: column k pinned to zero).  Entry (s, e) is
// q = sel_off[s] + s + e of Q = C + S, and the species' x block of E_s x K_s doubles (entry-major) starts at x_off[s] = sum over t < s of E_t K_t.
inline uint64_t dropout_entry(uint64_t sel_off_s, uint64_t s, uint64_t e) { return sel_off_s + s + e; }
// x_off [S + 1] from sel_off [S + 1]; false when the total passes 2^64 - 1 (x_off is then unspecified)
bool dropout_x_offsets(uint64_t S, const uint64_t *sel_off, uint64_t *x_off);

// A round e = 0 .. k_max holds every species once over ONE copy of the base pattern tables: P patterns and the closing slot, and S entries and the
// closing one.  Bytes of device scratch a replicated pattern costs: mask 8, start 4, the solver's scratch 3 x 8 + 5 x 4.
constexpr uint64_t DROP_BYTES_PER_PATTERN = 8 + 4 + 3 * 8 + 5 * 4;
constexpr uint64_t DROP_PATTERNS_HARD_MAX = 0xFFFFFFFFull - 1;   // the solver's pattern and entry indices are 32-bit
// The default of option dropout_patterns_max: a quarter of what is free on the device when the call begins, in patterns, at most the hard bound
uint64_t dropout_default_cap(uint64_t free_bytes);

struct DropoutPlan {
    uint32_t per_chunk = 0;       // rounds per chunk, >= 1 (the last chunk may hold fewer)
    uint32_t n_chunks = 0;        // ceil(rounds / per_chunk)
    uint64_t chunk_patterns = 0;  // per_chunk * (P + 1): what the replicated pattern tables hold
    uint64_t chunk_entries = 0;   // per_chunk * (S + 1)
};
// P base patterns, S species, rounds = k_max + 1 >= 1, cap = replicated patterns in flight (option dropout_patterns_max, or the default; cut to
// DROP_PATTERNS_HARD_MAX).  per_chunk = min(rounds, floor(cap / (P + 1))), also bounded so that per_chunk * (S + 1) stays 32-bit.  false, with the
// reason in err (PANTAX_HIP_E_LIMIT): not even one round fits.  P = 0: one chunk of all rounds (nothing is solved).
bool dropout_plan(uint64_t P, uint64_t S, uint64_t rounds, uint64_t cap, DropoutPlan &plan, std::string &err);

// The objective pass takes a species' sorted rows in slices of a fixed length that depends on its entries alone: DROP_SLICE_NARROW rows up to
// DROP_NARROW_E entries (accumulators in registers, rows across lanes), DROP_SLICE_WIDE beyond (entries across lanes).
constexpr uint32_t DROP_NARROW_E = 8, DROP_SLICE_NARROW = 16384, DROP_SLICE_WIDE = 4096;
constexpr uint32_t dropout_slice_rows(uint64_t E) { return E <= DROP_NARROW_E ? DROP_SLICE_NARROW : DROP_SLICE_WIDE; }
constexpr uint64_t dropout_slices(uint64_t rows, uint64_t E) { return rows / dropout_slice_rows(E) + (rows % dropout_slice_rows(E) ? 1 : 0); }

}  // namespace ptx
