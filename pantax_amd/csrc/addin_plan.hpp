// addin_plan.hpp -- the host decisions of pantax_hip_strain_addin (stage_addin.hip) as pure functions of plain values: where an entry and its x block sit
// in the outputs, how many rounds of add-one LPs go through the solver at once, the default of the cap on the replicated patterns in flight, which
// instance of the objective-and-count pass takes a species and how its sorted rows are cut into slices.  The host helper of the contract
// (pantax_hip_addin_donor) is defined in addin_plan.cpp beside them.  pantax_hip.h and standard headers only: tests/native/addin_plan_check.cpp compiles
// this with the host compiler alone.
#pragma once
#include <cstdint>
#include <string>

namespace ptx {

// Species s of K_s reported and J_s candidate haplotypes has W_s = K_s + J_s columns and E_s = J_s + 1 entries (0: every candidate pinned to zero; c + 1:
// candidate c free, the other candidates pinned).  Entry (s, e) is q = cand_off[s] + s + e of Q = J + S, and the species' x block of E_s x W_s doubles
// (entry-major) starts at x_off[s] = sum over t < s of E_t W_t.
inline uint64_t addin_entry(uint64_t cand_off_s, uint64_t s, uint64_t e) { return cand_off_s + s + e; }
// x_off [S + 1] from sel_off / cand_off [S + 1]; false when the total passes 2^64 - 1 (x_off is then unspecified)
bool addin_x_offsets(uint64_t S, const uint64_t *sel_off, const uint64_t *cand_off, uint64_t *x_off);

constexpr uint64_t ADDIN_MAX_W = 64;   // columns the solver's narrow instances and the 64-bit row mask serve

// A round e = 0 .. j_max holds every species once over ONE copy of the base pattern tables: P patterns and the closing slot, S entries and the closing
// one.  Bytes of device scratch a replicated pattern costs: mask 8, start 4, the solver's scratch 3 x 8 + 5 x 4.
constexpr uint64_t ADDIN_BYTES_PER_PATTERN = 8 + 4 + 3 * 8 + 5 * 4;
constexpr uint64_t ADDIN_PATTERNS_HARD_MAX = 0xFFFFFFFFull - 1;   // the solver's pattern and entry indices are 32-bit
// The default of option addin_patterns_max: a quarter of what is free on the device when the call begins, in patterns, at most the hard bound
uint64_t addin_default_cap(uint64_t free_bytes);

struct AddinPlan {
    uint32_t per_chunk = 0;       // rounds per chunk, >= 1 (the last chunk may hold fewer)
    uint32_t n_chunks = 0;        // ceil(rounds / per_chunk)
    uint64_t chunk_patterns = 0;  // per_chunk * (P + 1): what the replicated pattern tables hold
    uint64_t chunk_entries = 0;   // per_chunk * (S + 1)
};
// P base patterns, S species, rounds = j_max + 1 in 1 .. 65, cap = replicated patterns in flight (option addin_patterns_max, or the default; cut to
// ADDIN_PATTERNS_HARD_MAX).  per_chunk = min(rounds, floor(cap / (P + 1))), also bounded so that per_chunk * (S + 1) stays 32-bit.  false, with the reason
// in err (PANTAX_HIP_E_LIMIT): not even one round fits.  P = 0: one chunk of all rounds (nothing is solved).
bool addin_plan(uint64_t P, uint64_t S, uint64_t rounds, uint64_t cap, AddinPlan &plan, std::string &err);

// The objective-and-count pass.  The instance is a function of the species' W and E alone:
//   TABLE   W <= 7 (then E <= 8): the predictions of every entry for each of the 2^W <= 128 masks in LDS, rows across lanes, accumulators in registers;
//   FEW     W >  7, E <= 8: the entries' x in LDS, rows across lanes, a lane forms the E predictions when the mask of its row changes;
//   WIDE    E >  8: the entries' x in LDS, entries across lanes.
// The slice length depends on the instance alone: 16 384 rows where a row costs one table read, 4 096 where a thread may form predictions per row (a
// species of a few ten thousand rows and hundreds of patterns then spreads over four times the workgroups).
enum AddinInstance : uint32_t { ADDIN_TABLE = 0, ADDIN_FEW = 1, ADDIN_WIDE = 2 };
constexpr uint32_t ADDIN_TABLE_W = 7, ADDIN_FEW_E = 8, ADDIN_SLICE_TABLE = 16384, ADDIN_SLICE_FEW = 4096, ADDIN_SLICE_WIDE = 4096;
constexpr AddinInstance addin_instance(uint64_t W, uint64_t E) { return E > ADDIN_FEW_E ? ADDIN_WIDE : (W <= ADDIN_TABLE_W ? ADDIN_TABLE : ADDIN_FEW); }
constexpr uint32_t addin_slice_rows(uint64_t W, uint64_t E) {
    return addin_instance(W, E) == ADDIN_TABLE ? ADDIN_SLICE_TABLE : (addin_instance(W, E) == ADDIN_FEW ? ADDIN_SLICE_FEW : ADDIN_SLICE_WIDE);
}
constexpr uint64_t addin_slices(uint64_t rows, uint64_t W, uint64_t E) { return rows / addin_slice_rows(W, E) + (rows % addin_slice_rows(W, E) ? 1 : 0); }

}  // namespace ptx
