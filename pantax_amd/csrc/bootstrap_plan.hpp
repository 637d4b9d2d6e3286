// bootstrap_plan.hpp -- the host decisions of pantax_hip_strain_bootstrap (stage_bootstrap.hip) as pure functions of plain values: how many expanded rows
// a replicate is sized for, how many replicates go through the device at once, and the default of the cap on the expanded rows in flight.  The two host
// helpers of the contract (pantax_hip_bootstrap_weight, pantax_hip_bootstrap_summary) are defined in bootstrap_plan.cpp beside them.  pantax_hip.h and
// standard headers only: tests/native/bootstrap_plan_check.cpp compiles this with the host compiler alone.
#pragma once
#include <cstdint>
#include <string>

namespace ptx {

// A replicate repeats row v w_v times, w_v ~ Poisson(1) capped at 16: the sum over N rows has mean N and a standard deviation below sqrt(N).  The device
// buffers of a replicate are sized for N + 8 ceil(sqrt(N)) + 64 rows -- eight standard deviations (a tail below 1e-15 per replicate) -- and no more than
// the certain bound 16 N; the finalise pass checks the sum it found against the buffer, and a chunk beyond it solves nothing and fails the call with
// PANTAX_HIP_E_LIMIT instead of writing past the end.  Replicate 0 has exactly N.
uint64_t bootstrap_rows_bound(uint64_t n_rows);
// bytes of device scratch one expanded row costs at the most (every row a pattern of its own): the row 8, its offset 4, and per pattern mask 8, start 4,
// prefix 4, the solver's scratch 3 x 8 + 5 x 4
constexpr uint64_t BOOT_BYTES_PER_ROW = 8 + 4 + 8 + 4 + 4 + 3 * 8 + 5 * 4;
constexpr uint64_t BOOT_ROWS_HARD_MAX = 0xFFFFFFFFull - 1;   // the scan's prefixes and the solver's pat_start are 32-bit
// The default of option bootstrap_rows_max: a quarter of what is free on the device when the call begins (the rows and the db are resident beside it; the
// share dev_cache_max keeps out of its own cap plus a margin), in rows of BOOT_BYTES_PER_ROW, at most BOOT_ROWS_HARD_MAX
uint64_t bootstrap_default_cap(uint64_t free_bytes);

struct BootstrapPlan {
    uint64_t bound = 0;        // expanded rows a replicate is sized for (bootstrap_rows_bound)
    uint32_t per_chunk = 0;    // replicates per chunk, >= 1 (the last chunk may hold fewer)
    uint32_t n_chunks = 0;     // ceil(R / per_chunk)
    uint64_t chunk_rows = 0;   // per_chunk * bound: what the row buffers hold
};
// n_rows = rows of all served species (sum over species), R = n_replicates + 1 >= 1, cap = expanded rows in flight (option bootstrap_rows_max, or the
// default; cut to BOOT_ROWS_HARD_MAX).  per_chunk = min(R, floor(cap / bound)), also bounded so that per_chunk * n_rows (the scan's items) stays below
// 2^32.  false, with the reason in err (PANTAX_HIP_E_LIMIT): not even one replicate fits the cap.  n_rows = 0: one chunk of all R replicates.
bool bootstrap_plan(uint64_t n_rows, uint64_t R, uint64_t cap, BootstrapPlan &plan, std::string &err);

}  // namespace ptx
