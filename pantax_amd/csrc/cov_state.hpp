// cov_state.hpp -- what the coverage arena of a db holds and how far its unique-trio index is built, as two small state types whose fields change only
// through named transitions (one per event in the host code) and are read only through named queries, and the one decision of the strain step that
// depends on them: how the arena gets back to zero (cov_clean_plan).  Host only, no HIP: tests/native/cov_state_check.cpp drives both types against a
// transcription of the flags they replaced.  The states, the events and who raises them: DESIGN.md, "Lifecycle of the coverage arena and of the
// unique-trio index".
#pragma once
#include <cstddef>
#include <cstdint>

namespace ptx {

// what coverage_prepare has to do: wait for the fill that is running on the side stream (ev_cov_clean), then zero the arena itself or only its abort counter
struct CovPrepare { bool wait_side_fill, skip_fill; };

class CovState {
public:
    enum class Holds : uint8_t {
        unknown,        // nothing a later call may rely on: never filled, partly written, or a result whose index was replaced
        zero,           // all zero in the layout `sig`: the last readers of a resident step cleaned it
        zero_pending,   // ... once the fill enqueued on the side stream is over: whoever touches the arena next waits for ev_cov_clean first
        prepared,       // zero in the layout `sig` for the coverage pass that comes next in the same call
        result          // bases, trio_bases, bit vector and full-node flags of a finished coverage pass
    };
    Holds holds() const { return holds_; }
    size_t arena_bytes() const { return bytes_; }

    // ---- queries
    bool strain_may_run() const { return holds_ == Holds::result; }
    // node_base_cov is still to be counted from the bit vector: the node statistics pass of the strain step does it (or the fused node pass)
    bool count_pending() const { return holds_ == Holds::result && pending_; }
    // the strain reports of the file seam read bases and node_base_cov as the STAGE call leaves them
    bool stage_report_may_run() const { return holds_ == Holds::result && stage_ && !pending_; }
    // (their error text: a resident step used the arena last)
    bool resident_used_it() const { return holds_ == Holds::result || holds_ == Holds::zero || holds_ == Holds::zero_pending; }
    bool launch_needs_prepare() const { return holds_ != Holds::prepared; }

    // ---- transitions
    // coverage_prepare has bound the arena (layout signature, size) and is about to zero it: until prepare_finished nothing is claimed
    CovPrepare prepare_begun(uint64_t sig, size_t bytes) {
        const CovPrepare act{holds_ == Holds::zero_pending, (holds_ == Holds::zero || holds_ == Holds::zero_pending) && sig_ == sig};
        holds_ = Holds::unknown; sig_ = sig; bytes_ = bytes;
        return act;
    }
    void prepare_finished() { holds_ = Holds::prepared; }
    void prepare_dropped() { if (holds_ == Holds::prepared) holds_ = Holds::unknown; }   // the call that prepared returns without its coverage pass
    void launch_begun() { holds_ = Holds::unknown; }                                     // the kernels write from here on
    void launch_finished(bool count_deferred) { holds_ = Holds::result; stage_ = false; pending_ = count_deferred; }
    void stage_marked() { if (holds_ == Holds::result) stage_ = true; }                  // pantax_hip_node_coverage, behind its own pass
    void counted() { pending_ = false; }
    void readers_cleaned() { if (holds_ == Holds::result) holds_ = Holds::zero; }        // (in the layout of the pass they read)
    void side_fill_enqueued() { holds_ = Holds::zero_pending; }
    // the index the result was taken with is gone.  A zeroed arena stays zero, and a fill on the side stream stays to be waited for
    void invalidated() { if (holds_ == Holds::result) holds_ = Holds::unknown; }

private:
    Holds holds_ = Holds::unknown;
    bool stage_ = false, pending_ = false;   // of a result: left by the stage call (else by a resident step); covered bases not yet counted
    uint64_t sig_ = 0;                       // layout and place of the arena at the last prepare
    size_t bytes_ = 0;
};

class TrioState {
public:
    // ---- queries
    bool built() const { return built_; }
    bool has_keys() const { return built_ && keys_; }                // d_trio_q (window start of every row) was written by the last build
    bool export_order_valid() const { return perm_; }                // d_trio_perm holds the export order of the last build
    bool serves_coming_step() const { return prefetched_ && built_; }   // pantax_hip_trio_index_prefetch built it for the step that comes: its rebuild_trio is served
    bool free_event_valid() const { return free_valid_; }            // ev_trio_free stands behind the last reader of the tables
    bool free_event_pending() const { return free_pending_; }        // ... is still to be recorded by lad_prepare, behind the row compaction

    // ---- transitions
    // db_reset, a step that was asked to rebuild, prefetch, a build that failed: the tables hold no index.  The only place that resets U
    void invalidate(uint64_t &U) { built_ = false; U = 0; }
    void build_begun() { built_ = false; keys_ = false; perm_ = false; }   // the tables are being rewritten
    void build_finished(bool with_keys) { built_ = true; keys_ = with_keys; }
    void prefetched() { prefetched_ = true; }
    void prefetch_consumed() { prefetched_ = false; }                // (a prefetched index serves ONE step: the run it was started for)
    void export_order_made() { perm_ = true; }
    void free_event_awaited() { free_pending_ = true; }
    void free_event_recorded() { free_valid_ = true; free_pending_ = false; }
    void free_event_void() { free_valid_ = false; free_pending_ = false; }   // a new reader went onto the stream, or the step failed before it recorded

private:
    bool built_ = false, prefetched_ = false, keys_ = false, perm_ = false;
    bool free_valid_ = false, free_pending_ = false;
};

// How the arena a resident step has read gets back to zero for the next coverage pass.
//   fill_in_front : the next coverage_prepare zero-fills it (stage calls, whose caller may read bases / trio_bases again; small arenas)
//   readers_clean : option cov_self_clean -- this step's two statistics passes, the arena's only readers, zero what they read
//   side_fill     : option cov_clean_async -- a fill on the side stream in front of the LPs (coverage_arena_clean_async); -1: from 1 GiB of arena on (at
//                   0.4 GB the two events cost more than the 0.07 ms fill), and never while every launch is being clocked (the per-kernel table wants the
//                   fill's own time)
enum class CovClean : uint8_t { fill_in_front, readers_clean, side_fill };
constexpr size_t COV_CLEAN_ASYNC_MIN_BYTES = (size_t)1 << 30;
inline CovClean cov_clean_plan(bool count_pending, bool opt_self_clean, int opt_clean_async, bool clocked, size_t arena_bytes, uint64_t U) {
    if (!count_pending) return CovClean::fill_in_front;   // not a resident step's result
    if (opt_self_clean) return U != 0 ? CovClean::readers_clean : CovClean::fill_in_front;
    if (clocked) return CovClean::fill_in_front;
    return opt_clean_async > 0 || (opt_clean_async < 0 && arena_bytes >= COV_CLEAN_ASYNC_MIN_BYTES) ? CovClean::side_fill : CovClean::fill_in_front;
}

}  // namespace ptx
