// cov_state_check.cpp -- the lifecycle types of pantax_amd/csrc/cov_state.hpp (CovState, TrioState) against the flags they replaced, and cov_clean_plan
// at its edges.  A program of its own: tests/test_cov_state.py compiles it by the host compiler under -fsanitize=address,undefined and runs it; it
// returns non-zero at the first mismatch and prints the sequence of events that led there.
//
// `Old` is a transcription of the assignments the host code made to the flags of Db before the two types existed, event by event, in the order of the
// code (a successful call; the failure events are the ways a call returned part-way).  `New` holds the two types and goes through the lines that stand
// in the host code now.  Both are driven through every sequence of up to DEPTH events of the alphabet below that the code can raise:
//   * between coverage_prepare and coverage_launch the resident step raises nothing else -- while Old.cov_prepared only a launch or a failure follows;
//   * between the first filter and the row compaction the strain step raises nothing else -- while Old.trio_free_pending only the compaction or the
//     failed lad_prepare follows;
//   * the events of the strain step come behind its entry check (a coverage result and a built index), taken by each model on its own state.
// After every event:
//   * no failure event so far: every query answers the same in both, and coverage_prepare is told the same thing to do for the same and for a changed arena
//     signature.  (While Old.cov_prepared -- in the middle of a step's enqueue -- only "launch needs prepare" and the index queries are asked: nothing
//     else is asked there, and Old still claimed the result that the prepare had just zeroed.  The count of covered bases is asked where the strain step
//     may run, as in the code.)
//   * behind a failure event: New answers the same or claims less -- it never lets a call run that Old refused, never skips a fill Old made, never
//     skips a prepare Old made, and U is Old's or 0;
//   * always: coverage_prepare waits for the side-stream fill exactly when one was enqueued (in New's own history) and not yet waited for.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "cov_state.hpp"

using namespace ptx;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "cov_state_check:%d: %s\n", __LINE__, #cond);    \
            print_trail();                                                        \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

namespace {

constexpr int DEPTH = 5;
constexpr uint64_t ROWS = 7;        // U of a built index (the graphs decide it: every build of a db gives the same)
constexpr uint64_t SIG_SAME = 11;   // the arena's signature while its layout and place stay; a changed one is a fresh number

enum Event {
    stage_trio_build, same_rows_rebuild_with_keys, db_reset, prefetch, step_begin_rebuild, step_begin_keep, prepare_same, prepare_changed, launch_stage,
    launch_stage_trio_bases, launch_resident_deferred, launch_resident_counted, stage_mark, counted, readers_cleaned, side_fill_enqueued,
    first_filter_free_awaited, first_filter_free_recorded, row_compaction_passed,
    fail_between_prepare_and_launch, fail_between_fork_and_join, fail_lad_prepare, fail_inside_launch, N_EVENTS
};
const char *const NAMES[N_EVENTS] = {
    "stage trio build", "same-rows rebuild with keys (trio_get)", "db_reset", "prefetch", "step begin, rebuild_trio", "step begin, index kept", "prepare, same signature",
    "prepare, changed signature", "launch as stage", "launch as stage with trio_bases", "launch as resident, count deferred", "launch as resident, counted", "stage mark",
    "counted", "readers cleaned", "side fill enqueued", "first filter passed, free event awaited", "first filter passed, free event recorded", "row compaction passed",
    "FAILURE between prepare and launch", "FAILURE between fork and join (ForkGuard)", "FAILURE of lad_prepare", "FAILURE inside coverage_launch"};
bool is_failure(int e) { return e >= fail_between_prepare_and_launch; }

int trail[DEPTH], trail_n = 0;
void print_trail() {
    for (int i = 0; i < trail_n; ++i) std::fprintf(stderr, "  %d. %s\n", i + 1, NAMES[trail[i]]);
}

struct Action { bool ran = false, wait = false, skip = false; };

// ---- the flags of Db as they were, assigned as the code assigned them
struct Old {
    bool trio_built = false, trio_prefetched = false, trio_keys_built = false, trio_perm_valid = false;
    uint64_t U = 0;
    bool cov_prepared = false, cov_count_pending = false, cov_arena_clean = false;
    uint64_t cov_arena_sig = 0;
    bool cov_clean_pending = false, cov_done = false, cov_stage = false, trio_free_valid = false, trio_free_pending = false;

    void trio_index_build(bool with_keys) {
        trio_keys_built = false; trio_perm_valid = false;
        U = ROWS;
        trio_built = true; trio_keys_built = with_keys; cov_done = false;
    }
    void trio_export_ensure() {
        if (!(trio_built && trio_keys_built)) trio_index_build(true);   // trio_keys_ensure
        if (trio_perm_valid) return;
        trio_perm_valid = true;
    }
    Action coverage_prepare(uint64_t sig) {
        Action a; a.ran = true;
        if (cov_clean_pending) { a.wait = true; cov_clean_pending = false; }
        a.skip = cov_arena_clean && cov_arena_sig == sig;
        cov_arena_clean = false; cov_arena_sig = sig;
        cov_prepared = true;
        return a;
    }
    Action coverage_launch_begin() {
        Action a;
        if (!cov_prepared) a = coverage_prepare(SIG_SAME);
        cov_prepared = false; cov_stage = false; trio_free_valid = false;
        return a;
    }
    void coverage_launch_end(bool defer_count) { cov_count_pending = defer_count; cov_done = true; }
    bool strain_entry() const { return cov_done && trio_built; }

    Action apply(int e, uint64_t fresh_sig) {
        Action a;
        switch (e) {
        case stage_trio_build: if (!trio_built) trio_index_build(true); break;
        case same_rows_rebuild_with_keys:
            if (!trio_built) break;
            if (U) { const bool saved = cov_done; trio_export_ensure(); cov_done = saved; }
            break;
        case db_reset: trio_built = false; cov_done = false; U = 0; break;
        case prefetch:
            trio_built = false; cov_done = false; U = 0; trio_prefetched = false;
            trio_index_build(false);
            trio_prefetched = true;
            break;
        case step_begin_rebuild: case step_begin_keep:
            if (e == step_begin_rebuild && !(trio_prefetched && trio_built)) { trio_built = false; cov_done = false; U = 0; }
            trio_prefetched = false;
            if (!trio_built) trio_index_build(false);
            break;
        case prepare_same: a = coverage_prepare(SIG_SAME); break;
        case prepare_changed: a = coverage_prepare(fresh_sig); break;
        case launch_stage: a = coverage_launch_begin(); coverage_launch_end(false); cov_stage = true; break;
        case launch_stage_trio_bases:
            if (!trio_built) break;
            if (U) trio_export_ensure();
            a = coverage_launch_begin(); coverage_launch_end(false); cov_stage = true;
            break;
        case launch_resident_deferred: a = coverage_launch_begin(); coverage_launch_end(true); break;
        case launch_resident_counted: a = coverage_launch_begin(); coverage_launch_end(false); break;
        case stage_mark: cov_stage = true; break;
        case counted: if (strain_entry() && cov_count_pending) cov_count_pending = false; break;
        case readers_cleaned: if (strain_entry()) { cov_arena_clean = true; cov_done = false; } break;
        case side_fill_enqueued: if (strain_entry()) { cov_done = false; cov_arena_clean = true; cov_clean_pending = true; } break;
        case first_filter_free_awaited: if (strain_entry()) trio_free_pending = true; break;
        case first_filter_free_recorded: if (strain_entry()) { trio_free_pending = false; trio_free_valid = true; } break;
        case row_compaction_passed: if (strain_entry() && trio_free_pending) { trio_free_valid = true; trio_free_pending = false; } break;
        case fail_between_prepare_and_launch: cov_prepared = false; break;                              // CovPrepGuard
        case fail_between_fork_and_join: trio_built = false; cov_done = false; cov_prepared = false; break;   // ForkGuard, CovPrepGuard
        case fail_lad_prepare: if (strain_entry()) { trio_free_pending = false; trio_free_valid = false; } break;
        case fail_inside_launch: a = coverage_launch_begin(); break;
        }
        return a;
    }
};

// ---- the two types, through the lines of the host code
struct New {
    TrioState trio;
    CovState cov;
    uint64_t U = 0;
    bool fill_outstanding = false;   // (of the check) a fill went onto the side stream and no prepare has waited for it yet

    void index_invalidate() { trio.invalidate(U); cov.invalidated(); }
    void trio_index_build(bool with_keys) {
        const bool same_rows = trio.built();
        trio.build_begun();
        U = ROWS;
        trio.build_finished(with_keys);
        if (!same_rows) cov.invalidated();
    }
    void trio_export_ensure() {
        if (!trio.has_keys()) trio_index_build(true);
        if (trio.export_order_valid()) return;
        trio.export_order_made();
    }
    Action coverage_prepare(uint64_t sig) {
        Action a; a.ran = true;
        const CovPrepare todo = cov.prepare_begun(sig, 4096);
        a.wait = todo.wait_side_fill; a.skip = todo.skip_fill;
        cov.prepare_finished();
        return a;
    }
    Action coverage_launch_begin() {
        Action a;
        if (cov.launch_needs_prepare()) a = coverage_prepare(SIG_SAME);
        cov.launch_begun(); trio.free_event_void();
        return a;
    }
    bool strain_entry() const { return cov.strain_may_run() && trio.built(); }

    Action apply(int e, uint64_t fresh_sig) {
        Action a;
        switch (e) {
        case stage_trio_build: if (!trio.built()) trio_index_build(true); break;
        case same_rows_rebuild_with_keys:
            if (!trio.built()) break;
            if (U) trio_export_ensure();
            break;
        case db_reset: index_invalidate(); break;
        case prefetch:
            index_invalidate(); trio.prefetch_consumed();
            trio_index_build(false);
            trio.prefetched();
            break;
        case step_begin_rebuild: case step_begin_keep:
            if (e == step_begin_rebuild && !trio.serves_coming_step()) index_invalidate();
            trio.prefetch_consumed();
            if (!trio.built()) trio_index_build(false);
            break;
        case prepare_same: a = coverage_prepare(SIG_SAME); break;
        case prepare_changed: a = coverage_prepare(fresh_sig); break;
        case launch_stage: a = coverage_launch_begin(); cov.launch_finished(false); cov.stage_marked(); break;
        case launch_stage_trio_bases:
            if (!trio.built()) break;
            if (U) trio_export_ensure();
            a = coverage_launch_begin(); cov.launch_finished(false); cov.stage_marked();
            break;
        case launch_resident_deferred: a = coverage_launch_begin(); cov.launch_finished(true); break;
        case launch_resident_counted: a = coverage_launch_begin(); cov.launch_finished(false); break;
        case stage_mark: cov.stage_marked(); break;
        case counted: if (strain_entry() && cov.count_pending()) cov.counted(); break;
        case readers_cleaned: if (strain_entry()) cov.readers_cleaned(); break;
        case side_fill_enqueued: if (strain_entry()) { cov.invalidated(); cov.side_fill_enqueued(); fill_outstanding = true; } break;
        case first_filter_free_awaited: if (strain_entry()) trio.free_event_awaited(); break;
        case first_filter_free_recorded: if (strain_entry()) trio.free_event_recorded(); break;
        case row_compaction_passed: if (strain_entry() && trio.free_event_pending()) trio.free_event_recorded(); break;
        case fail_between_prepare_and_launch: cov.prepare_dropped(); break;
        case fail_between_fork_and_join: index_invalidate(); cov.prepare_dropped(); break;
        case fail_lad_prepare: if (strain_entry()) trio.free_event_void(); break;
        case fail_inside_launch: a = coverage_launch_begin(); break;
        }
        if (a.ran) {
            CHECK(a.wait == fill_outstanding);
            fill_outstanding = false;
        }
        return a;
    }
};

bool reachable(const Old &o, int e) {
    const bool in_launch = e == launch_stage || e == launch_stage_trio_bases || e == launch_resident_deferred || e == launch_resident_counted || e == fail_inside_launch;
    if (o.cov_prepared) return in_launch || e == fail_between_prepare_and_launch || e == fail_between_fork_and_join;
    if (e == fail_between_prepare_and_launch) return false;
    if (o.trio_free_pending) return e == row_compaction_passed || e == fail_lad_prepare;
    return true;
}

bool implies(bool a, bool b) { return !a || b; }

void compare(const Old &o, const New &n, bool failed, const Action &ao, const Action &an) {
    // what the old code asked of its flags
    const bool o_strain = o.cov_done, o_arena_gone = o.cov_arena_clean || o.cov_clean_pending;
    const bool o_stage = o.cov_done && o.cov_stage && !o.cov_count_pending && !o_arena_gone;
    const bool o_hint = o.cov_done || o_arena_gone;
    CHECK(n.cov.launch_needs_prepare() == !o.cov_prepared);
    CHECK(ao.ran == an.ran);
    if (!failed) {
        CHECK(ao.wait == an.wait && ao.skip == an.skip);
        CHECK(n.trio.built() == o.trio_built && n.trio.has_keys() == (o.trio_built && o.trio_keys_built) && n.trio.export_order_valid() == o.trio_perm_valid);
        CHECK(n.trio.serves_coming_step() == (o.trio_prefetched && o.trio_built));
        CHECK(n.trio.free_event_valid() == o.trio_free_valid && n.trio.free_event_pending() == o.trio_free_pending);
        CHECK(n.U == o.U);
        if (!o.cov_prepared) {
            CHECK(n.cov.strain_may_run() == o_strain && n.cov.stage_report_may_run() == o_stage && n.cov.resident_used_it() == o_hint);
            if (o_strain) CHECK(n.cov.count_pending() == o.cov_count_pending);
            else CHECK(!n.cov.count_pending());
            for (const uint64_t sig : {SIG_SAME, (uint64_t)5}) {   // what a prepare would be told now
                Old o2 = o; New n2 = n;
                const Action a2 = o2.coverage_prepare(sig), b2 = n2.coverage_prepare(sig);
                CHECK(a2.wait == b2.wait && a2.skip == b2.skip);
            }
        }
    } else {
        CHECK(implies(an.skip, ao.skip));
        CHECK(implies(n.trio.built(), o.trio_built) && implies(n.trio.has_keys(), o.trio_built && o.trio_keys_built) && implies(n.trio.export_order_valid(), o.trio_perm_valid));
        CHECK(implies(n.trio.serves_coming_step(), o.trio_prefetched && o.trio_built));
        CHECK(implies(n.trio.free_event_valid(), o.trio_free_valid) && implies(n.trio.free_event_pending(), o.trio_free_pending));
        CHECK(n.U == o.U || n.U == 0);
        CHECK(implies(n.cov.strain_may_run(), o_strain) && implies(n.cov.stage_report_may_run(), o_stage));
        if (n.cov.strain_may_run()) CHECK(n.cov.count_pending() == o.cov_count_pending);
        for (const uint64_t sig : {SIG_SAME, (uint64_t)5}) {
            Old o2 = o; New n2 = n;
            const Action a2 = o2.coverage_prepare(sig), b2 = n2.coverage_prepare(sig);
            CHECK(implies(b2.skip, a2.skip));
        }
    }
}

unsigned long long n_sequences = 0, n_with_failure = 0;
void run(const Old &o, const New &n, bool failed, int depth) {
    if (depth == DEPTH) return;
    for (int e = 0; e < N_EVENTS; ++e) {
        if (!reachable(o, e)) continue;
        Old o2 = o; New n2 = n;
        trail[depth] = e; trail_n = depth + 1;
        const uint64_t fresh_sig = 100 + (uint64_t)depth;
        const Action ao = o2.apply(e, fresh_sig), an = n2.apply(e, fresh_sig);
        const bool f2 = failed || is_failure(e);
        compare(o2, n2, f2, ao, an);
        ++n_sequences; n_with_failure += f2;
        run(o2, n2, f2, depth + 1);
    }
    trail_n = depth;
}

void check_clean_plan() {
    const size_t GiB = (size_t)1 << 30;
    // the conditions of strain_enqueue as they stood
    auto old_self = [](bool cp, bool opt_self, uint64_t U) { return cp && opt_self && U != 0; };
    auto old_async = [&](bool cp, bool opt_self, int opt_async, bool clocked, size_t bytes) {
        return cp && !opt_self && !clocked && (opt_async > 0 || (opt_async < 0 && bytes >= ((size_t)1 << 30)));
    };
    for (int cp = 0; cp < 2; ++cp) for (int self = 0; self < 2; ++self) for (int async = -1; async <= 1; ++async) for (int clocked = 0; clocked < 2; ++clocked)
        for (const size_t bytes : {(size_t)0, GiB - 1, GiB, 5 * GiB}) for (const uint64_t U : {(uint64_t)0, (uint64_t)1, ROWS}) {
            const CovClean c = cov_clean_plan(cp, self, async, clocked, bytes, U);
            const bool s = old_self(cp, self, U), a = old_async(cp, self, async, clocked, bytes);
            trail_n = 0;
            CHECK(!(s && a));
            CHECK(c == (s ? CovClean::readers_clean : a ? CovClean::side_fill : CovClean::fill_in_front));
        }
    trail_n = 0;
    // ... and spelled out at the edges
    CHECK(cov_clean_plan(true, false, -1, false, GiB - 1, ROWS) == CovClean::fill_in_front);
    CHECK(cov_clean_plan(true, false, -1, false, GiB, ROWS) == CovClean::side_fill);
    CHECK(cov_clean_plan(true, false, 0, false, 5 * GiB, ROWS) == CovClean::fill_in_front);
    CHECK(cov_clean_plan(true, false, 1, false, 0, ROWS) == CovClean::side_fill);
    CHECK(cov_clean_plan(true, false, 1, false, 0, 0) == CovClean::side_fill);            // (the side fill does not ask for trio rows)
    CHECK(cov_clean_plan(true, false, 1, true, 5 * GiB, ROWS) == CovClean::fill_in_front); // clocked
    CHECK(cov_clean_plan(true, true, 1, false, 5 * GiB, ROWS) == CovClean::readers_clean); // option cov_self_clean wins over cov_clean_async
    CHECK(cov_clean_plan(true, true, 1, true, 5 * GiB, ROWS) == CovClean::readers_clean);  // ... and is not a matter of clocking
    CHECK(cov_clean_plan(true, true, 1, false, 5 * GiB, 0) == CovClean::fill_in_front);    // U = 0: the trio_bases reader has nothing to clean by
    CHECK(cov_clean_plan(false, true, 1, false, 5 * GiB, ROWS) == CovClean::fill_in_front); // a stage call's result: its caller may read the arena again
    CHECK(cov_clean_plan(false, false, 1, false, 5 * GiB, ROWS) == CovClean::fill_in_front);
}

}  // namespace

int main() {
    check_clean_plan();
    run(Old{}, New{}, false, 0);
    std::printf("cov_state_check: ok (%llu sequences of up to %d events, %llu of them behind a failure event)\n", n_sequences, DEPTH, n_with_failure);
    return 0;
}
