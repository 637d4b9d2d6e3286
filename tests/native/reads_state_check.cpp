// reads_state_check.cpp -- the lifecycle type of resident reads (pantax_amd/csrc/reads_state.hpp: ReadsState) against the seven flags of Reads it replaced.
// A program of its own: tests/test_reads_state.py compiles it by the host compiler under -fsanitize=address,undefined and runs it; it returns non-zero at
// the first mismatch and prints the sequence of events that led there.
//
// `Old` is a transcription of the assignments the host code made to has_flags, g_flags_valid, species_valid, binned, binned_db, grouped and long_sums_db
// before the type existed, event site by event site, in the order of the code; a failure event is a way the call returned part-way.  `New` holds a
// ReadsState and goes through the lines that stand in the host code now.  Both are driven through every sequence of DEPTH events of the alphabet below
// that the code can raise:
//   * a sequence begins where a reads object begins: at one of the three sites that put columns in place (pantax_hip_reads_upload, the device tokenizer,
//     reads_from_routed).  All three work on an object they have just created, so a later one starts a fresh object;
//   * a columns site that fails hands no object out (its callers delete it, or end the run): only another columns site follows;
//   * pantax_hip_reads_set_flags meets grouped reads only -- every reads handle of the C ABI is grouped, and the file seam calls it behind reads_group;
//     route_reads meets plain columns only -- the slice of a sharded run, which is routed away before anything groups it.  (The type decides by
//     "grouped", the flags decided by the site: on the other side of either line the type voids a binning the flags kept, or keeps one they voided.)
// Two dbs, uid 1 and 2.  After every event, for both uids:
//   * no failure event so far: has_flags, grouped, species_in_file_order and slot_flags_current answer as the flags did; binned_against(u) and
//     long_sums_from(u) answer as the flags did for the db of the last binning pass, and are false for the other db;
//   * always: has_flags is the flag's, and where any other query is true the flags' answer was true too (never laxer) -- for binned_against(u) that is
//     the strictest spelling the old callers used, binned && binned_db == u.
// Every query that is false where the flags said true is a stricter case: counted, and one example listed per (query, first cause).  DESIGN.md,
// "Lifecycle of resident reads", names the same cases.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "reads_state.hpp"

using namespace ptx;

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "reads_state_check:%d: %s\n", __LINE__, #cond);   \
            print_trail(stderr);                                                   \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

namespace {

constexpr int DEPTH = 5;
constexpr uint64_t UID[2] = {1, 2};

enum Event {
    upload_flags, upload_plain, upload_FAIL_build,
    tok_grouped, tok_columns, tok_grouped_FAIL_early, tok_columns_FAIL_early, tok_grouped_FAIL_build,
    routed, routed_FAIL_build,
    reads_group, reads_group_FAIL_build,
    set_flags_some, set_flags_null, set_flags_FAIL_upload,
    route_flags, route_flags_FAIL_upload,
    bin1_sums, bin1, bin1_FAIL_early, bin1_FAIL_mid, bin1_FAIL_late,
    bin2_sums, bin2, bin2_FAIL_early, bin2_FAIL_mid, bin2_FAIL_late,
    species_ensure, species_ensure_FAIL,
    N_EVENTS
};
const char *const NAMES[N_EVENTS] = {
    "reads_upload with flags", "reads_upload without flags", "reads_upload, FAILURE in build_step_read",
    "tokenizer, group", "tokenizer, columns only", "tokenizer, group, FAILURE before the columns are taken", "tokenizer, columns only, FAILURE before the columns are taken",
    "tokenizer, group, FAILURE in build_step_read",
    "reads_from_routed", "reads_from_routed, FAILURE in build_step_read",
    "reads_group", "reads_group, FAILURE in build_step_read",
    "set_flags(flags)", "set_flags(null)", "set_flags(flags), FAILURE of the upload",
    "route_reads replaces the flags", "route_reads, FAILURE of the flag upload",
    "bin against db 1, walk sums on the way", "bin against db 1", "bin against db 1, FAILURE before the pass begins", "bin against db 1, FAILURE at its first allocation",
    "bin against db 1, FAILURE behind its kernels",
    "bin against db 2, walk sums on the way", "bin against db 2", "bin against db 2, FAILURE before the pass begins", "bin against db 2, FAILURE at its first allocation",
    "bin against db 2, FAILURE behind its kernels",
    "species_ensure", "species_ensure, FAILURE of its allocation"};
bool is_failure(int e) { return std::strstr(NAMES[e], "FAILURE") != nullptr; }
bool is_columns_site(int e) { return e <= routed_FAIL_build; }

int trail[DEPTH], trail_n = 0;
void print_trail(FILE *f) {
    for (int i = 0; i < trail_n; ++i) std::fprintf(f, "      %d. %s\n", i + 1, NAMES[trail[i]]);
}

enum BinEnd { bin_ok, bin_fail_early, bin_fail_mid, bin_fail_late };
struct BinCall { uint64_t uid; bool sums; BinEnd end; };
BinCall bin_call(int e) {
    const int k = e >= bin2_sums ? e - bin2_sums : e - bin1_sums;
    const uint64_t uid = e >= bin2_sums ? UID[1] : UID[0];
    // (a pass that fails is one that would have taken the sums: the worst case for the claim it leaves)
    switch (k) {
    case 0: return {uid, true, bin_ok};
    case 1: return {uid, false, bin_ok};
    case 2: return {uid, true, bin_fail_early};
    case 3: return {uid, true, bin_fail_mid};
    default: return {uid, true, bin_fail_late};
    }
}

// ---- the flags of Reads as they were, assigned as the code assigned them
struct Old {
    bool has_flags = false, g_flags_valid = false, species_valid = false, binned = false;
    uint64_t binned_db = 0;
    bool grouped = true;
    uint64_t long_sums_db = 0;

    bool build_step_read(bool ok) { g_flags_valid = false; species_valid = false; return ok; }
    void bin_reads_launch(const BinCall &c) {
        if (c.end == bin_fail_early) return;                 // the memset of the counters, option bin_route
        species_valid = false;
        binned_db = c.uid;
        if (grouped) {
            if (has_flags) {
                if (!g_flags_valid) {
                    if (c.end == bin_fail_mid) return;       // d_g_flag.alloc
                    g_flags_valid = true;
                }
            }
            long_sums_db = c.sums ? c.uid : 0;
        } else {
            if (c.end == bin_fail_mid) return;               // d_species.alloc
            species_valid = true;
        }
        if (c.end != bin_ok) return;                         // hipGetLastError behind the kernels
        binned = true;
    }
    void apply(int e) {
        switch (e) {
        case upload_flags: case upload_plain: case upload_FAIL_build:          // api_core.cpp, on `new pantax_hip_reads()`
            *this = Old();
            has_flags = e != upload_plain;
            (void)build_step_read(e != upload_FAIL_build);
            break;
        case tok_grouped: case tok_columns: case tok_grouped_FAIL_early: case tok_columns_FAIL_early: case tok_grouped_FAIL_build: {   // stage_gaf.hip, on a new object
            const bool group = e != tok_columns && e != tok_columns_FAIL_early;
            *this = Old();
            grouped = group;
            if (e == tok_grouped_FAIL_early || e == tok_columns_FAIL_early) break;
            has_flags = true;
            if (group) (void)build_step_read(e != tok_grouped_FAIL_build);
            break;
        }
        case routed: case routed_FAIL_build:                                    // stage_route.hip, on a new object, group = true
            *this = Old();
            has_flags = false;
            binned = false;
            (void)build_step_read(e != routed_FAIL_build);
            break;
        case reads_group: case reads_group_FAIL_build:                          // stage_read_layout.hip
            if (grouped) break;
            if (!build_step_read(e != reads_group_FAIL_build)) break;
            grouped = true;
            binned = false;
            break;
        case set_flags_some: case set_flags_null: case set_flags_FAIL_upload:   // stage_gaf.hip
            has_flags = e != set_flags_null;
            if (e == set_flags_FAIL_upload) break;
            g_flags_valid = false;
            binned = false;
            break;
        case route_flags: case route_flags_FAIL_upload:                         // api_profile.cpp
            if (e == route_flags_FAIL_upload) break;
            has_flags = true;
            g_flags_valid = false;
            break;
        case species_ensure: case species_ensure_FAIL:                          // stage_bin.hip
            if (species_valid) break;
            if (e == species_ensure_FAIL) break;
            species_valid = true;
            break;
        default: bin_reads_launch(bin_call(e));
        }
    }
};

// ---- the type, through the lines of the host code
struct New {
    ReadsState st;

    bool build_step_read(bool ok) {
        st.layout_begun();
        if (!ok) return false;
        st.layout_finished();
        return true;
    }
    void bin_reads_launch(const BinCall &c) {
        if (c.end == bin_fail_early) return;
        const bool grouped = st.grouped();
        st.bin_begun();
        bool sums = false;
        if (grouped) {
            if (st.has_flags()) {
                if (!st.slot_flags_current()) {
                    if (c.end == bin_fail_mid) return;
                    st.slot_flags_filed();
                }
            }
            sums = c.sums;
        } else {
            if (c.end == bin_fail_mid) return;
        }
        if (c.end != bin_ok) return;
        st.bin_finished(c.uid, !grouped, sums);
    }
    void apply(int e) {
        switch (e) {
        case upload_flags: case upload_plain: case upload_FAIL_build:
            st = ReadsState();
            st.columns_replaced(e != upload_plain);
            (void)build_step_read(e != upload_FAIL_build);
            break;
        case tok_grouped: case tok_columns: case tok_grouped_FAIL_early: case tok_columns_FAIL_early: case tok_grouped_FAIL_build:
            st = ReadsState();
            if (e == tok_grouped_FAIL_early || e == tok_columns_FAIL_early) break;
            st.columns_replaced(true);
            if (e != tok_columns) (void)build_step_read(e != tok_grouped_FAIL_build);
            break;
        case routed: case routed_FAIL_build:
            st = ReadsState();
            st.columns_replaced(false);
            (void)build_step_read(e != routed_FAIL_build);
            break;
        case reads_group: case reads_group_FAIL_build:
            if (st.grouped()) break;
            (void)build_step_read(e != reads_group_FAIL_build);
            break;
        case set_flags_some: case set_flags_null: case set_flags_FAIL_upload:
            st.flags_replaced(e != set_flags_null);
            break;
        case route_flags: case route_flags_FAIL_upload:
            if (e == route_flags_FAIL_upload) break;
            st.flags_replaced(true);
            break;
        case species_ensure: case species_ensure_FAIL:
            if (st.species_in_file_order()) break;
            if (e == species_ensure_FAIL) break;
            st.species_gathered();
            break;
        default: bin_reads_launch(bin_call(e));
        }
    }
};

bool reachable(const Old &o, int depth, int prev, int e) {
    if (depth == 0 || (is_columns_site(prev) && is_failure(prev))) return is_columns_site(e);
    if (e == set_flags_some || e == set_flags_null || e == set_flags_FAIL_upload) return o.grouped;
    if (e == route_flags || e == route_flags_FAIL_upload) return !o.grouped;
    return true;
}

// ---- the stricter cases: (query, the event at which the type first answered less than the flags) -> how often, and the first trail that showed it
enum Query { q_grouped, q_species, q_slot_flags, q_binned, q_binned_2, q_long_sums, q_long_sums_2, N_QUERIES };   // (the _2: the same query for db 2)
const char *const QUERY_NAMES[N_QUERIES] = {"grouped", "species_in_file_order", "slot_flags_current", "binned_against", "binned_against", "long_sums_from", "long_sums_from"};
constexpr int OTHER_DB = N_EVENTS;   // cause: no event -- the consumer's db is not the db of the last binning pass
struct Case { unsigned long long n = 0; int trail[DEPTH], trail_n = 0; } cases[N_QUERIES][N_EVENTS + 1];

bool implies(bool a, bool b) { return !a || b; }

// returns the queries (bit per Query) that answer stricter than the flags now; `before`: those that did before this event
unsigned compare(const Old &o, const New &n, bool failed, unsigned before) {
    const ReadsState &s = n.st;
    unsigned stricter = 0;
    auto one = [&](int q, bool now, bool was, bool must_equal, int cause) {
        CHECK(implies(now, was));
        if (must_equal) CHECK(now == was);
        if (!was || now) return;
        stricter |= 1u << q;
        if (before & (1u << q)) return;
        Case &c = cases[q == q_binned_2 ? q_binned : q == q_long_sums_2 ? q_long_sums : q][cause];
        if (c.n++ == 0) { c.trail_n = trail_n; std::memcpy(c.trail, trail, sizeof(trail)); }
    };
    const int e = trail[trail_n - 1];
    CHECK(s.has_flags() == o.has_flags);
    one(q_grouped, s.grouped(), o.grouped, !failed, e);
    one(q_species, s.species_in_file_order(), o.species_valid, !failed, e);
    one(q_slot_flags, s.slot_flags_current(), o.g_flags_valid, !failed, e);
    for (int k = 0; k < 2; ++k) {
        const uint64_t u = UID[k];
        const bool last = o.binned_db == u;   // (without a failure: the db of the last binning pass, or none yet)
        // node_coverage, species_profile and route_pack asked `binned` alone; check_read_strain_set asked binned && binned_db == u
        CHECK(implies(s.binned_against(u), o.binned && o.binned_db == u));
        one(q_binned + k, s.binned_against(u), o.binned, !failed && last, last ? e : OTHER_DB);
        if (!failed && !last) CHECK(!s.binned_against(u) && !s.long_sums_from(u));
        one(q_long_sums + k, s.long_sums_from(u), o.long_sums_db != 0 && o.long_sums_db == u, !failed, e);
    }
    return stricter;
}

unsigned long long n_sequences = 0, n_stricter = 0, n_with_failure = 0;
void run(const Old &o, const New &n, bool failed, unsigned stricter, int depth, int prev) {
    if (depth == DEPTH) return;
    for (int e = 0; e < N_EVENTS; ++e) {
        if (!reachable(o, depth, prev, e)) continue;
        Old o2 = o; New n2 = n;
        trail[depth] = e; trail_n = depth + 1;
        o2.apply(e); n2.apply(e);
        const bool f2 = is_columns_site(e) ? is_failure(e) : failed || is_failure(e);   // (a new object forgets the failures of the one before it)
        const unsigned s2 = compare(o2, n2, f2, is_columns_site(e) ? 0u : stricter);
        if (depth + 1 == DEPTH) { ++n_sequences; n_stricter += s2 != 0; n_with_failure += f2; }
        run(o2, n2, f2, s2, depth + 1, e);
    }
    trail_n = depth;
}

}  // namespace

int main() {
    run(Old{}, New{}, false, 0u, 0, -1);
    std::printf("reads_state_check: ok (%llu sequences of %d events, %llu of them behind a failure event; %llu ended stricter than the flags)\n", n_sequences, DEPTH,
                n_with_failure, n_stricter);
    std::printf("stricter cases (a query false where the flags said true; by the event that made it so), one example each, from the object's first event on:\n");
    for (int q = 0; q < N_QUERIES; ++q)
        for (int c = 0; c <= N_EVENTS; ++c) {
            const Case &k = cases[q][c];
            if (!k.n) continue;
            std::printf("  %s, at: %s (%llu times)\n", QUERY_NAMES[q], c == OTHER_DB ? "no event -- the consumer's db is not the db of the last binning pass" : NAMES[c], k.n);
            int first = 0;
            for (int i = 0; i < k.trail_n; ++i) if (is_columns_site(k.trail[i])) first = i;
            trail_n = k.trail_n - first; std::memcpy(trail, k.trail + first, sizeof(int) * (size_t)trail_n);
            print_trail(stdout);
        }
    return 0;
}
