// dropout_plan_check.cpp -- the host side of pantax_hip_strain_dropout at its edges: the plan of the chunks of rounds and the index arithmetic of the
// outputs (pantax_amd/csrc/dropout_plan.hpp), the substitute helper, and the report's row in the plan of the file seam.  A program of its own:
// tests/test_dropout_plan.py compiles it with dropout_plan.cpp and report_plan.cpp by the host C++ compiler under -fsanitize=address,undefined and runs it;
// it returns non-zero at the first check that fails.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "dropout_plan.hpp"
#include "report_plan.hpp"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "dropout_plan_check:%d: %s\n", __LINE__, #cond);     \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

using namespace ptx;

int main() {
    DropoutPlan pl;
    std::string err;
    // ---- the plan: one round (K = 0 everywhere is never planned; k_max = 0 cannot happen with rows, but one round must still stand)
    CHECK(dropout_plan(1000, 9, 1, 1u << 20, pl, err));
    CHECK(pl.per_chunk == 1 && pl.n_chunks == 1 && pl.chunk_patterns == 1001 && pl.chunk_entries == 10);
    // all rounds in one chunk, and never more than there are
    CHECK(dropout_plan(1000, 9, 65, 1u << 20, pl, err));
    CHECK(pl.per_chunk == 65 && pl.n_chunks == 1 && pl.chunk_patterns == 65 * 1001 && pl.chunk_entries == 650);
    // a cap of exactly one round (P patterns and the closing slot), of exactly two, one below three, and one below one
    CHECK(dropout_plan(1000, 9, 65, 1001, pl, err) && pl.per_chunk == 1 && pl.n_chunks == 65 && pl.chunk_patterns == 1001);
    CHECK(dropout_plan(1000, 9, 65, 2002, pl, err) && pl.per_chunk == 2 && pl.n_chunks == 33 && pl.chunk_entries == 20);
    CHECK(dropout_plan(1000, 9, 65, 3002, pl, err) && pl.per_chunk == 2);
    CHECK(dropout_plan(1000, 9, 4, 2002, pl, err) && pl.per_chunk == 2 && pl.n_chunks == 2);
    CHECK(dropout_plan(1000, 9, 3, 2002, pl, err) && pl.per_chunk == 2 && pl.n_chunks == 2);   // the last chunk holds one
    err.clear();
    CHECK(!dropout_plan(1000, 9, 65, 1000, pl, err));
    CHECK(err.find("dropout_patterns_max") != std::string::npos && err.find("1000 patterns") != std::string::npos && pl.per_chunk == 0);
    CHECK(!dropout_plan(1000, 9, 65, 0, pl, err));
    // no pattern at all: nothing to size, one chunk, whatever the cap
    CHECK(dropout_plan(0, 9, 65, 0, pl, err) && pl.per_chunk == 65 && pl.n_chunks == 1 && pl.chunk_patterns == 0 && pl.chunk_entries == 0);
    // no round, and more than the 65 a species of 64 columns has
    CHECK(!dropout_plan(10, 1, 0, 1000, pl, err));
    CHECK(!dropout_plan(10, 1, 66, 1000, pl, err));
    // u64 sizes: the cap is cut to 32-bit pattern positions; the entries of a chunk stay 32-bit; patterns or species beyond them are refused
    CHECK(dropout_plan(1u << 20, 3, 65, ~0ull, pl, err) && pl.per_chunk == 65 && pl.chunk_patterns <= DROP_PATTERNS_HARD_MAX);
    CHECK(dropout_plan(4000000000ull, 3, 65, ~0ull, pl, err) && pl.per_chunk == 1 && pl.n_chunks == 65);
    CHECK(dropout_plan(10, 4000000000ull, 65, ~0ull, pl, err) && pl.per_chunk == 1 && pl.chunk_entries == 4000000001ull);
    CHECK(dropout_plan(10, 1u << 30, 65, ~0ull, pl, err) && pl.per_chunk == 3 && (uint64_t)pl.per_chunk * ((1ull << 30) + 1) <= DROP_PATTERNS_HARD_MAX);
    CHECK(!dropout_plan(1ull << 32, 3, 2, ~0ull, pl, err));
    CHECK(!dropout_plan(~0ull, 3, 2, ~0ull, pl, err));
    CHECK(!dropout_plan(DROP_PATTERNS_HARD_MAX, 3, 2, ~0ull, pl, err));
    CHECK(!dropout_plan(10, 1ull << 32, 2, ~0ull, pl, err));
    // the default cap: a quarter of the free memory in patterns, cut to 32-bit positions
    CHECK(dropout_default_cap(0) == 0);
    CHECK(dropout_default_cap(4 * DROP_BYTES_PER_PATTERN * 1000 + 5) == 1000);
    CHECK(dropout_default_cap(~0ull) == DROP_PATTERNS_HARD_MAX);
    // ---- entries and x blocks: K = 0, 1, 64, 65 side by side
    {
        const uint64_t sel_off[5] = {0, 0, 1, 65, 130};
        uint64_t x_off[5];
        CHECK(dropout_x_offsets(4, sel_off, x_off));
        CHECK(x_off[0] == 0 && x_off[1] == 0 && x_off[2] == 2 && x_off[3] == 2 + 65 * 64 && x_off[4] == 2 + 65 * 64 + 66 * 65);
        CHECK(dropout_entry(sel_off[0], 0, 0) == 0);                                      // K = 0: the one entry
        CHECK(dropout_entry(sel_off[1], 1, 0) == 1 && dropout_entry(sel_off[1], 1, 1) == 2);   // K = 1: two
        CHECK(dropout_entry(sel_off[2], 2, 0) == 3 && dropout_entry(sel_off[2], 2, 64) == 67);
        CHECK(dropout_entry(sel_off[3], 3, 0) == 68 && dropout_entry(sel_off[3], 3, 65) == 133);
        CHECK(dropout_entry(sel_off[4], 4, 0) == 130 + 4);                                // Q = C + S: one beyond the last entry
        const uint64_t none[1] = {0};
        CHECK(dropout_x_offsets(0, none, x_off) && x_off[0] == 0);
        const uint64_t huge[2] = {0, 1ull << 33};                                         // (2^33 + 1) 2^33 passes 2^64
        CHECK(!dropout_x_offsets(1, huge, x_off));
        const uint64_t big[2] = {0, (1ull << 32) - 1};                                    // 2^32 (2^32 - 1) does not
        CHECK(dropout_x_offsets(1, big, x_off) && x_off[1] == ((1ull << 32) - 1) << 32);
    }
    // ---- the slices of the objective pass
    CHECK(dropout_slice_rows(1) == DROP_SLICE_NARROW && dropout_slice_rows(8) == DROP_SLICE_NARROW && dropout_slice_rows(9) == DROP_SLICE_WIDE && dropout_slice_rows(65) == DROP_SLICE_WIDE);
    CHECK(dropout_slices(0, 2) == 0 && dropout_slices(1, 2) == 1 && dropout_slices(DROP_SLICE_NARROW, 2) == 1 && dropout_slices(DROP_SLICE_NARROW + 1, 2) == 2);
    CHECK(dropout_slices(DROP_SLICE_WIDE, 65) == 1 && dropout_slices(DROP_SLICE_WIDE + 1, 65) == 2 && dropout_slices(~0ull, 65) == (~0ull) / DROP_SLICE_WIDE + 1);
    // ---- the substitute
    double out[3];
    const double one_f[1] = {2.5}, one_d[1] = {0.0};
    CHECK(pantax_hip_dropout_substitute(1, 0, one_f, one_d, nullptr) == PANTAX_HIP_E_INVALID);
    CHECK(pantax_hip_dropout_substitute(1, 1, one_f, one_d, out) == PANTAX_HIP_E_INVALID);
    CHECK(pantax_hip_dropout_substitute(0, 0, one_f, one_d, out) == PANTAX_HIP_E_INVALID);
    CHECK(pantax_hip_dropout_substitute(1, 0, nullptr, one_d, out) == PANTAX_HIP_E_INVALID);
    CHECK(pantax_hip_dropout_substitute(1, 0, one_f, one_d, out) == 0 && out[0] == -1.0 && out[1] == 0.0 && out[2] == 0.0);   // K = 1: nobody is left
    const double f4[4] = {1.0, 2.0, 3.0, 4.0};
    const double tie[4] = {0.0, 2.5, 3.5, 4.25};                 // columns 1 and 2 gain 0.5 each, column 3 0.25: the lowest of the tie
    CHECK(pantax_hip_dropout_substitute(4, 0, f4, tie, out) == 0 && out[0] == 1.0 && out[1] == 0.5 && out[2] == 1.25);
    const double drop3[4] = {1.5, 2.5, 3.0, 0.0};                 // the dropped column is not looked at, whatever it holds
    CHECK(pantax_hip_dropout_substitute(4, 3, f4, drop3, out) == 0 && out[0] == 0.0 && out[1] == 0.5 && out[2] == 1.0);
    const double big3[4] = {1.0, 2.0, 0.0, 99.0};                 // k = 2: the largest gain wins over an earlier smaller one
    CHECK(pantax_hip_dropout_substitute(4, 2, f4, big3, out) == 0 && out[0] == 3.0 && out[1] == 95.0 && out[2] == 95.0);
    const double loss[4] = {0.0, 1.5, 3.0, 3.0};                  // nobody gains: -1, gain 0, the shift still counts the losses
    CHECK(pantax_hip_dropout_substitute(4, 0, f4, loss, out) == 0 && out[0] == -1.0 && out[1] == 0.0 && out[2] == 1.5);
    CHECK(pantax_hip_dropout_substitute(4, 1, f4, f4, out) == 0 && out[0] == -1.0 && out[2] == 0.0);   // no difference is no positive gain
    // ---- the report in the file seam's plan: a field of pantax_hip_profile_ext3, which begins with the 40-byte second version; a row of EXT3_REPORTS
    {
        static_assert(offsetof(pantax_hip_profile_ext3, v2) == 0 && sizeof(pantax_hip_profile_ext2) == 40 && sizeof(pantax_hip_profile_ext) == 16, "the earlier versions keep their place and size");
        static_assert(offsetof(pantax_hip_profile_ext3, strain_dropout_file) == 40 && sizeof(pantax_hip_profile_ext3) == 48, "appended behind them");
        CHECK(N_EXT3_REPORTS == 1 && EXT3_REPORTS[X3REP_DROPOUT].field == &pantax_hip_profile_ext3::strain_dropout_file && EXT3_REPORTS[X3REP_DROPOUT].rows);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        pantax_hip_profile_ext3 e3{};
        e3.v2.v1.struct_size = sizeof(e3);
        e3.strain_dropout_file = "drop.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(&e3.v2.v1, 1, false, rp, err));
        CHECK(rp.ext3_want[X3REP_DROPOUT] && !rp.ext3_run[X3REP_DROPOUT] && rp.ext3_path[X3REP_DROPOUT] == "drop.tsv" && !rp.ext_want[XREP_FIT] && !rp.ext2_want[X2REP_BOOTSTRAP]);
        resume_reports(rp, true, true, false);
        CHECK(rp.ext3_run[X3REP_DROPOUT] && rp.any_run() && rp.rows_run() && !rp.ext2_run[X2REP_BOOTSTRAP]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext3_run[X3REP_DROPOUT] && !rp.any_run() && !rp.rows_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext3_run[X3REP_DROPOUT]);
        CHECK(!plan_ext_reports(&e3.v2.v1, 2, false, rp, err) && err == "profile: the leave-one-out report (strain_dropout_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(&e3.v2.v1, 1, true, rp, err) && err == "profile: the leave-one-out report (strain_dropout_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e3.v2.strain_bootstrap_file = "boot.tsv";                     // the bootstrap report's refusal comes first, the fit report's before it
        CHECK(!plan_ext_reports(&e3.v2.v1, 2, false, rp, err) && err.find("strain_bootstrap_file") != std::string::npos);
        e3.v2.v1.strain_fit_file = "fit.tsv";
        CHECK(!plan_ext_reports(&e3.v2.v1, 2, false, rp, err) && err.find("strain_fit_file") != std::string::npos);
        CHECK(plan_ext_reports(&e3.v2.v1, 1, false, rp, err) && rp.ext_want[XREP_FIT] && rp.ext2_want[X2REP_BOOTSTRAP] && rp.ext3_want[X3REP_DROPOUT]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes
        e3.v2.v1.struct_size = 16;
        CHECK(plan_ext_reports(&e3.v2.v1, 1, false, rp, err) && rp.ext_want[XREP_FIT] && !rp.ext2_want[X2REP_BOOTSTRAP] && !rp.ext3_want[X3REP_DROPOUT] && rp.ext3_path[X3REP_DROPOUT].empty());
        e3.v2.v1.struct_size = 40;
        CHECK(plan_ext_reports(&e3.v2.v1, 1, false, rp, err) && rp.ext2_want[X2REP_BOOTSTRAP] && !rp.ext3_want[X3REP_DROPOUT]);
        CHECK(plan_ext_reports(&e3.v2.v1, 2, false, rp, err) == false && err.find("strain_dropout_file") == std::string::npos);   // (refused for the two it holds, not for this one)
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e3.v2.v1.struct_size = sizeof(e3); e3.strain_dropout_file = off;
            e3.v2.v1.strain_fit_file = nullptr; e3.v2.strain_bootstrap_file = nullptr;
            CHECK(plan_ext_reports(&e3.v2.v1, 2, true, rp, err) && !rp.ext3_want[X3REP_DROPOUT]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext3_want[X3REP_DROPOUT]);
    }
    std::printf("dropout_plan_check: ok\n");
    return 0;
}
