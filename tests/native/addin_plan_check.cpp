// addin_plan_check.cpp -- the host side of pantax_hip_strain_addin at its edges: the plan of the chunks of rounds, the index arithmetic of the outputs and
// the choice of the objective pass's instance (pantax_amd/csrc/addin_plan.hpp), the donor helper, and the report's row in the plan of the file seam.  A
// program of its own: tests/test_addin_plan.py compiles it with addin_plan.cpp and report_plan.cpp by the host C++ compiler under
// -fsanitize=address,undefined and runs it; it returns non-zero at the first check that fails.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "addin_plan.hpp"
#include "report_plan.hpp"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "addin_plan_check:%d: %s\n", __LINE__, #cond);     \
            return 1;                                                               \
        }                                                                           \
    } while (0)

using namespace ptx;

int main() {
    AddinPlan pl;
    std::string err;
    // ---- the plan: one round (J = 0 everywhere: entry 0 alone), all rounds in one chunk, and never more than there are
    CHECK(addin_plan(1000, 9, 1, 1u << 20, pl, err));
    CHECK(pl.per_chunk == 1 && pl.n_chunks == 1 && pl.chunk_patterns == 1001 && pl.chunk_entries == 10);
    CHECK(addin_plan(1000, 9, 65, 1u << 20, pl, err));
    CHECK(pl.per_chunk == 65 && pl.n_chunks == 1 && pl.chunk_patterns == 65 * 1001 && pl.chunk_entries == 650);
    // a cap of exactly one round (P patterns and the closing slot), of exactly two, one below three, and one below one
    CHECK(addin_plan(1000, 9, 65, 1001, pl, err) && pl.per_chunk == 1 && pl.n_chunks == 65 && pl.chunk_patterns == 1001);
    CHECK(addin_plan(1000, 9, 65, 2002, pl, err) && pl.per_chunk == 2 && pl.n_chunks == 33 && pl.chunk_entries == 20);
    CHECK(addin_plan(1000, 9, 65, 3002, pl, err) && pl.per_chunk == 2);
    CHECK(addin_plan(1000, 9, 6, 2002, pl, err) && pl.per_chunk == 2 && pl.n_chunks == 3);
    CHECK(addin_plan(1000, 9, 3, 2002, pl, err) && pl.per_chunk == 2 && pl.n_chunks == 2);   // the last chunk holds one
    err.clear();
    CHECK(!addin_plan(1000, 9, 65, 1000, pl, err));
    CHECK(err.find("addin_patterns_max") != std::string::npos && err.find("1000 patterns") != std::string::npos && pl.per_chunk == 0);
    CHECK(!addin_plan(1000, 9, 65, 0, pl, err));
    // no pattern at all: nothing to size, one chunk, whatever the cap
    CHECK(addin_plan(0, 9, 65, 0, pl, err) && pl.per_chunk == 65 && pl.n_chunks == 1 && pl.chunk_patterns == 0 && pl.chunk_entries == 0);
    // no round, and more than the 65 a species of 64 candidates has
    CHECK(!addin_plan(10, 1, 0, 1000, pl, err));
    CHECK(!addin_plan(10, 1, 66, 1000, pl, err));
    // u64 sizes: the cap is cut to 32-bit pattern positions; the entries of a chunk stay 32-bit; patterns or species beyond them are refused
    CHECK(addin_plan(1u << 20, 3, 65, ~0ull, pl, err) && pl.per_chunk == 65 && pl.chunk_patterns <= ADDIN_PATTERNS_HARD_MAX);
    CHECK(addin_plan(4000000000ull, 3, 65, ~0ull, pl, err) && pl.per_chunk == 1 && pl.n_chunks == 65);
    CHECK(addin_plan(10, 4000000000ull, 65, ~0ull, pl, err) && pl.per_chunk == 1 && pl.chunk_entries == 4000000001ull);
    CHECK(addin_plan(10, 1u << 30, 65, ~0ull, pl, err) && pl.per_chunk == 3 && (uint64_t)pl.per_chunk * ((1ull << 30) + 1) <= ADDIN_PATTERNS_HARD_MAX);
    CHECK(!addin_plan(1ull << 32, 3, 2, ~0ull, pl, err));
    CHECK(!addin_plan(~0ull, 3, 2, ~0ull, pl, err));
    CHECK(!addin_plan(ADDIN_PATTERNS_HARD_MAX, 3, 2, ~0ull, pl, err));
    CHECK(!addin_plan(10, 1ull << 32, 2, ~0ull, pl, err));
    // the default cap: a quarter of the free memory in patterns, cut to 32-bit positions
    CHECK(addin_default_cap(0) == 0);
    CHECK(addin_default_cap(4 * ADDIN_BYTES_PER_PATTERN * 1000 + 5) == 1000);
    CHECK(addin_default_cap(~0ull) == ADDIN_PATTERNS_HARD_MAX);
    // ---- entries and x blocks: (K, J) = (0, 0), (4, 0), (0, 1), (32, 32), (60, 5), (0, 64) side by side
    {
        const uint64_t sel_off[7] = {0, 0, 4, 4, 36, 96, 96}, cand_off[7] = {0, 0, 0, 1, 33, 38, 102};
        uint64_t x_off[7];
        CHECK(addin_x_offsets(6, sel_off, cand_off, x_off));
        CHECK(x_off[0] == 0 && x_off[1] == 0 && x_off[2] == 4 && x_off[3] == 4 + 2 && x_off[4] == 6 + 33 * 64 && x_off[5] == 6 + 33 * 64 + 6 * 65);
        CHECK(x_off[6] == 6 + 33 * 64 + 6 * 65 + 65 * 64);
        CHECK(addin_entry(cand_off[0], 0, 0) == 0);                                             // W = 0: the one entry
        CHECK(addin_entry(cand_off[1], 1, 0) == 1);                                             // J = 0: entry 0 alone
        CHECK(addin_entry(cand_off[2], 2, 0) == 2 && addin_entry(cand_off[2], 2, 1) == 3);      // K = 0, J = 1: two
        CHECK(addin_entry(cand_off[3], 3, 0) == 4 && addin_entry(cand_off[3], 3, 32) == 36);
        CHECK(addin_entry(cand_off[4], 4, 0) == 37 && addin_entry(cand_off[4], 4, 5) == 42);
        CHECK(addin_entry(cand_off[5], 5, 0) == 43 && addin_entry(cand_off[5], 5, 64) == 107);
        CHECK(addin_entry(cand_off[6], 6, 0) == 102 + 6);                                       // Q = J + S: one beyond the last entry
        const uint64_t none[1] = {0};
        CHECK(addin_x_offsets(0, none, none, x_off) && x_off[0] == 0);
        const uint64_t zero[2] = {0, 0}, huge[2] = {0, 1ull << 33}, all[2] = {0, ~0ull};
        CHECK(!addin_x_offsets(1, zero, huge, x_off));                                          // (2^33 + 1) 2^33 passes 2^64
        CHECK(addin_x_offsets(1, huge, zero, x_off) && x_off[1] == 1ull << 33);                 // J = 0: one entry of K columns
        CHECK(!addin_x_offsets(1, all, all, x_off) && !addin_x_offsets(1, zero, all, x_off));   // K + J, J + 1 beyond 64 bits
        const uint64_t big[2] = {0, (1ull << 32) - 1};                                          // 2^32 (2^32 - 1) does not
        CHECK(addin_x_offsets(1, zero, big, x_off) && x_off[1] == ((1ull << 32) - 1) << 32);
    }
    // ---- the instance of the objective pass is a function of W and E alone; the slice of the instance
    CHECK(addin_instance(1, 1) == ADDIN_TABLE && addin_instance(1, 2) == ADDIN_TABLE && addin_instance(7, 8) == ADDIN_TABLE && addin_instance(7, 1) == ADDIN_TABLE);
    CHECK(addin_instance(8, 6) == ADDIN_FEW && addin_instance(8, 1) == ADDIN_FEW && addin_instance(64, 1) == ADDIN_FEW && addin_instance(64, 8) == ADDIN_FEW && addin_instance(8, 8) == ADDIN_FEW);
    CHECK(addin_instance(8, 9) == ADDIN_WIDE && addin_instance(32, 17) == ADDIN_WIDE && addin_instance(64, 33) == ADDIN_WIDE && addin_instance(64, 65) == ADDIN_WIDE);
    CHECK(addin_slice_rows(1, 1) == ADDIN_SLICE_TABLE && addin_slice_rows(7, 8) == ADDIN_SLICE_TABLE && addin_slice_rows(8, 6) == ADDIN_SLICE_FEW && addin_slice_rows(64, 1) == ADDIN_SLICE_FEW);
    CHECK(addin_slice_rows(8, 9) == ADDIN_SLICE_WIDE && addin_slice_rows(64, 65) == ADDIN_SLICE_WIDE && ADDIN_SLICE_TABLE == 16384 && ADDIN_SLICE_FEW == 4096 && ADDIN_SLICE_WIDE == 4096);
    CHECK(addin_slices(0, 2, 2) == 0 && addin_slices(1, 2, 2) == 1 && addin_slices(ADDIN_SLICE_TABLE, 2, 2) == 1 && addin_slices(ADDIN_SLICE_TABLE + 1, 2, 2) == 2);
    CHECK(addin_slices(ADDIN_SLICE_FEW, 9, 6) == 1 && addin_slices(ADDIN_SLICE_FEW + 1, 9, 6) == 2);
    CHECK(addin_slices(ADDIN_SLICE_WIDE, 64, 65) == 1 && addin_slices(ADDIN_SLICE_WIDE + 1, 64, 65) == 2 && addin_slices(~0ull, 64, 65) == (~0ull) / ADDIN_SLICE_WIDE + 1);
    CHECK(ADDIN_MAX_W == 64);
    // ---- the donor
    double out[3];
    const double b4[4] = {1.0, 2.0, 3.0, 0.0};
    const double one[4] = {0.5, 2.0, 2.0, 1.5};                   // column 2 loses 1, column 0 half of that
    CHECK(pantax_hip_addin_donor(4, 3, b4, one, nullptr) == PANTAX_HIP_E_INVALID);
    CHECK(pantax_hip_addin_donor(4, 3, nullptr, one, out) == PANTAX_HIP_E_INVALID && pantax_hip_addin_donor(4, 3, b4, nullptr, out) == PANTAX_HIP_E_INVALID);
    CHECK(pantax_hip_addin_donor(4, 5, b4, one, out) == PANTAX_HIP_E_INVALID);
    CHECK(pantax_hip_addin_donor(4, 3, b4, one, out) == 0 && out[0] == 2.0 && out[1] == 1.0 && out[2] == 1.5);
    const double tie[4] = {0.5, 1.5, 3.0, 1.0};                   // columns 0 and 1 lose 0.5 each: the lowest of the tie
    CHECK(pantax_hip_addin_donor(4, 3, b4, tie, out) == 0 && out[0] == 0.0 && out[1] == 0.5 && out[2] == 1.0);
    const double gainer[4] = {1.0, 2.5, 3.25, 0.5};               // nobody loses: -1, loss 0, the shift still counts the gains
    CHECK(pantax_hip_addin_donor(4, 3, b4, gainer, out) == 0 && out[0] == -1.0 && out[1] == 0.0 && out[2] == 0.75);
    CHECK(pantax_hip_addin_donor(4, 3, b4, b4, out) == 0 && out[0] == -1.0 && out[2] == 0.0);   // no difference is no positive loss
    const double cand_only[4] = {1.0, 2.0, 3.0, 9.0};             // the candidate columns are not looked at
    CHECK(pantax_hip_addin_donor(4, 3, b4, cand_only, out) == 0 && out[0] == -1.0 && out[2] == 0.0);
    CHECK(pantax_hip_addin_donor(4, 0, b4, one, out) == 0 && out[0] == -1.0 && out[1] == 0.0 && out[2] == 0.0);   // K = 0: nobody to take from
    CHECK(pantax_hip_addin_donor(0, 0, b4, one, out) == 0 && out[0] == -1.0);
    CHECK(pantax_hip_addin_donor(4, 4, b4, one, out) == 0 && out[0] == 2.0 && out[2] == 3.0);                       // K = W: every column is a reported one
    // ---- the report in the file seam's plan: a field of pantax_hip_profile_ext4, which begins with the 48-byte third version; the one row of EXT4_REPORTS
    {
        static_assert(offsetof(pantax_hip_profile_ext4, v3) == 0 && sizeof(pantax_hip_profile_ext3) == 48 && sizeof(pantax_hip_profile_ext2) == 40 && sizeof(pantax_hip_profile_ext) == 16,
                      "the earlier versions keep their place and size");
        static_assert(offsetof(pantax_hip_profile_ext4, strain_addin_file) == 48 && offsetof(pantax_hip_profile_ext4, strain_addin_top) == 56 && sizeof(pantax_hip_profile_ext4) == 64,
                      "appended behind them");
        CHECK(N_EXT4_REPORTS == 1 && EXT4_REPORTS[X4REP_ADDIN].field == &pantax_hip_profile_ext4::strain_addin_file && !EXT4_REPORTS[X4REP_ADDIN].rows);
        CHECK(std::string(EXT4_REPORTS[X4REP_ADDIN].name) == "strain_addin_file" && std::string(EXT4_REPORTS[X4REP_ADDIN].what) == "add-one report");
        CHECK(N_EXT3_REPORTS == 1 && N_EXT2_REPORTS == 1 && N_EXT_REPORTS == 1);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        pantax_hip_profile_ext4 e4{};
        pantax_hip_profile_ext *e1 = &e4.v3.v2.v1;
        e1->struct_size = sizeof(e4);
        e4.strain_addin_file = "addin.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(e1, 1, false, rp, err));
        CHECK(rp.ext4_want[X4REP_ADDIN] && !rp.ext4_run[X4REP_ADDIN] && rp.ext4_path[X4REP_ADDIN] == "addin.tsv" && rp.ai_top == 5 && !rp.ext3_want[X3REP_DROPOUT]);
        resume_reports(rp, true, true, false);
        CHECK(rp.ext4_run[X4REP_ADDIN] && rp.any_run() && !rp.rows_run() && !rp.ext3_run[X3REP_DROPOUT]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext4_run[X4REP_ADDIN] && !rp.any_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext4_run[X4REP_ADDIN]);
        e4.strain_addin_top = 1;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ai_top == 1);
        e4.strain_addin_top = 1ull << 40;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ai_top == 0xFFFFFFFFu);
        e1->struct_size = 56;                                          // a struct that holds the file but not the top: 5
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext4_want[X4REP_ADDIN] && rp.ai_top == 5);
        e1->struct_size = sizeof(e4); e4.strain_addin_top = 0;
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err == "profile: the add-one report (strain_addin_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(e1, 1, true, rp, err) && err == "profile: the add-one report (strain_addin_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e4.v3.strain_dropout_file = "drop.tsv";                         // the leave-one-out report's refusal comes first
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err.find("strain_dropout_file") != std::string::npos);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext3_want[X3REP_DROPOUT] && rp.ext4_want[X4REP_ADDIN]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes, the leave-one-out report on where it is held
        for (const uint64_t size : {16ull, 40ull, 48ull}) {
            e1->struct_size = size;
            CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext4_want[X4REP_ADDIN] && rp.ext4_path[X4REP_ADDIN].empty() && rp.ai_top == 5);
            CHECK(rp.ext3_want[X3REP_DROPOUT] == (size == 48));
        }
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e1->struct_size = sizeof(e4); e4.strain_addin_file = off; e4.v3.strain_dropout_file = nullptr;
            CHECK(plan_ext_reports(e1, 2, true, rp, err) && !rp.ext4_want[X4REP_ADDIN]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext4_want[X4REP_ADDIN]);
    }
    std::printf("addin_plan_check: ok\n");
    return 0;
}
