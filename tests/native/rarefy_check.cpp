// rarefy_check.cpp -- the host side of pantax_hip_strain_rarefy at its edges: the cut of a replicate's levels into passes (rarefy_plan), the entry of a
// (replicate, level), the depth rule's host helper on values that follow from the rule alone, and the report's row in the plan of the file seam.  A program
// of its own: tests/test_rarefy_plan.py compiles it with rarefy_plan.cpp and report_plan.cpp by the host C++ compiler under
// -fsanitize=address,undefined and runs it; it returns non-zero at the first check that fails.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include "../../include/pantax_hip.h"
#include "rarefy_depth.hpp"
#include "rarefy_plan.hpp"
#include "report_plan.hpp"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "rarefy_check:%d: %s\n", __LINE__, #cond);         \
            return 1;                                                               \
        }                                                                           \
    } while (0)

using namespace ptx;

int main() {
    // ---- the level cut
    {
        RarefyPlan p;
        std::string why;
        CHECK(rarefy_plan(5, 100, 0, p, why) && p.per_pass == 5 && p.n_passes == 1);           // everything fits: one pass a replicate
        CHECK(rarefy_plan(5, 2, 0, p, why) && p.per_pass == 2 && p.n_passes == 3);             // the memory holds two arrays
        CHECK(rarefy_plan(5, 100, 2, p, why) && p.per_pass == 2 && p.n_passes == 3);           // the option caps it
        CHECK(rarefy_plan(5, 1, 3, p, why) && p.per_pass == 1 && p.n_passes == 5);             // the smaller of the two
        CHECK(rarefy_plan(16, 16, 0, p, why) && p.per_pass == 16 && p.n_passes == 1);
        CHECK(rarefy_plan(16, 5, 0, p, why) && p.per_pass == 5 && p.n_passes == 4);
        CHECK(rarefy_plan(1, 1, 1, p, why) && p.per_pass == 1 && p.n_passes == 1);
        CHECK(rarefy_plan(3, 100, 100, p, why) && p.per_pass == 3 && p.n_passes == 1);         // never more than the levels asked for
        CHECK(!rarefy_plan(5, 0, 0, p, why) && why.find("level array") != std::string::npos && p.per_pass == 0);   // not one array fits
        CHECK(!rarefy_plan(0, 100, 0, p, why) && !rarefy_plan(17, 100, 0, p, why) && why.find("17 levels") != std::string::npos);
        // the passes of a replicate cover the levels 1 .. n once, in order
        CHECK(rarefy_plan(5, 2, 0, p, why));
        uint32_t l0 = 0, l1 = 0, next = 1;
        for (uint32_t i = 0; i < p.n_passes; ++i) {
            rarefy_pass_levels(p, 5, i, l0, l1);
            CHECK(l0 == next && l1 > l0 && l1 - l0 <= p.per_pass);
            next = l1;
        }
        CHECK(next == 6);
        CHECK(rarefy_plan(16, 5, 0, p, why));
        rarefy_pass_levels(p, 16, 3, l0, l1);
        CHECK(l0 == 16 && l1 == 17);
        CHECK(RAREFY_MAX_LEVELS == 16);
        CHECK(rarefy_default_arrays((size_t)64 << 20, 1 << 20) == 2 && rarefy_default_arrays((size_t)1 << 20, 1 << 20) == 0 && rarefy_default_arrays(0, 0) == 16);
        CHECK(rarefy_entry(5, 1, 1) == 1 && rarefy_entry(5, 1, 5) == 5 && rarefy_entry(5, 2, 1) == 6 && rarefy_entry(12, 3, 12) == 36);
    }
    // ---- the depth rule: the helper is the header's rule, 63 at the most, and a read's depth is a function of (seed, replicate, read) alone
    {
        CHECK(boot_sm(0) == 0xE220A8397B1DCDAFull);   // splitmix64's first output from state 0
        uint64_t hist[64] = {};
        for (uint64_t r = 0; r < 4096; ++r) {
            const uint32_t d = pantax_hip_rarefy_depth(42, 1, r);
            CHECK(d <= RAREFY_DEPTH_MAX && d == rarefy_depth_hashed(rarefy_replicate_hash(42, 1), r));
            const uint64_t h = boot_sm(boot_sm(42ull ^ boot_sm(1)) + r);
            CHECK(d >= 63 || ((h >> (63 - d)) & 1ull));          // the bit behind the leading zeros is set ...
            CHECK(d == 0 || (h >> (64 - d)) == 0);               // ... and the bits in front of it are not
            ++hist[d];
        }
        CHECK(hist[0] > 1800 && hist[0] < 2300 && hist[1] > 850 && hist[1] < 1200);
        CHECK(pantax_hip_rarefy_depth(42, 1, (1ull << 32) + 7) == rarefy_depth_hashed(rarefy_replicate_hash(42, 1), (1ull << 32) + 7));
    }
    // ---- the report's row in the plan of the file seam: pantax_hip_profile_ext10 behind the 168-byte ninth version
    {
        static_assert(offsetof(pantax_hip_profile_ext10, v9) == 0 && sizeof(pantax_hip_profile_ext9) == 168 && sizeof(pantax_hip_profile_ext8) == 152 &&
                          sizeof(pantax_hip_profile_ext7) == 136 && sizeof(pantax_hip_profile_ext6) == 120 && sizeof(pantax_hip_profile_ext5) == 88 &&
                          sizeof(pantax_hip_profile_ext4) == 64 && sizeof(pantax_hip_profile_ext3) == 48 && sizeof(pantax_hip_profile_ext2) == 40 &&
                          sizeof(pantax_hip_profile_ext) == 16,
                      "the earlier versions keep their size");
        static_assert(offsetof(pantax_hip_profile_ext10, strain_rarefy_file) == 168 && offsetof(pantax_hip_profile_ext10, strain_rarefy_levels) == 176 &&
                          offsetof(pantax_hip_profile_ext10, strain_rarefy_replicates) == 184 && offsetof(pantax_hip_profile_ext10, strain_rarefy_seed) == 192 &&
                          sizeof(pantax_hip_profile_ext10) == 200,
                      "the layout of the tenth version");
        CHECK(N_EXT10_REPORTS == 1 && EXT10_REPORTS[X10REP_RAREFY].field == &pantax_hip_profile_ext10::strain_rarefy_file && EXT10_REPORTS[X10REP_RAREFY].rows);
        CHECK(std::string(EXT10_REPORTS[X10REP_RAREFY].name) == "strain_rarefy_file" && std::string(EXT10_REPORTS[X10REP_RAREFY].what) == "rarefaction report");
        CHECK(N_EXT9_REPORTS == 1 && N_EXT8_REPORTS == 1 && N_EXT7_REPORTS == 1 && N_EXT6_REPORTS == 1 && N_EXT5_REPORTS == 1 && N_EXT4_REPORTS == 1 &&
              N_EXT3_REPORTS == 1 && N_EXT2_REPORTS == 1 && N_EXT_REPORTS == 1);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        std::string err;
        pantax_hip_profile_ext10 e10{};
        pantax_hip_profile_ext *e1 = &e10.v9.v8.v7.v6.v5.v4.v3.v2.v1;
        e1->struct_size = sizeof(e10);
        e10.strain_rarefy_file = "rf.tsv";
        e10.strain_rarefy_seed = 42;
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(e1, 1, false, rp, err));
        CHECK(rp.ext10_want[X10REP_RAREFY] && !rp.ext10_run[X10REP_RAREFY] && rp.ext10_path[X10REP_RAREFY] == "rf.tsv" && !rp.ext9_want[X9REP_LINKS]);
        CHECK(rp.rf_levels == 5 && rp.rf_replicates == 5 && rp.rf_seed == 42);                 // 0 reads as the default
        resume_reports(rp, true, true, false);
        CHECK(rp.ext10_run[X10REP_RAREFY] && rp.any_run() && rp.rows_run() && !rp.ext9_run[X9REP_LINKS]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext10_run[X10REP_RAREFY] && !rp.any_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext10_run[X10REP_RAREFY]);
        resume_reports(rp, true, false, true);                                                 // the strain-only resume writes it
        CHECK(rp.ext10_run[X10REP_RAREFY]);
        e10.strain_rarefy_levels = 12; e10.strain_rarefy_replicates = 3; e10.strain_rarefy_seed = 0;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.rf_levels == 12 && rp.rf_replicates == 3 && rp.rf_seed == 0);   // a seed of 0 passed explicitly is 0
        e10.strain_rarefy_levels = 16;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.rf_levels == 16);
        e10.strain_rarefy_levels = 17;                                                         // beyond the stage call's limit: refused
        CHECK(!plan_ext_reports(e1, 1, false, rp, err) && err == "profile: strain_rarefy_levels 17 (at most 16)");
        e10.strain_rarefy_levels = 4;
        e10.strain_rarefy_replicates = 1ull << 28;
        CHECK(!plan_ext_reports(e1, 1, false, rp, err) && err.find("strain_rarefy_replicates") != std::string::npos);
        e10.strain_rarefy_replicates = 7; e10.strain_rarefy_seed = 9;
        e1->struct_size = 192;                                                                 // a struct without the seed: 42
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.rf_levels == 4 && rp.rf_replicates == 7 && rp.rf_seed == 42);
        e1->struct_size = 184;                                                                 // ... without the replicates: 5
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.rf_levels == 4 && rp.rf_replicates == 5 && rp.rf_seed == 42);
        e1->struct_size = 176;                                                                 // the file alone: the defaults
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext10_want[X10REP_RAREFY] && rp.rf_levels == 5 && rp.rf_replicates == 5 && rp.rf_seed == 42);
        e1->struct_size = sizeof(e10);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.rf_seed == 9);
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err == "profile: the rarefaction report (strain_rarefy_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(e1, 1, true, rp, err) && err == "profile: the rarefaction report (strain_rarefy_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e10.v9.strain_links_file = "lk.tsv";                                                   // the link support report's refusal comes first
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err.find("strain_links_file") != std::string::npos);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext9_want[X9REP_LINKS] && rp.ext10_want[X10REP_RAREFY]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes, the link support report on where it is held
        for (const uint64_t size : {16ull, 40ull, 48ull, 64ull, 88ull, 120ull, 136ull, 152ull, 160ull, 168ull}) {
            e1->struct_size = size;
            CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext10_want[X10REP_RAREFY] && rp.ext10_path[X10REP_RAREFY].empty() && rp.rf_levels == 5);
            CHECK(rp.ext9_want[X9REP_LINKS] == (size >= 160));
        }
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e1->struct_size = sizeof(e10); e10.strain_rarefy_file = off; e10.v9.strain_links_file = nullptr;
            CHECK(plan_ext_reports(e1, 2, true, rp, err) && !rp.ext10_want[X10REP_RAREFY]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext10_want[X10REP_RAREFY]);
    }
    std::printf("rarefy_check: ok\n");
    return 0;
}
