// read_em_check.cpp -- the host side of pantax_hip_strain_read_em at its edges: the sizing and growth of the class tables and the ranking of a species'
// classes for the report (pantax_amd/csrc/read_em_plan.hpp), the host helper of the estimate on cases done by hand, and the report's row in the plan of the
// file seam.  A program of its own: tests/test_read_em_plan.py compiles it with read_em_plan.cpp and report_plan.cpp by the host C++ compiler under
// -fsanitize=address,undefined and runs it; it returns non-zero at the first check that fails.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "read_em_plan.hpp"
#include "report_plan.hpp"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "read_em_check:%d: %s\n", __LINE__, #cond);        \
            return 1;                                                               \
        }                                                                           \
    } while (0)

using namespace ptx;

int main() {
    // ---- slots of a species' class table: the power of two >= 2 min(2^K - 1, read_class_slots)
    CHECK(read_class_pow2(0) == 1 && read_class_pow2(1) == 1 && read_class_pow2(2) == 2 && read_class_pow2(3) == 4 && read_class_pow2(1ull << 63) == 1ull << 63);
    CHECK(read_class_slots(0, 0) == 0 && read_class_slots(65, 0) == 0 && read_class_slots(1000, 0) == 0);   // no candidates, a skipped species
    CHECK(read_class_slots(1, 0) == 2);                                      // one class at most
    CHECK(read_class_slots(6, 0) == 128 && read_class_slots(7, 0) == 256);    // 2 x 63 -> 128; 2 x 127 -> 256
    CHECK(read_class_slots(10, 0) == 2048 && read_class_slots(11, 0) == 4096 && read_class_slots(12, 0) == 4096);   // 2 x 1023; 2 x 2047; the cap of 2048
    CHECK(read_class_slots(63, 0) == 4096 && read_class_slots(64, 0) == 4096);
    CHECK(read_class_slots(1, 1) == 2 && read_class_slots(6, 1) == 2 && read_class_slots(64, 1) == 2);
    CHECK(read_class_slots(1, 2) == 2 && read_class_slots(2, 2) == 4 && read_class_slots(64, 2) == 4);
    CHECK(read_class_slots(1, 1ull << 31) == 2 && read_class_slots(7, 1ull << 31) == 256 && read_class_slots(31, 1ull << 31) == 1ull << 32);
    CHECK(read_class_slots(32, 1ull << 31) == 1ull << 32 && read_class_slots(63, 1ull << 31) == 1ull << 32 && read_class_slots(64, 1ull << 31) == 1ull << 32);
    CHECK(read_class_slots(64, ~0ull) == 1ull << 32 && read_class_slots(64, (1ull << 31) + 1) == 1ull << 32);   // the option is cut to 2^31
    // ---- the growth: eightfold, up to the bound 2 min(2^K - 1, counted) rounded up, where overflow is impossible
    CHECK(read_class_slots_bound(0, 100) == 0 && read_class_slots_bound(65, 100) == 0);
    CHECK(read_class_slots_bound(1, 100) == 2 && read_class_slots_bound(6, 1000) == 128 && read_class_slots_bound(6, 10) == 32 && read_class_slots_bound(64, 161) == 512);
    CHECK(read_class_slots_bound(64, 0) == 2 && read_class_slots_bound(64, 1) == 2 && read_class_slots_bound(64, ~0ull) == 1ull << 63 && read_class_slots_bound(63, ~0ull) == 1ull << 63);
    CHECK(read_class_grow(4, 64, 3000) == 32 && read_class_grow(32, 64, 3000) == 256 && read_class_grow(256, 64, 3000) == 2048 && read_class_grow(2048, 64, 3000) == 8192);
    CHECK(read_class_grow(8192, 64, 3000) == 8192);                          // at the bound: no further (the caller's internal error)
    CHECK(read_class_grow(4096, 64, 3000) == 8192 && read_class_grow(1024, 64, 3000) == 8192 && read_class_grow(1023, 64, 3000) == 8184);
    CHECK(read_class_grow(2, 1, 10) == 2 && read_class_grow(4, 2, 2) == 4 && read_class_grow(2, 2, 5) == 8);
    CHECK(read_class_grow(1ull << 62, 64, ~0ull) == 1ull << 63 && read_class_grow(1ull << 63, 64, ~0ull) == 1ull << 63 && read_class_grow(1ull << 59, 64, ~0ull) == 1ull << 62);
    {
        // the loop of reruns is bounded: from the smallest table to the largest bound
        uint64_t slots = 2;
        int n = 0;
        for (;; ++n) {
            const uint64_t next = read_class_grow(slots, 64, ~0ull);
            if (next == slots) break;
            CHECK(next > slots);
            slots = next;
        }
        CHECK(slots == 1ull << 63 && n == 21);
        // a table at its bound holds every class the species can have, at most half full
        for (uint64_t K = 1; K <= 64; ++K)
            for (const uint64_t counted : {1ull, 2ull, 100ull, 1ull << 20}) {
                const uint64_t classes = std::min(read_class_masks(K), counted);
                CHECK(read_class_slots_bound(K, counted) >= 2 * classes && read_class_slots_bound(K, counted) < 4 * classes + 2);
            }
    }
    CHECK(READ_EM_MAX_K == 64 && READ_CLASS_SLOTS_DEFAULT == 2048 && READ_EM_LDS_CLASSES == 2048);
    // ---- the classes the report prints: span descending, ties by mask ascending; J below, at and above N
    {
        const uint64_t mask[6] = {1, 2, 3, 5, 6, 7}, span[6] = {10, 40, 10, 40, 0, 25};
        typedef std::vector<uint64_t> V;
        CHECK(read_class_rank(6, mask, span, 10) == (V{1, 3, 5, 0, 2, 4}));       // J below N: all, the ties (2, 5) and (1, 3) by mask
        CHECK(read_class_rank(6, mask, span, 6) == (V{1, 3, 5, 0, 2, 4}));        // J at N
        CHECK(read_class_rank(6, mask, span, 4) == (V{1, 3, 5, 0}));              // J above N: the tie at the cut goes to the lower mask
        CHECK(read_class_rank(6, mask, span, 1) == (V{1}));
        CHECK(read_class_rank(6, mask, span, 0).empty() && read_class_rank(0, nullptr, nullptr, 3).empty());
        CHECK(read_class_rank(1, mask, span, ~0ull) == (V{0}));
    }
    // ---- the helper on the cases done by hand (tests/test_read_em_ref.py)
    {
        double x[64], delta = -1.0;
        uint32_t it = 99;
        int32_t cv = -1;
        const uint64_t m1[1] = {1}, b1[1] = {100}, g1[1] = {50};
        CHECK(pantax_hip_read_em(1, 1, m1, b1, g1, 1000, 1e-6, x, &it, &cv, &delta) == 0 && x[0] == 2.0 && it == 2 && cv == 1 && delta == 0.0);
        const uint64_t m2[2] = {1, 2}, b2[2] = {300, 70}, g2[2] = {100, 7};
        CHECK(pantax_hip_read_em(2, 2, m2, b2, g2, 1000, 1e-6, x, &it, &cv, &delta) == 0 && x[0] == 3.0 && x[1] == 10.0 && it == 2 && cv == 1);
        CHECK(pantax_hip_read_em(2, 2, m2, b2, g2, 1, 1e-6, x, &it, &cv, &delta) == 0 && x[0] == 3.0 && x[1] == 10.0 && it == 1 && cv == 0 && delta == 9.0);
        const uint64_t m3[1] = {3}, b3[1] = {600}, g3[2] = {100, 100};
        CHECK(pantax_hip_read_em(2, 1, m3, b3, g3, 1000, 1e-6, x, &it, &cv, &delta) == 0 && x[0] == 3.0 && x[1] == 3.0 && cv == 1);
        const uint64_t m4[2] = {1, 3}, b4[2] = {0, 0}, g4[2] = {10, 20};
        CHECK(pantax_hip_read_em(2, 2, m4, b4, g4, 1000, 1e-6, x, &it, &cv, &delta) == 0 && x[0] == 0.0 && x[1] == 0.0 && it == 2 && cv == 1 && delta == 0.0);
        const uint64_t m5[3] = {1, 2, 3}, b5[3] = {100, 55, 40}, g5[2] = {70, 0};      // G = 0, and a class whose only member is at 0
        CHECK(pantax_hip_read_em(2, 3, m5, b5, g5, 1000, 1e-6, x, &it, &cv, &delta) == 0 && x[0] == 2.0 && x[1] == 0.0 && cv == 1);
        const uint64_t b6[2] = {1000, 10}, g6[2] = {100, 100};                          // the floor: the dying strain ends at exactly 0
        CHECK(pantax_hip_read_em(2, 2, m4, b6, g6, 300, 0.0, x, &it, &cv, &delta) == 0 && x[1] == 0.0 && std::fabs(x[0] - 10.1) < 1e-12 && it > 50);
        CHECK(pantax_hip_read_em(2, 2, m4, b6, g6, 1000, 1e-6, x, &it, &cv, &delta) == 0 && x[1] > 0.0 && x[1] < 1e-6 && cv == 1 && it < 10);
        CHECK(pantax_hip_read_em(2, 0, nullptr, nullptr, g6, 7, 0.0, x, &it, &cv, &delta) == 0 && x[0] == 0.0 && x[1] == 0.0 && it == 2 && cv == 1);   // no class
        CHECK(pantax_hip_read_em(0, 0, nullptr, nullptr, nullptr, 3, 0.0, nullptr, &it, &cv, &delta) == 0 && it == 1 && cv == 1);
        uint64_t g64[64], m64[2] = {1ull << 63, ~0ull}, b64[2] = {640, 6400};
        for (int k = 0; k < 64; ++k) g64[k] = 10;
        CHECK(pantax_hip_read_em(64, 2, m64, b64, g64, 1000, 1e-6, x, &it, &cv, &delta) == 0 && cv == 1 && x[63] > x[0] && x[0] == x[62]);   // bit 63
        double mass = 0.0;
        for (int k = 0; k < 64; ++k) mass += x[k] * 10.0;
        CHECK(std::fabs(mass - 7040.0) <= 1e-9 * 7040.0);
        // refusals
        CHECK(pantax_hip_read_em(65, 1, m1, b1, g64, 5, 0.0, x, &it, &cv, &delta) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_read_em(1, 1, m1, b1, g1, 0, 0.0, x, &it, &cv, &delta) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_read_em(1, 1, m1, b1, g1, 5, -1.0, x, &it, &cv, &delta) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_read_em(1, 1, m1, b1, g1, 5, NAN, x, &it, &cv, &delta) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_read_em(1, 1, m1, b1, g1, 5, INFINITY, x, &it, &cv, &delta) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_read_em(1, 1, m2 + 1, b1, g1, 5, 0.0, x, &it, &cv, &delta) == PANTAX_HIP_E_INVALID);    // bit 1 of one candidate
        CHECK(pantax_hip_read_em(1, 1, nullptr, b1, g1, 5, 0.0, x, &it, &cv, &delta) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_read_em(1, 1, m1, b1, g1, 5, 0.0, nullptr, &it, &cv, &delta) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_read_em(1, 1, m1, b1, g1, 5, 0.0, x, nullptr, &cv, &delta) == PANTAX_HIP_E_INVALID);
    }
    // ---- the report in the file seam's plan: three fields of pantax_hip_profile_ext5, which begins with the 64-byte fourth version; the one row of EXT5_REPORTS
    {
        static_assert(offsetof(pantax_hip_profile_ext5, v4) == 0 && sizeof(pantax_hip_profile_ext4) == 64 && sizeof(pantax_hip_profile_ext3) == 48 &&
                          sizeof(pantax_hip_profile_ext2) == 40 && sizeof(pantax_hip_profile_ext) == 16,
                      "the earlier versions keep their place and size");
        static_assert(offsetof(pantax_hip_profile_ext5, strain_em_file) == 64 && offsetof(pantax_hip_profile_ext5, strain_em_classes) == 72 &&
                          offsetof(pantax_hip_profile_ext5, strain_em_iterations) == 80 && sizeof(pantax_hip_profile_ext5) == 88,
                      "appended behind them");
        CHECK(N_EXT5_REPORTS == 1 && EXT5_REPORTS[X5REP_EM].field == &pantax_hip_profile_ext5::strain_em_file && EXT5_REPORTS[X5REP_EM].rows);
        CHECK(std::string(EXT5_REPORTS[X5REP_EM].name) == "strain_em_file" && std::string(EXT5_REPORTS[X5REP_EM].what) == "read class report");
        CHECK(N_EXT4_REPORTS == 1 && N_EXT3_REPORTS == 1 && N_EXT2_REPORTS == 1 && N_EXT_REPORTS == 1);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        std::string err;
        pantax_hip_profile_ext5 e5{};
        pantax_hip_profile_ext *e1 = &e5.v4.v3.v2.v1;
        e1->struct_size = sizeof(e5);
        e5.strain_em_file = "em.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(e1, 1, false, rp, err));
        CHECK(rp.ext5_want[X5REP_EM] && !rp.ext5_run[X5REP_EM] && rp.ext5_path[X5REP_EM] == "em.tsv" && rp.em_classes == 10 && rp.em_iterations == 1000 && !rp.ext4_want[X4REP_ADDIN]);
        resume_reports(rp, true, true, false);
        CHECK(rp.ext5_run[X5REP_EM] && rp.any_run() && rp.rows_run() && !rp.ext4_run[X4REP_ADDIN]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext5_run[X5REP_EM] && !rp.any_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext5_run[X5REP_EM]);
        e5.strain_em_classes = 1; e5.strain_em_iterations = 7;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.em_classes == 1 && rp.em_iterations == 7);
        e5.strain_em_classes = ~0ull; e5.strain_em_iterations = 1ull << 40;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.em_classes == ~0ull && rp.em_iterations == 0xFFFFFFFFu);
        e1->struct_size = 72;                                          // a struct that holds the file alone: 10 and 1000
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext5_want[X5REP_EM] && rp.em_classes == 10 && rp.em_iterations == 1000);
        e1->struct_size = 80; e5.strain_em_classes = 3;                // ... the file and the classes
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext5_want[X5REP_EM] && rp.em_classes == 3 && rp.em_iterations == 1000);
        e1->struct_size = sizeof(e5); e5.strain_em_classes = 0; e5.strain_em_iterations = 0;
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err == "profile: the read class report (strain_em_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(e1, 1, true, rp, err) && err == "profile: the read class report (strain_em_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e5.v4.strain_addin_file = "addin.tsv";                          // the add-one report's refusal comes first
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err.find("strain_addin_file") != std::string::npos);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext4_want[X4REP_ADDIN] && rp.ext5_want[X5REP_EM]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes, the add-one report on where it is held
        for (const uint64_t size : {16ull, 40ull, 48ull, 56ull, 64ull}) {
            e1->struct_size = size;
            CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext5_want[X5REP_EM] && rp.ext5_path[X5REP_EM].empty() && rp.em_classes == 10 && rp.em_iterations == 1000);
            CHECK(rp.ext4_want[X4REP_ADDIN] == (size >= 56));
        }
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e1->struct_size = sizeof(e5); e5.strain_em_file = off; e5.v4.strain_addin_file = nullptr;
            CHECK(plan_ext_reports(e1, 2, true, rp, err) && !rp.ext5_want[X5REP_EM]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext5_want[X5REP_EM]);
    }
    std::printf("read_em_check: ok\n");
    return 0;
}
