// rescue_check.cpp -- the host side of pantax_hip_strain_read_rescue at its edges: the classes of one walk (pantax_hip_rescue_walk) on cases done by
// hand, the order in which a species' candidates are printed (pantax_hip_rescue_rank), the candidate list of the file seam
// (pantax_amd/csrc/rescue_plan.hpp), and the report's row in the plan of the file seam.  A program of its own: tests/test_rescue_plan.py compiles it
// with rescue_plan.cpp and report_plan.cpp by the host C++ compiler under -fsanitize=address,undefined and runs it; it returns non-zero at the first
// check that fails.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "report_plan.hpp"
#include "rescue_plan.hpp"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "rescue_check:%d: %s\n", __LINE__, #cond);         \
            return 1;                                                               \
        }                                                                           \
    } while (0)

using namespace ptx;

namespace {

struct Walk { uint32_t cls; uint64_t d; uint64_t steps[3]; int rc; };
Walk walk(const std::vector<uint64_t> &sel, const std::vector<uint64_t> &cand, uint32_t K, uint32_t J) {
    Walk w{77u, 77ull, {77ull, 77ull, 77ull}, 0};
    w.rc = pantax_hip_rescue_walk(sel.size(), sel.data(), cand.data(), K, J, &w.cls, &w.d, w.steps);
    return w;
}
bool is(const Walk &w, uint32_t cls, uint64_t d, uint64_t f, uint64_t c, uint64_t n) {
    return w.rc == 0 && w.cls == cls && w.d == d && w.steps[0] == f && w.steps[1] == c && w.steps[2] == n;
}

}  // namespace

int main() {
    // ---- the six outcomes of one walk
    {
        CHECK(is(walk({1, 3}, {0, 0}, 2, 2), PANTAX_HIP_RESCUE_COMPATIBLE, 0, 0, 0, 0));
        CHECK(is(walk({2, 0}, {1, 3}, 2, 2), PANTAX_HIP_RESCUE_FOREIGN_RESCUED, 1, 1, 1, 0));
        CHECK(is(walk({0, 0}, {3, 4}, 2, 3), PANTAX_HIP_RESCUE_FOREIGN_PATCHWORK, 0, 2, 2, 0));
        CHECK(is(walk({1, 0}, {1, 0}, 2, 2), PANTAX_HIP_RESCUE_FOREIGN_NOVEL, 0, 1, 0, 1));
        CHECK(is(walk({1, 2}, {1, 1}, 2, 2), PANTAX_HIP_RESCUE_MOSAIC_RESCUED, 1, 0, 0, 0));
        CHECK(is(walk({1, 2}, {0, 1}, 2, 2), PANTAX_HIP_RESCUE_MOSAIC_UNRESCUED, 0, 0, 0, 0));
        CHECK(is(walk({1}, {2}, 1, 2), PANTAX_HIP_RESCUE_COMPATIBLE, 2, 0, 0, 0));                // D(r) is reported for a compatible walk too
        CHECK(is(walk({0, 0, 0}, {3, 3, 7}, 1, 3), PANTAX_HIP_RESCUE_FOREIGN_RESCUED, 3, 3, 3, 0));   // two candidates: contested
        CHECK(is(walk({0, 1, 0}, {1, 1, 1}, 1, 1), PANTAX_HIP_RESCUE_FOREIGN_RESCUED, 1, 2, 2, 0));   // a node visited twice: two steps
        // K = 0: every walk is foreign; J = 0: no rescue
        CHECK(is(walk({7, 7}, {1, 1}, 0, 1), PANTAX_HIP_RESCUE_FOREIGN_RESCUED, 1, 2, 2, 0));
        CHECK(is(walk({7, 7}, {1, 0}, 0, 1), PANTAX_HIP_RESCUE_FOREIGN_NOVEL, 0, 2, 1, 1));
        CHECK(is(walk({1, 0}, {7, 7}, 1, 0), PANTAX_HIP_RESCUE_FOREIGN_NOVEL, 0, 1, 0, 1));
        CHECK(is(walk({1, 1}, {7, 7}, 1, 0), PANTAX_HIP_RESCUE_COMPATIBLE, 0, 0, 0, 0));
        CHECK(is(walk({0}, {0}, 0, 0), PANTAX_HIP_RESCUE_FOREIGN_NOVEL, 0, 1, 0, 1));
        // bits at and above K or J are ignored
        CHECK(is(walk({4, 4}, {8, 9}, 2, 3), PANTAX_HIP_RESCUE_FOREIGN_NOVEL, 0, 2, 1, 1));
        // bit 63: K = 64 with J = 0, and J = 64 with K = 0
        const uint64_t top = 1ull << 63;
        CHECK(is(walk({top, top | 1}, {0, 0}, 64, 0), PANTAX_HIP_RESCUE_COMPATIBLE, 0, 0, 0, 0));
        CHECK(is(walk({top, 1}, {0, 0}, 64, 0), PANTAX_HIP_RESCUE_MOSAIC_UNRESCUED, 0, 0, 0, 0));
        CHECK(is(walk({0, 0}, {top | 2, top}, 0, 64), PANTAX_HIP_RESCUE_FOREIGN_RESCUED, top, 2, 2, 0));
        CHECK(is(walk({1, 0}, {1ull << 62, 1ull << 62}, 1, 63), PANTAX_HIP_RESCUE_FOREIGN_RESCUED, 1ull << 62, 1, 1, 0));
    }
    // ---- the refusals
    {
        const uint64_t m[2] = {1, 1};
        uint32_t cls = 77;
        uint64_t d = 77, st[3] = {77, 77, 77};
        CHECK(pantax_hip_rescue_walk(2, nullptr, m, 1, 1, &cls, &d, st) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_walk(2, m, nullptr, 1, 1, &cls, &d, st) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_walk(2, m, m, 1, 1, nullptr, &d, st) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_walk(2, m, m, 1, 1, &cls, nullptr, st) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_walk(2, m, m, 1, 1, &cls, &d, nullptr) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_walk(0, m, m, 1, 1, &cls, &d, st) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_walk(2, m, m, 33, 32, &cls, &d, st) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_walk(2, m, m, 65, 0, &cls, &d, st) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_walk(2, m, m, 0xFFFFFFFFu, 1, &cls, &d, st) == PANTAX_HIP_E_INVALID);
        CHECK(cls == 77 && d == 77 && st[0] == 77 && st[2] == 77);                                // nothing written
        CHECK(pantax_hip_rescue_walk(2, m, m, 32, 32, &cls, &d, st) == 0);
    }
    // ---- the rank: rescued.span descending, then rescued.n_reads descending, then haplotype index ascending
    {
        const uint32_t hap[6] = {9, 4, 7, 2, 5, 1};
        uint64_t out[6 * 9] = {};
        const auto set = [&](int c, uint64_t n, uint64_t steps, uint64_t span) { out[9 * c] = n; out[9 * c + 1] = steps; out[9 * c + 2] = span; };
        set(0, 3, 90, 100);   // hap 9
        set(1, 5, 10, 100);   // hap 4: the same span, more reads
        set(2, 5, 99, 100);   // hap 7: the same span and reads as hap 4: the haplotype index decides (steps do not)
        set(3, 1, 1, 500);    // hap 2: the widest span
        set(4, 0, 0, 0);      // hap 5: rescues nothing
        set(5, 2, 2, 0);      // hap 1: reads of span 0 still rank
        out[9 * 4 + 3] = 8;   // (alone of a candidate without rescued reads: not looked at)
        uint32_t rank[6] = {77, 77, 77, 77, 77, 77}, n = 77;
        CHECK(pantax_hip_rescue_rank(6, hap, out, 0, rank, &n) == 0 && n == 5);
        CHECK(rank[0] == 3 && rank[1] == 1 && rank[2] == 2 && rank[3] == 0 && rank[4] == 5 && rank[5] == 77);
        CHECK(pantax_hip_rescue_rank(6, hap, out, 2, rank, &n) == 0 && n == 2 && rank[0] == 3 && rank[1] == 1);
        CHECK(pantax_hip_rescue_rank(6, hap, out, 9, rank, &n) == 0 && n == 5);
        CHECK(pantax_hip_rescue_rank(0, hap, out, 0, rank, &n) == 0 && n == 0);
        n = 77;
        CHECK(pantax_hip_rescue_rank(6, nullptr, out, 0, rank, &n) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_rank(6, hap, nullptr, 0, rank, &n) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_rank(6, hap, out, 0, nullptr, &n) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_rank(6, hap, out, 0, rank, nullptr) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_rescue_rank(0, nullptr, out, 0, rank, &n) == PANTAX_HIP_E_INVALID && n == 77);
    }
    // ---- the seam's candidates: the ranked ones first, then the rest in ascending haplotype index, cut to 64 - K
    {
        const uint32_t hap[6] = {9, 4, 7, 2, 5, 1};
        const uint32_t ranked[2] = {2, 0};
        CHECK(rescue_candidates(3, 6, hap, ranked, 2) == (std::vector<uint32_t>{2, 0, 5, 3, 1, 4}));
        CHECK(rescue_candidates(0, 6, hap, ranked, 0) == (std::vector<uint32_t>{5, 3, 1, 4, 2, 0}));
        CHECK(rescue_candidates(60, 6, hap, ranked, 2) == (std::vector<uint32_t>{2, 0, 5, 3}));    // 64 - 60
        CHECK(rescue_candidates(63, 6, hap, ranked, 2) == (std::vector<uint32_t>{2}));
        CHECK(rescue_candidates(64, 6, hap, ranked, 2).empty() && rescue_candidates(70, 6, hap, ranked, 2).empty());
        CHECK(rescue_candidates(3, 0, hap, ranked, 0).empty());
        std::vector<uint32_t> wide(100);
        for (uint32_t i = 0; i < 100; ++i) wide[i] = 99 - i;
        const std::vector<uint32_t> cut = rescue_candidates(10, 100, wide.data(), ranked, 2);
        CHECK(cut.size() == 54 && cut[0] == 2 && cut[1] == 0 && cut[2] == 99 && cut[3] == 98 && cut[53] == 48);   // haplotypes 97, 99, then 0, 1, ..
        CHECK(RESCUE_MAX_LIST == 64 && RES_N_CLASSES == PANTAX_HIP_RESCUE_CLASSES && RES_N_CAND == 3 && RES_CONTESTED == 8 && RES_MOSAIC == 6);
    }
    // ---- the report's row in the plan of the file seam: pantax_hip_profile_ext8 behind the 136-byte seventh version
    {
        static_assert(offsetof(pantax_hip_profile_ext8, v7) == 0 && sizeof(pantax_hip_profile_ext7) == 136 && sizeof(pantax_hip_profile_ext6) == 120 &&
                          sizeof(pantax_hip_profile_ext5) == 88 && sizeof(pantax_hip_profile_ext4) == 64 && sizeof(pantax_hip_profile_ext3) == 48 &&
                          sizeof(pantax_hip_profile_ext2) == 40 && sizeof(pantax_hip_profile_ext) == 16,
                      "the earlier versions keep their size");
        static_assert(offsetof(pantax_hip_profile_ext8, strain_rescue_file) == 136 && offsetof(pantax_hip_profile_ext8, strain_rescue_top) == 144 &&
                          sizeof(pantax_hip_profile_ext8) == 152,
                      "the layout of the eighth version");
        CHECK(N_EXT8_REPORTS == 1 && EXT8_REPORTS[X8REP_RESCUE].field == &pantax_hip_profile_ext8::strain_rescue_file && !EXT8_REPORTS[X8REP_RESCUE].rows);
        CHECK(std::string(EXT8_REPORTS[X8REP_RESCUE].name) == "strain_rescue_file" && std::string(EXT8_REPORTS[X8REP_RESCUE].what) == "read rescue report");
        CHECK(N_EXT7_REPORTS == 1 && N_EXT6_REPORTS == 1 && N_EXT5_REPORTS == 1 && N_EXT4_REPORTS == 1 && N_EXT3_REPORTS == 1 && N_EXT2_REPORTS == 1 && N_EXT_REPORTS == 1);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        std::string err;
        pantax_hip_profile_ext8 e8{};
        pantax_hip_profile_ext *e1 = &e8.v7.v6.v5.v4.v3.v2.v1;
        e1->struct_size = sizeof(e8);
        e8.strain_rescue_file = "rc.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(e1, 1, false, rp, err));
        CHECK(rp.ext8_want[X8REP_RESCUE] && !rp.ext8_run[X8REP_RESCUE] && rp.ext8_path[X8REP_RESCUE] == "rc.tsv" && !rp.ext7_want[X7REP_MOSAIC] && rp.rs_top == 5);
        resume_reports(rp, true, true, false);
        CHECK(rp.ext8_run[X8REP_RESCUE] && rp.any_run() && !rp.rows_run() && !rp.ext7_run[X7REP_MOSAIC]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext8_run[X8REP_RESCUE] && !rp.any_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext8_run[X8REP_RESCUE]);
        resume_reports(rp, true, false, true);                         // the strain-only resume writes it
        CHECK(rp.ext8_run[X8REP_RESCUE]);
        e8.strain_rescue_top = 3;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.rs_top == 3);
        e8.strain_rescue_top = 0;                                      // 0 reads as 5
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.rs_top == 5);
        e8.strain_rescue_top = 7;
        e1->struct_size = 144;                                         // a struct that holds the file alone: the default
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext8_want[X8REP_RESCUE] && rp.rs_top == 5);
        e1->struct_size = sizeof(e8);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.rs_top == 7);
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err == "profile: the read rescue report (strain_rescue_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(e1, 1, true, rp, err) && err == "profile: the read rescue report (strain_rescue_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e8.v7.strain_mosaic_file = "mo.tsv";                           // the mosaic read report's refusal comes first
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err.find("strain_mosaic_file") != std::string::npos);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext7_want[X7REP_MOSAIC] && rp.ext8_want[X8REP_RESCUE]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes, the mosaic read report on where it is held
        for (const uint64_t size : {16ull, 40ull, 48ull, 64ull, 88ull, 120ull, 128ull, 136ull}) {
            e1->struct_size = size;
            CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext8_want[X8REP_RESCUE] && rp.ext8_path[X8REP_RESCUE].empty() && rp.rs_top == 5);
            CHECK(rp.ext7_want[X7REP_MOSAIC] == (size >= 128));
        }
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e1->struct_size = sizeof(e8); e8.strain_rescue_file = off; e8.v7.strain_mosaic_file = nullptr;
            CHECK(plan_ext_reports(e1, 2, true, rp, err) && !rp.ext8_want[X8REP_RESCUE]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext8_want[X8REP_RESCUE]);
    }
    std::printf("rescue_check: ok\n");
    return 0;
}
