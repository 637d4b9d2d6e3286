// links_check.cpp -- the host side of pantax_hip_strain_links at its edges: the classes of one walk's crossings (pantax_hip_link_crossings) on cases done by
// hand, the order in which a strain's breaks are printed (pantax_hip_link_top), and the report's row in the plan of the file seam.  A program of its
// own: tests/test_links_plan.py compiles it with links_plan.cpp and report_plan.cpp by the host C++ compiler under -fsanitize=address,undefined and runs
// it; it returns non-zero at the first check that fails.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "links_plan.hpp"
#include "report_plan.hpp"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "links_check:%d: %s\n", __LINE__, #cond);          \
            return 1;                                                               \
        }                                                                           \
    } while (0)

using namespace ptx;

namespace {

struct Cross { uint64_t q[4]; int rc; };
Cross cross(const std::vector<uint64_t> &masks, const std::vector<uint8_t> &known, uint32_t K) {
    Cross c{{77ull, 77ull, 77ull, 77ull}, 0};
    c.rc = pantax_hip_link_crossings(masks.size(), masks.data(), known.data(), K, c.q);
    return c;
}
bool is(const Cross &c, uint64_t known, uint64_t skip, uint64_t sw, uint64_t foreign) {
    return c.rc == 0 && c.q[0] == known && c.q[1] == skip && c.q[2] == sw && c.q[3] == foreign;
}
bool untouched(const Cross &c) { return c.rc == PANTAX_HIP_E_INVALID && c.q[0] == 77 && c.q[1] == 77 && c.q[2] == 77 && c.q[3] == 77; }

std::vector<uint64_t> top(const std::vector<uint64_t> &flank, const std::vector<uint64_t> &start, uint64_t n_top) {
    std::vector<uint64_t> idx(flank.size() + 1, 99), out;
    uint64_t n = 99;
    if (pantax_hip_link_top(flank.size(), flank.data(), start.data(), n_top, idx.data(), &n) != 0) return {12345};
    out.assign(idx.begin(), idx.begin() + n);
    if (idx[n] != 99) out.push_back(54321);   // nothing behind the kept ones is written
    return out;
}

}  // namespace

int main() {
    // ---- the four classes of a crossing
    CHECK(is(cross({1, 1}, {1}, 1), 1, 0, 0, 0));                       // a link of a member
    CHECK(is(cross({3, 1}, {0}, 2), 0, 1, 0, 0));                       // member 0 walks both nodes, never one after the other: skip
    CHECK(is(cross({1, 2}, {0}, 2), 0, 0, 1, 0));                       // disjoint and both non-empty: switch
    CHECK(is(cross({1, 0}, {0}, 2), 0, 0, 0, 1) && is(cross({0, 2}, {0}, 2), 0, 0, 0, 1) && is(cross({0, 0}, {0}, 2), 0, 0, 0, 1));   // an M is empty: foreign
    CHECK(is(cross({0, 0}, {1}, 2), 1, 0, 0, 0));                       // known goes first, whatever the masks
    CHECK(is(cross({1, 1, 2, 0, 3, 3}, {1, 0, 0, 0, 0}, 2), 1, 1, 1, 2));   // known, switch, foreign, foreign, skip
    CHECK(is(cross({5}, {}, 3), 0, 0, 0, 0));                           // a single step makes no crossing
    uint64_t one_mask = 1, out4[4] = {77, 77, 77, 77};
    CHECK(pantax_hip_link_crossings(1, &one_mask, nullptr, 1, out4) == 0 && out4[0] == 0 && out4[3] == 0);   // known may be null when n = 1
    // K = 0: every crossing is foreign, whatever bits the masks carry
    CHECK(is(cross({~0ull, ~0ull, ~0ull}, {0, 0}, 0), 0, 0, 0, 2));
    // K = 64 with bit 63 in use
    CHECK(is(cross({1ull << 63, 1ull << 63}, {0}, 64), 0, 1, 0, 0));
    CHECK(is(cross({1ull << 63, 1ull}, {0}, 64), 0, 0, 1, 0));
    // bits at and above K are ignored: bit 63 with K = 63 is nobody; bit 2 with K = 2 joins nothing
    CHECK(is(cross({1ull << 63, 1ull << 63}, {0}, 63), 0, 0, 0, 1));
    CHECK(is(cross({1 | 4, 2 | 4}, {0}, 2), 0, 0, 1, 0) && is(cross({1 | 4, 2 | 4}, {0}, 3), 0, 1, 0, 0));
    // the refusals: a null argument, n = 0, K > 64; nothing written
    CHECK(untouched(cross({}, {}, 1)));
    CHECK(untouched(cross({1, 1}, {0}, 65)));
    {
        const uint64_t m[2] = {1, 1};
        const uint8_t k[1] = {0};
        uint64_t o[4] = {77, 77, 77, 77};
        CHECK(pantax_hip_link_crossings(2, nullptr, k, 1, o) == PANTAX_HIP_E_INVALID && pantax_hip_link_crossings(2, m, nullptr, 1, o) == PANTAX_HIP_E_INVALID &&
              pantax_hip_link_crossings(2, m, k, 1, nullptr) == PANTAX_HIP_E_INVALID && o[0] == 77 && o[3] == 77);
    }
    CHECK(link_unknown_class(1, 1) == LNK_SKIP && link_unknown_class(1, 2) == LNK_SWITCH && link_unknown_class(0, 2) == LNK_FOREIGN);
    CHECK(LINKS_MAX_LIST == 64 && LNK_N_SPECIES == PANTAX_HIP_LINK_SPECIES_N && LNK_N_HAP == PANTAX_HIP_LINK_HAP_N && LNK_N_TABLE == 4 && LNK_SUPPORT == 7 &&
          LNK_FOREIGN == 5 && LNK_PRIVATE_BROKEN == 6);
    // ---- the order of the printed breaks: flank descending, then start ascending, then index
    CHECK(top({5, 9, 5, 9, 1}, {40, 30, 10, 20, 0}, 0) == (std::vector<uint64_t>{3, 1, 2, 0, 4}));
    CHECK(top({5, 9, 5, 9, 1}, {40, 30, 10, 20, 0}, 2) == (std::vector<uint64_t>{3, 1}));
    CHECK(top({5, 9, 5, 9, 1}, {40, 30, 10, 20, 0}, 9) == (std::vector<uint64_t>{3, 1, 2, 0, 4}));
    CHECK(top({7, 7, 7}, {3, 3, 1}, 0) == (std::vector<uint64_t>{2, 0, 1}));   // a full tie keeps the index order
    CHECK(top({0, ~0ull}, {0, ~0ull}, 1) == (std::vector<uint64_t>{1}));
    CHECK(top({}, {}, 0).empty());
    {
        uint64_t idx[1] = {99}, n = 99;
        const uint64_t f[1] = {1}, s[1] = {1};
        CHECK(pantax_hip_link_top(0, nullptr, nullptr, 0, idx, &n) == 0 && n == 0 && idx[0] == 99);   // n = 0: the arrays may be null
        n = 99;
        CHECK(pantax_hip_link_top(1, nullptr, s, 0, idx, &n) == PANTAX_HIP_E_INVALID && pantax_hip_link_top(1, f, nullptr, 0, idx, &n) == PANTAX_HIP_E_INVALID &&
              pantax_hip_link_top(1, f, s, 0, nullptr, &n) == PANTAX_HIP_E_INVALID && pantax_hip_link_top(1, f, s, 0, idx, nullptr) == PANTAX_HIP_E_INVALID &&
              n == 99 && idx[0] == 99);
    }
    // ---- the report's row in the plan of the file seam: pantax_hip_profile_ext9 behind the 152-byte eighth version
    {
        static_assert(offsetof(pantax_hip_profile_ext9, v8) == 0 && sizeof(pantax_hip_profile_ext8) == 152 && sizeof(pantax_hip_profile_ext7) == 136 &&
                          sizeof(pantax_hip_profile_ext6) == 120 && sizeof(pantax_hip_profile_ext5) == 88 && sizeof(pantax_hip_profile_ext4) == 64 &&
                          sizeof(pantax_hip_profile_ext3) == 48 && sizeof(pantax_hip_profile_ext2) == 40 && sizeof(pantax_hip_profile_ext) == 16,
                      "the earlier versions keep their size");
        static_assert(offsetof(pantax_hip_profile_ext9, strain_links_file) == 152 && offsetof(pantax_hip_profile_ext9, strain_links_top) == 160 &&
                          sizeof(pantax_hip_profile_ext9) == 168,
                      "the layout of the ninth version");
        CHECK(N_EXT9_REPORTS == 1 && EXT9_REPORTS[X9REP_LINKS].field == &pantax_hip_profile_ext9::strain_links_file && EXT9_REPORTS[X9REP_LINKS].rows);   // it follows the rows of strain_abundance.txt
        CHECK(std::string(EXT9_REPORTS[X9REP_LINKS].name) == "strain_links_file" && std::string(EXT9_REPORTS[X9REP_LINKS].what) == "link support report");
        CHECK(N_EXT8_REPORTS == 1 && N_EXT7_REPORTS == 1 && N_EXT6_REPORTS == 1 && N_EXT5_REPORTS == 1 && N_EXT4_REPORTS == 1 && N_EXT3_REPORTS == 1 && N_EXT2_REPORTS == 1 &&
              N_EXT_REPORTS == 1);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        std::string err;
        pantax_hip_profile_ext9 e9{};
        pantax_hip_profile_ext *e1 = &e9.v8.v7.v6.v5.v4.v3.v2.v1;
        e1->struct_size = sizeof(e9);
        e9.strain_links_file = "lk.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(e1, 1, false, rp, err));
        CHECK(rp.ext9_want[X9REP_LINKS] && !rp.ext9_run[X9REP_LINKS] && rp.ext9_path[X9REP_LINKS] == "lk.tsv" && !rp.ext8_want[X8REP_RESCUE] && rp.lk_top == 10);
        resume_reports(rp, true, true, false);
        CHECK(rp.ext9_run[X9REP_LINKS] && rp.any_run() && rp.rows_run() && !rp.ext8_run[X8REP_RESCUE]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext9_run[X9REP_LINKS] && !rp.any_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext9_run[X9REP_LINKS]);
        resume_reports(rp, true, false, true);                         // the strain-only resume writes it
        CHECK(rp.ext9_run[X9REP_LINKS]);
        e9.strain_links_top = 3;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.lk_top == 3);
        e9.strain_links_top = 0;                                       // 0 reads as 10
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.lk_top == 10);
        e9.strain_links_top = 7;
        e1->struct_size = 160;                                         // a struct that holds the file alone: the default
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext9_want[X9REP_LINKS] && rp.lk_top == 10);
        e1->struct_size = sizeof(e9);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.lk_top == 7);
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err == "profile: the link support report (strain_links_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(e1, 1, true, rp, err) && err == "profile: the link support report (strain_links_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e9.v8.strain_rescue_file = "rc.tsv";                           // the read rescue report's refusal comes first
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err.find("strain_rescue_file") != std::string::npos);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext8_want[X8REP_RESCUE] && rp.ext9_want[X9REP_LINKS]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes, the read rescue report on where it is held
        for (const uint64_t size : {16ull, 40ull, 48ull, 64ull, 88ull, 120ull, 136ull, 144ull, 152ull}) {
            e1->struct_size = size;
            CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext9_want[X9REP_LINKS] && rp.ext9_path[X9REP_LINKS].empty() && rp.lk_top == 10);
            CHECK(rp.ext8_want[X8REP_RESCUE] == (size >= 144));
        }
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e1->struct_size = sizeof(e9); e9.strain_links_file = off; e9.v8.strain_rescue_file = nullptr;
            CHECK(plan_ext_reports(e1, 2, true, rp, err) && !rp.ext9_want[X9REP_LINKS]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext9_want[X9REP_LINKS]);
    }
    std::printf("links_check: ok\n");
    return 0;
}
