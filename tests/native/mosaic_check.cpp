// mosaic_check.cpp -- the host side of pantax_hip_strain_mosaic at its edges: the greedy cut of one walk (pantax_hip_mosaic_walk) on cases done by hand
// and against a brute-force minimum over all cuts, the junction order of the report (pantax_hip_mosaic_top), the sort and run-length of the device's break
// records (pantax_amd/csrc/mosaic_plan.hpp), and the report's row in the plan of the file seam.  A program of its own: tests/test_mosaic_plan.py compiles
// it with mosaic_plan.cpp and report_plan.cpp by the host C++ compiler under -fsanitize=address,undefined and runs it; it returns non-zero at the first
// check that fails.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "mosaic_plan.hpp"
#include "report_plan.hpp"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "mosaic_check:%d: %s\n", __LINE__, #cond);         \
            return 1;                                                               \
        }                                                                           \
    } while (0)

using namespace ptx;

namespace {

// the smallest number of stretches of masks[0 .. n) whose AND is non-zero each, by dynamic programming over the cut before step i
uint64_t brute_min(const std::vector<uint64_t> &m) {
    const size_t n = m.size();
    std::vector<uint64_t> best(n + 1, ~0ull);
    best[0] = 0;
    for (size_t i = 1; i <= n; ++i) {
        uint64_t run = ~0ull;
        for (size_t j = i; j-- > 0;) {   // the last stretch is [j, i)
            run &= m[j];
            if (!run) break;
            if (best[j] != ~0ull) best[i] = std::min(best[i], best[j] + 1);
        }
    }
    return best[n];
}

}  // namespace

int main() {
    uint64_t k = 99, fs = 99;
    // ---- the cut, by hand: positions 0, 1, 2 with haplotypes 5, 3, 4 and weights 1, 2, 2
    {
        const double w[3] = {1.0, 2.0, 2.0};
        const uint32_t hap[3] = {5, 3, 4};
        uint64_t end[8];
        uint32_t pos[8];
        const uint64_t one_break[4] = {0b011, 0b001, 0b110, 0b110};                      // {0,1} {0} | {1,2} {1,2}
        CHECK(pantax_hip_mosaic_walk(4, one_break, 3, w, hap, end, pos, 8, &k, &fs) == 0 && k == 2 && fs == 0);
        CHECK(end[0] == 2 && pos[0] == 0 && end[1] == 4 && pos[1] == 1);                 // equal weights 2, 2: haplotype 3 (position 1) before haplotype 4
        const uint64_t first_step[3] = {0b001, 0b110, 0b100};                            // a break at the first possible step
        CHECK(pantax_hip_mosaic_walk(3, first_step, 3, w, hap, end, pos, 8, &k, &fs) == 0 && k == 2 && end[0] == 1 && pos[0] == 0 && end[1] == 3 && pos[1] == 2);
        const uint64_t late[4] = {0b011, 0b011, 0b110, 0b110};                           // the break goes as late as it can: position 1 fits all four steps
        CHECK(pantax_hip_mosaic_walk(4, late, 3, w, hap, end, pos, 8, &k, &fs) == 0 && k == 1 && end[0] == 4 && pos[0] == 1);
        const uint64_t foreign[5] = {0, 0b001, 0b110, 0, 0b1000};                         // bit 3 is at K: ignored, the step is empty
        end[0] = 77;
        CHECK(pantax_hip_mosaic_walk(5, foreign, 3, w, hap, end, pos, 8, &k, &fs) == 0 && k == 0 && fs == 3 && end[0] == 77);   // not cut
        const uint64_t twice[4] = {0b001, 0b110, 0b110, 0b001};                          // a step's mask on both sides of two breaks
        CHECK(pantax_hip_mosaic_walk(4, twice, 3, w, hap, end, pos, 8, &k, &fs) == 0 && k == 3 && end[0] == 1 && end[1] == 3 && end[2] == 4 && pos[0] == 0 && pos[1] == 1 && pos[2] == 0);
        // cap too small: k and the first cap segments are written, nothing behind them
        end[1] = 77; pos[1] = 77;
        CHECK(pantax_hip_mosaic_walk(4, twice, 3, w, hap, end, pos, 1, &k, &fs) == PANTAX_HIP_E_LIMIT && k == 3 && fs == 0 && end[0] == 1 && end[1] == 77 && pos[1] == 77);
        CHECK(pantax_hip_mosaic_walk(4, twice, 3, w, hap, nullptr, nullptr, 0, &k, &fs) == PANTAX_HIP_E_LIMIT && k == 3);    // sizing call
        // an empty walk
        k = fs = 99;
        CHECK(pantax_hip_mosaic_walk(0, nullptr, 3, w, hap, end, pos, 8, &k, &fs) == 0 && k == 0 && fs == 0);
        // refusals
        const uint32_t dup[3] = {5, 3, 5};
        CHECK(pantax_hip_mosaic_walk(4, twice, 3, w, dup, end, pos, 8, &k, &fs) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_mosaic_walk(4, twice, 0, w, hap, end, pos, 8, &k, &fs) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_mosaic_walk(4, twice, 65, w, hap, end, pos, 8, &k, &fs) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_mosaic_walk(4, nullptr, 3, w, hap, end, pos, 8, &k, &fs) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_mosaic_walk(4, twice, 3, w, hap, end, pos, 8, nullptr, &fs) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_mosaic_walk(4, twice, 3, w, hap, nullptr, pos, 8, &k, &fs) == PANTAX_HIP_E_INVALID);
    }
    // ---- 64 candidates: words with bit 63 set, and a walk of 65 steps with 64 breaks
    {
        std::vector<double> w(64, 1.0);
        std::vector<uint32_t> hap(64);
        for (uint32_t i = 0; i < 64; ++i) hap[i] = 63 - i;                               // position 63 is haplotype 0: it wins every tie
        w[63] = 1.0;
        uint64_t end[80];
        uint32_t pos[80];
        const uint64_t hi[3] = {1ull << 63 | 1ull, 1ull << 63, ~0ull};
        CHECK(pantax_hip_mosaic_walk(3, hi, 64, w.data(), hap.data(), end, pos, 80, &k, &fs) == 0 && k == 1 && end[0] == 3 && pos[0] == 63);
        std::vector<uint64_t> alt(65);
        for (size_t i = 0; i < 65; ++i) alt[i] = i % 2 ? 1ull << 63 : 1ull << (i / 2 % 63);   // neighbours never share a bit
        CHECK(pantax_hip_mosaic_walk(65, alt.data(), 64, w.data(), hap.data(), end, pos, 80, &k, &fs) == 0 && k == 65 && fs == 0);
        for (size_t i = 0; i < 65; ++i) CHECK(end[i] == i + 1 && pos[i] == (i % 2 ? 63u : (uint32_t)(i / 2 % 63)));
        CHECK(pantax_hip_mosaic_walk(65, alt.data(), 64, w.data(), hap.data(), end, pos, 64, &k, &fs) == PANTAX_HIP_E_LIMIT && k == 65);
        w[7] = -1.0;                                                                      // a weight below the others loses; NaN never wins
        const uint64_t two[1] = {1ull << 7 | 1ull << 9};
        CHECK(pantax_hip_mosaic_walk(1, two, 64, w.data(), hap.data(), end, pos, 80, &k, &fs) == 0 && k == 1 && pos[0] == 9);
    }
    // ---- greedy = the minimum over all cuts = the greedy of the reversed walk
    {
        std::mt19937_64 rng(17);
        uint64_t seen = 0;
        for (int round = 0; round < 600; ++round) {
            const uint32_t K = 1 + (uint32_t)(rng() % 6);
            const size_t n = 1 + rng() % 12;
            std::vector<uint64_t> m(n);
            for (uint64_t &x : m) { x = rng() & rng() & ((1ull << K) - 1); if (!x) x = 1ull << (rng() % K); }
            std::vector<double> w(K, 1.0);
            std::vector<uint32_t> hap(K);
            for (uint32_t i = 0; i < K; ++i) hap[i] = i;
            std::vector<uint64_t> end(n);
            std::vector<uint32_t> pos(n);
            uint64_t kr = 0;
            CHECK(pantax_hip_mosaic_walk(n, m.data(), K, w.data(), hap.data(), end.data(), pos.data(), n, &k, &fs) == 0 && fs == 0 && k == brute_min(m));
            uint64_t at = 0;
            for (uint64_t j = 0; j < k; ++j) {                                            // every segment's AND holds its assigned position; the next step does not fit
                uint64_t run = ~0ull;
                for (; at < end[j]; ++at) run &= m[at];
                CHECK(run && ((run >> pos[j]) & 1ull) && (j + 1 == k || (run & m[at]) == 0));
            }
            CHECK(at == n);
            std::reverse(m.begin(), m.end());
            CHECK(pantax_hip_mosaic_walk(n, m.data(), K, w.data(), hap.data(), end.data(), pos.data(), n, &kr, &fs) == 0 && kr == k);
            seen |= 1ull << std::min<uint64_t>(k, 5);
        }
        CHECK((seen & 0b111110) == 0b111110);
    }
    // ---- the junctions a report prints
    {
        const uint32_t a[6] = {4, 1, 1, 9, 2, 2}, b[6] = {5, 7, 3, 9, 8, 1};
        const uint64_t c[6] = {2, 5, 5, 1, 2, 9};
        uint64_t idx[6], m = 99;
        CHECK(pantax_hip_mosaic_top(6, a, b, c, 10, idx, &m) == 0 && m == 6);
        CHECK(idx[0] == 5 && idx[1] == 2 && idx[2] == 1 && idx[3] == 4 && idx[4] == 0 && idx[5] == 3);   // count down; then node_a, node_b up
        CHECK(pantax_hip_mosaic_top(6, a, b, c, 2, idx, &m) == 0 && m == 2 && idx[0] == 5 && idx[1] == 2);
        CHECK(pantax_hip_mosaic_top(6, a, b, c, 0, nullptr, &m) == 0 && m == 0);
        CHECK(pantax_hip_mosaic_top(0, nullptr, nullptr, nullptr, 3, nullptr, &m) == 0 && m == 0);
        CHECK(pantax_hip_mosaic_top(6, a, b, nullptr, 3, idx, &m) == PANTAX_HIP_E_INVALID && pantax_hip_mosaic_top(6, a, b, c, 3, idx, nullptr) == PANTAX_HIP_E_INVALID);
    }
    // ---- break records -> distinct junctions with their counts
    {
        std::vector<MosaicBreak> recs = {{2, 7, 1}, {0, 9, 9}, {2, 7, 1}, {2, 1, 7}, {0, 9, 9}, {2, 7, 1}, {1, 0xFFFFFFFFu, 0}}, d;
        std::vector<uint64_t> n;
        mosaic_junctions(recs, d, n);
        CHECK(d.size() == 4 && n.size() == 4);
        CHECK(d[0] == (MosaicBreak{0, 9, 9}) && n[0] == 2 && d[1] == (MosaicBreak{1, 0xFFFFFFFFu, 0}) && n[1] == 1 && d[2] == (MosaicBreak{2, 1, 7}) && n[2] == 1 &&
              d[3] == (MosaicBreak{2, 7, 1}) && n[3] == 3);
        recs.clear();
        mosaic_junctions(recs, d, n);
        CHECK(d.empty() && n.empty());
        CHECK(mosaic_class_of(1) == MOS_COMPATIBLE && mosaic_class_of(2) == MOS_MOSAIC1 && mosaic_class_of(3) == MOS_MOSAIC2 && mosaic_class_of(4) == MOS_MOSAIC3PLUS &&
              mosaic_class_of(64) == MOS_MOSAIC3PLUS && MOS_N_CLASSES == PANTAX_HIP_MOSAIC_CLASSES);
    }
    // ---- the report's row in the plan of the file seam: pantax_hip_profile_ext7 behind the 120-byte sixth version
    {
        static_assert(offsetof(pantax_hip_profile_ext7, v6) == 0 && sizeof(pantax_hip_profile_ext6) == 120 && sizeof(pantax_hip_profile_ext5) == 88 &&
                          sizeof(pantax_hip_profile_ext4) == 64 && sizeof(pantax_hip_profile_ext3) == 48 && sizeof(pantax_hip_profile_ext2) == 40 &&
                          sizeof(pantax_hip_profile_ext) == 16,
                      "the earlier versions keep their size");
        static_assert(offsetof(pantax_hip_profile_ext7, strain_mosaic_file) == 120 && offsetof(pantax_hip_profile_ext7, strain_mosaic_top) == 128 &&
                          sizeof(pantax_hip_profile_ext7) == 136,
                      "the layout of the seventh version");
        CHECK(N_EXT7_REPORTS == 1 && EXT7_REPORTS[X7REP_MOSAIC].field == &pantax_hip_profile_ext7::strain_mosaic_file && EXT7_REPORTS[X7REP_MOSAIC].rows);
        CHECK(std::string(EXT7_REPORTS[X7REP_MOSAIC].name) == "strain_mosaic_file" && std::string(EXT7_REPORTS[X7REP_MOSAIC].what) == "mosaic read report");
        CHECK(N_EXT6_REPORTS == 1 && N_EXT5_REPORTS == 1 && N_EXT4_REPORTS == 1 && N_EXT3_REPORTS == 1 && N_EXT2_REPORTS == 1 && N_EXT_REPORTS == 1);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        std::string err;
        pantax_hip_profile_ext7 e7{};
        pantax_hip_profile_ext *e1 = &e7.v6.v5.v4.v3.v2.v1;
        e1->struct_size = sizeof(e7);
        e7.strain_mosaic_file = "mo.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(e1, 1, false, rp, err));
        CHECK(rp.ext7_want[X7REP_MOSAIC] && !rp.ext7_run[X7REP_MOSAIC] && rp.ext7_path[X7REP_MOSAIC] == "mo.tsv" && !rp.ext6_want[X6REP_SEGMENTS] && rp.mo_top == 10);
        resume_reports(rp, true, true, false);
        CHECK(rp.ext7_run[X7REP_MOSAIC] && rp.any_run() && rp.rows_run() && !rp.ext6_run[X6REP_SEGMENTS]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext7_run[X7REP_MOSAIC] && !rp.any_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext7_run[X7REP_MOSAIC]);
        resume_reports(rp, true, false, true);                         // the strain-only resume writes it
        CHECK(rp.ext7_run[X7REP_MOSAIC]);
        e7.strain_mosaic_top = 3;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.mo_top == 3);
        e7.strain_mosaic_top = PANTAX_HIP_MOSAIC_TOP_OFF;              // no junction rows
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext7_want[X7REP_MOSAIC] && rp.mo_top == 0);
        e7.strain_mosaic_top = 7;
        e1->struct_size = 128;                                         // a struct that holds the file alone: the default
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext7_want[X7REP_MOSAIC] && rp.mo_top == 10);
        e1->struct_size = sizeof(e7);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.mo_top == 7);
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err == "profile: the mosaic read report (strain_mosaic_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(e1, 1, true, rp, err) && err == "profile: the mosaic read report (strain_mosaic_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e7.v6.strain_segments_file = "seg.tsv";                        // the segment report's refusal comes first
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err.find("strain_segments_file") != std::string::npos);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext6_want[X6REP_SEGMENTS] && rp.ext7_want[X7REP_MOSAIC]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes, the segment report on where it is held
        for (const uint64_t size : {16ull, 40ull, 48ull, 64ull, 88ull, 96ull, 120ull}) {
            e1->struct_size = size;
            CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext7_want[X7REP_MOSAIC] && rp.ext7_path[X7REP_MOSAIC].empty() && rp.mo_top == 10);
            CHECK(rp.ext6_want[X6REP_SEGMENTS] == (size >= 96));
        }
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e1->struct_size = sizeof(e7); e7.strain_mosaic_file = off; e7.v6.strain_segments_file = nullptr;
            CHECK(plan_ext_reports(e1, 2, true, rp, err) && !rp.ext7_want[X7REP_MOSAIC]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext7_want[X7REP_MOSAIC]);
    }
    std::printf("mosaic_check: ok\n");
    return 0;
}
