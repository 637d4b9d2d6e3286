// growth_plan_check.cpp -- the host side of the replication index report at its edges: the fit over own-node windows (pantax_hip_growth_fit) on windows
// done by hand, every status and every refusal, and the report's row in the plan of the file seam (pantax_hip_profile_ext12 behind the 208-byte eleventh
// version).  A program of its own: tests/test_growth_plan.py compiles it with growth_plan.cpp and report_plan.cpp by the host C++ compiler under
// -fsanitize=address,undefined and runs it; it returns non-zero at the first check that fails.  With a file name as its argument it reads one case a line
// ("min_own trim_permille min_windows min_depth n len_own[n] bases_own[n]") and prints the result of each, floats as hexadecimal f64, for the test to hold
// against the Python restatement.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "growth_plan.hpp"
#include "report_plan.hpp"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "growth_plan_check:%d: %s\n", __LINE__, #cond); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

using namespace ptx;

namespace {

pantax_hip_growth_fit_result fit_of(const std::vector<uint64_t> &len, const std::vector<uint64_t> &bases, uint64_t min_own, uint64_t trim, uint64_t min_windows,
                                    double min_depth, int *rc) {
    pantax_hip_growth_fit_result r;
    std::memset(&r, 0x5A, sizeof(r));
    const std::vector<uint64_t> l(len), b(bases);   // exact copies: the sanitizer sees a read past their ends
    *rc = pantax_hip_growth_fit(l.size(), l.empty() ? nullptr : l.data(), b.empty() ? nullptr : b.data(), min_own, trim, min_windows, min_depth, &r);
    return r;
}
bool near(double a, double b) { return a == b || (a - b < 1e-12 * (b < 0 ? -b : b) && b - a < 1e-12 * (b < 0 ? -b : b)); }

}  // namespace

int main(int argc, char **argv) {
    int rc = 0;
    // ---- by hand: depths 4, 1, 2, a window without bases, and a window of 4 own bases that min_own = 5 drops: y = 0, 1, 2 at x = 1/6, 3/6, 5/6
    const std::vector<uint64_t> L{10, 10, 10, 10, 4}, B{40, 10, 20, 0, 400};
    {
        const auto r = fit_of(L, B, 5, 0, 2, 1.0, &rc);
        CHECK(rc == 0 && r.n_kept == 4 && r.n_zero == 1 && r.n_f == 3 && r.n_fit == 3 && r.own_len == 40 && r.status == PANTAX_HIP_GROWTH_OK && r.pad == 0);
        CHECK(r.median_depth == 2.0 && near(r.slope, 3.0) && near(r.intercept, -0.5) && near(r.r2, 1.0) && near(r.index, 8.0));
    }
    // ---- every status, the first that applies
    CHECK(fit_of(L, B, 5, 0, 4, 1.0, &rc).status == PANTAX_HIP_GROWTH_FEW_WINDOWS && rc == 0);
    CHECK(fit_of(L, B, 5, 0, 4, 3.0, &rc).status == PANTAX_HIP_GROWTH_FEW_WINDOWS && rc == 0);       // few windows AND low depth
    CHECK(fit_of(L, B, 5, 0, 3, 3.0, &rc).status == PANTAX_HIP_GROWTH_LOW_DEPTH && rc == 0);
    {
        const auto r = fit_of({1, 2, 3}, {2, 4, 6}, 1, 0, 1, 0.0, &rc);                                 // 2/1 = 4/2 = 6/3
        CHECK(rc == 0 && r.status == PANTAX_HIP_GROWTH_FLAT && r.slope == 0.0 && r.r2 == 0.0 && r.index == 1.0 && r.intercept == 1.0 && r.median_depth == 2.0 && r.n_fit == 3);
        CHECK(fit_of({1, 2, 3}, {2, 4, 6}, 1, 0, 1, 2.5, &rc).status == PANTAX_HIP_GROWTH_LOW_DEPTH);   // low depth before flat
    }
    for (const auto &none : {std::vector<uint64_t>{}, std::vector<uint64_t>{0, 0}}) {                   // no window; windows without bases
        const auto r = fit_of(std::vector<uint64_t>(none.size(), 5), none, 1, 100, 0, 0.0, &rc);
        CHECK(rc == 0 && r.status == PANTAX_HIP_GROWTH_EMPTY && r.n_fit == 0 && r.n_f == 0 && r.n_zero == none.size() && r.n_kept == none.size() && r.own_len == 5 * none.size());
        CHECK(r.median_depth == 0.0 && r.slope == 0.0 && r.intercept == 0.0 && r.r2 == 0.0 && r.index == 1.0);
    }
    CHECK(fit_of({3, 3}, {9, 9}, 4, 0, 0, 0.0, &rc).status == PANTAX_HIP_GROWTH_EMPTY && rc == 0);        // nothing kept
    CHECK(std::string(pantax_hip_growth_status_name(PANTAX_HIP_GROWTH_OK)) == "ok" && std::string(pantax_hip_growth_status_name(PANTAX_HIP_GROWTH_EMPTY)) == "empty" &&
          std::string(pantax_hip_growth_status_name(PANTAX_HIP_GROWTH_FEW_WINDOWS)) == "few_windows" &&
          std::string(pantax_hip_growth_status_name(PANTAX_HIP_GROWTH_LOW_DEPTH)) == "low_depth" && std::string(pantax_hip_growth_status_name(PANTAX_HIP_GROWTH_FLAT)) == "flat" &&
          std::string(pantax_hip_growth_status_name(5)) == "?" && std::string(pantax_hip_growth_status_name(-1)) == "?");
    CHECK(PANTAX_HIP_GROWTH_MIN_WINDOWS == 20 && PANTAX_HIP_GROWTH_MIN_DEPTH == 5.0);
    // ---- the median, the factor of 8 and the trim; the exact order where f64 cannot tell
    {
        auto r = fit_of({1, 1, 1, 1}, {1, 2, 16, 1000}, 1, 0, 1, 0.0, &rc);
        CHECK(rc == 0 && r.median_depth == 2.0 && r.n_f == 3 && r.n_fit == 3);
        std::vector<uint64_t> p2;
        for (int k = 0; k < 10; ++k) p2.push_back(1ull << k);
        r = fit_of(std::vector<uint64_t>(10, 1), p2, 1, 150, 1, 0.0, &rc);
        CHECK(rc == 0 && r.n_kept == 10 && r.n_f == 7 && r.n_fit == 5 && r.median_depth == 16.0 && near(r.slope, 7.0) && near(r.index, 128.0) && near(r.intercept, 0.5));
        r = fit_of({1ull << 60, 1, 1}, {(1ull << 60) + 1, 1, 2}, 1, 0, 1, 0.0, &rc);
        CHECK(rc == 0 && r.n_fit == 3 && r.median_depth == 1.0);
        r = fit_of({~0ull, ~0ull, ~0ull - 1}, {~0ull - 1, ~0ull, ~0ull}, 1, 0, 1, 0.0, &rc);             // products near 2^128
        CHECK(rc == 0 && r.n_fit == 3 && r.n_kept == 3);
    }
    // ---- the refusals: nothing is written
    {
        pantax_hip_growth_fit_result r;
        std::memset(&r, 0x5A, sizeof(r));
        const pantax_hip_growth_fit_result before = r;
        const uint64_t l[2] = {5, 5}, b[2] = {1, 2};
        CHECK(pantax_hip_growth_fit(2, nullptr, b, 1, 0, 1, 0.0, &r) == PANTAX_HIP_E_INVALID && pantax_hip_growth_fit(2, l, nullptr, 1, 0, 1, 0.0, &r) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_growth_fit(2, l, b, 1, 0, 1, 0.0, nullptr) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_growth_fit(2, l, b, 0, 0, 1, 0.0, &r) == PANTAX_HIP_E_INVALID);                 // min_own 0
        CHECK(pantax_hip_growth_fit(2, l, b, 1, 500, 1, 0.0, &r) == PANTAX_HIP_E_INVALID && pantax_hip_growth_fit(2, l, b, 1, ~0ull, 1, 0.0, &r) == PANTAX_HIP_E_INVALID);
        CHECK(std::memcmp(&r, &before, sizeof(r)) == 0);
        CHECK(pantax_hip_growth_fit(2, l, b, 1, 499, 1, 0.0, &r) == 0 && r.n_fit == 2);                  // the largest trim leaves a window
        CHECK(pantax_hip_growth_fit(0, nullptr, nullptr, 1, 0, 1, 0.0, &r) == 0 && r.status == PANTAX_HIP_GROWTH_EMPTY);
    }
    // ---- the report's row in the plan of the file seam: pantax_hip_profile_ext12 behind the 208-byte eleventh version
    {
        static_assert(offsetof(pantax_hip_profile_ext12, v11) == 0 && sizeof(pantax_hip_profile_ext11) == 208 && sizeof(pantax_hip_profile_ext10) == 200 &&
                          sizeof(pantax_hip_profile_ext9) == 168 && sizeof(pantax_hip_profile_ext8) == 152 && sizeof(pantax_hip_profile_ext7) == 136 &&
                          sizeof(pantax_hip_profile_ext6) == 120 && sizeof(pantax_hip_profile_ext5) == 88 && sizeof(pantax_hip_profile_ext4) == 64 &&
                          sizeof(pantax_hip_profile_ext3) == 48 && sizeof(pantax_hip_profile_ext2) == 40 && sizeof(pantax_hip_profile_ext) == 16,
                      "the closed versions of the extension keep their sizes");
        static_assert(offsetof(pantax_hip_profile_ext12, strain_growth_file) == 208 && offsetof(pantax_hip_profile_ext12, strain_growth_window) == 216 &&
                          offsetof(pantax_hip_profile_ext12, strain_growth_min_own_permille) == 224 && offsetof(pantax_hip_profile_ext12, strain_growth_trim_permille) == 232 &&
                          sizeof(pantax_hip_profile_ext12) == 240,
                      "the twelfth version");
        static_assert(sizeof(pantax_hip_growth_fit_result) == 88 && offsetof(pantax_hip_growth_fit_result, median_depth) == 40 && offsetof(pantax_hip_growth_fit_result, status) == 80,
                      "the fit's result");
        CHECK(N_EXT12_REPORTS == 1 && EXT12_REPORTS[X12REP_GROWTH].field == &pantax_hip_profile_ext12::strain_growth_file && EXT12_REPORTS[X12REP_GROWTH].rows);
        CHECK(std::string(EXT12_REPORTS[X12REP_GROWTH].name) == "strain_growth_file" && std::string(EXT12_REPORTS[X12REP_GROWTH].what) == "replication index report");
        CHECK(N_EXT11_REPORTS == 1 && N_EXT10_REPORTS == 1);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        std::string err;
        pantax_hip_profile_ext12 e12{};
        pantax_hip_profile_ext *e1 = &e12.v11.v10.v9.v8.v7.v6.v5.v4.v3.v2.v1;
        e1->struct_size = sizeof(e12);
        e12.strain_growth_file = "gr.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(e1, 1, false, rp, err));
        CHECK(rp.ext12_want[X12REP_GROWTH] && !rp.ext12_run[X12REP_GROWTH] && rp.ext12_path[X12REP_GROWTH] == "gr.tsv" && !rp.ext11_want[X11REP_FRAGMENTS]);
        CHECK(rp.gr_window == 5000 && rp.gr_min_own == 500 && rp.gr_trim == 100);                      // a zero is the default
        resume_reports(rp, true, true, false);
        CHECK(rp.ext12_run[X12REP_GROWTH] && rp.any_run() && rp.rows_run() && !rp.ext11_run[X11REP_FRAGMENTS]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext12_run[X12REP_GROWTH] && !rp.any_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext12_run[X12REP_GROWTH]);
        resume_reports(rp, true, false, true);                         // the strain-only resume writes it
        CHECK(rp.ext12_run[X12REP_GROWTH]);
        e12.strain_growth_window = 777; e12.strain_growth_min_own_permille = 1000; e12.strain_growth_trim_permille = 499;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.gr_window == 777 && rp.gr_min_own == 1000 && rp.gr_trim == 499);
        e12.strain_growth_min_own_permille = 1001;
        CHECK(!plan_ext_reports(e1, 1, false, rp, err) && err == "profile: strain_growth_min_own_permille 1001 (at most 1000)");
        e12.strain_growth_min_own_permille = 0; e12.strain_growth_trim_permille = 500;
        CHECK(!plan_ext_reports(e1, 1, false, rp, err) && err == "profile: strain_growth_trim_permille 500 (below 500)");
        e12.strain_growth_file = nullptr;                               // ... and of a report that is off nothing is read
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext12_want[X12REP_GROWTH] && rp.gr_trim == 100);
        e12.strain_growth_file = "gr.tsv"; e12.strain_growth_trim_permille = 0; e12.strain_growth_window = 0;
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err == "profile: the replication index report (strain_growth_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(e1, 1, true, rp, err) &&
              err == "profile: the replication index report (strain_growth_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e12.v11.strain_fragments_file = "fr.tsv";                       // the fragment report's refusal comes first
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err.find("strain_fragments_file") != std::string::npos);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext11_want[X11REP_FRAGMENTS] && rp.ext12_want[X12REP_GROWTH]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes, the fragment report on where it is held; a struct that ends
        // inside the twelfth version holds the fields it holds
        for (const uint64_t size : {16ull, 40ull, 48ull, 64ull, 88ull, 120ull, 136ull, 152ull, 168ull, 200ull, 208ull}) {
            e1->struct_size = size;
            CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext12_want[X12REP_GROWTH] && rp.ext12_path[X12REP_GROWTH].empty());
            CHECK(rp.ext11_want[X11REP_FRAGMENTS] == (size >= 208));
        }
        e12.strain_growth_window = 777; e12.strain_growth_min_own_permille = 5; e12.strain_growth_trim_permille = 7;
        e1->struct_size = 216;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext12_want[X12REP_GROWTH] && rp.gr_window == 5000 && rp.gr_min_own == 500 && rp.gr_trim == 100);
        e1->struct_size = 232;
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.gr_window == 777 && rp.gr_min_own == 5 && rp.gr_trim == 100);
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e1->struct_size = sizeof(e12); e12.strain_growth_file = off; e12.v11.strain_fragments_file = nullptr;
            CHECK(plan_ext_reports(e1, 2, true, rp, err) && !rp.ext12_want[X12REP_GROWTH]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext12_want[X12REP_GROWTH]);
    }
    // ---- the cases of the caller
    if (argc > 1) {
        std::ifstream in(argv[1]);
        CHECK(bool(in));
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            uint64_t min_own, trim, min_windows, n;
            double min_depth;
            CHECK(bool(ss >> min_own >> trim >> min_windows >> min_depth >> n));
            std::vector<uint64_t> len(n), bases(n);
            for (auto &x : len) CHECK(bool(ss >> x));
            for (auto &x : bases) CHECK(bool(ss >> x));
            const auto r = fit_of(len, bases, min_own, trim, min_windows, min_depth, &rc);
            if (rc != 0) { std::printf("fit refused %d\n", rc); continue; }
            std::printf("fit %llu %llu %llu %llu %llu %a %a %a %a %a %s\n", (unsigned long long)r.n_kept, (unsigned long long)r.n_zero, (unsigned long long)r.n_f,
                        (unsigned long long)r.n_fit, (unsigned long long)r.own_len, r.median_depth, r.slope, r.intercept, r.r2, r.index, pantax_hip_growth_status_name(r.status));
        }
    }
    std::printf("growth_plan_check: ok\n");
    return 0;
}
