// pair_report_plan_check.cpp -- the second id space of the file seam's report plan (pantax_amd/csrc/report_plan.hpp: PAIR_REPORTS, the reports about pairs
// of rows of the strain table) and the four-column mirror of the pair sums (hap_pairs_plan.hpp) at their edges.  A program of its own:
// tests/test_pair_report_plan.py compiles it with report_plan.cpp and hap_pairs_plan.cpp by the host compiler under -fsanitize=address,undefined and runs
// it; it returns non-zero at the first mismatch.  The stated order of refusals: the per-strain table REPORTS first, then PAIR_REPORTS.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "hap_pairs_plan.hpp"
#include "report_plan.hpp"

using namespace ptx;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::fprintf(stderr, "pair_report_plan_check:%d: %s\n", __LINE__, #cond);    \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

static const char *const PAIR_W2 = "profile: the pairwise strain evidence report (strain_pair_evidence_file) needs one rank and an unsharded ingest (world_size 2)";
static const char *const PAIR_SHARDED = "profile: the pairwise strain evidence report (strain_pair_evidence_file) needs one rank and an unsharded ingest (world_size 1, sharded)";

static void table() {
    CHECK(N_PAIR_REPORTS == 1 && N_REPORTS == 6);
    CHECK(PAIR_REPORTS[PREP_EVIDENCE].field == &pantax_hip_profiling_config::strain_pair_evidence_file);
    CHECK(std::string(PAIR_REPORTS[PREP_EVIDENCE].name) == "strain_pair_evidence_file" && PAIR_REPORTS[PREP_EVIDENCE].rows);
    // the field is the last of the config: nothing before it moved
    CHECK(offsetof(pantax_hip_profiling_config, strain_pair_evidence_file) > offsetof(pantax_hip_profiling_config, strain_near_miss_top));
    CHECK(offsetof(pantax_hip_profiling_config, strain_pair_evidence_file) + sizeof(const char *) == sizeof(pantax_hip_profiling_config));
}

static void off_and_refused() {
    for (const char *off : {(const char *)nullptr, "", "None"})
        for (const int W : {1, 2})
            for (const bool sharded : {false, true}) {   // off: never refused, never wanted
                pantax_hip_profiling_config cfg{};
                cfg.strain_pair_evidence_file = off;
                ReportPlan plan;
                std::string err = "untouched";
                CHECK(plan_reports(&cfg, W, sharded, plan, err) && err == "untouched");
                CHECK(!plan.pair_want[PREP_EVIDENCE] && !plan.pair_run[PREP_EVIDENCE] && plan.pair_path[PREP_EVIDENCE] == (off ? off : ""));
                resume_reports(plan, true, true, false);
                CHECK(!plan.pair_run[PREP_EVIDENCE] && !plan.any_run() && !plan.rows_run());
            }
    pantax_hip_profiling_config cfg{};
    cfg.strain_pair_evidence_file = "out/pe.tsv";
    ReportPlan plan;
    std::string err;
    CHECK(plan_reports(&cfg, 1, false, plan, err) && err.empty());
    CHECK(plan.pair_want[PREP_EVIDENCE] && !plan.pair_run[PREP_EVIDENCE] && plan.pair_path[PREP_EVIDENCE] == "out/pe.tsv");
    for (int j = 0; j < N_REPORTS; ++j) CHECK(!plan.want[j] && !plan.run[j] && plan.path[j].empty());
    CHECK(!plan.any_run() && !plan.rows_run());
    CHECK(!plan_reports(&cfg, 2, false, plan, err) && err == PAIR_W2);
    CHECK(!plan_reports(&cfg, 1, true, plan, err) && err == PAIR_SHARDED);
    CHECK(!plan_reports(&cfg, 3, true, plan, err) && err.find("strain_pair_evidence_file") != std::string::npos && err.find("world_size 3, sharded") != std::string::npos);
}

static void first_failure() {
    // a per-strain report and the pair report both refused: the per-strain one's message, whichever it is
    for (int a = 0; a < N_REPORTS; ++a) {
        pantax_hip_profiling_config cfg{};
        cfg.*REPORTS[a].field = "a.tsv";
        cfg.strain_pair_evidence_file = "pe.tsv";
        ReportPlan plan;
        std::string err;
        CHECK(!plan_reports(&cfg, 2, false, plan, err));
        CHECK(err.find(REPORTS[a].name) != std::string::npos && err.find("strain_pair_evidence_file") == std::string::npos);
        CHECK(!plan_reports(&cfg, 1, true, plan, err));
        CHECK(err.find(REPORTS[a].name) != std::string::npos && err.find("strain_pair_evidence_file") == std::string::npos);
        CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.want[a] && plan.pair_want[PREP_EVIDENCE]);
    }
    // a parameter of the per-strain table fails before the pair report is looked at; with the per-strain report off, the pair report's refusal stands
    pantax_hip_profiling_config cfg{};
    cfg.strain_coverage_file = "ct.tsv";
    cfg.strain_coverage_window = -1;
    cfg.strain_pair_evidence_file = "pe.tsv";
    ReportPlan plan;
    std::string err;
    CHECK(!plan_reports(&cfg, 1, false, plan, err) && err == "profile: strain_coverage_window -1");
    cfg.strain_coverage_file = "None";
    CHECK(!plan_reports(&cfg, 2, false, plan, err) && err == PAIR_W2);
    CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.pair_want[PREP_EVIDENCE] && plan.ct_window == 10000);
}

static void resume() {
    // {strain, full_path, strain_done} -> runs: the rule of the six, on the pair report alone and beside them
    const bool rows[8][4] = {{false, false, false, false}, {false, false, true, false}, {false, true, false, false}, {false, true, true, false},
                             {true, false, false, true},   {true, false, true, true},   {true, true, false, true},   {true, true, true, false}};
    for (const bool beside : {false, true}) {
        pantax_hip_profiling_config cfg{};
        cfg.strain_pair_evidence_file = "pe.tsv";
        if (beside) for (int i = 0; i < N_REPORTS; ++i) cfg.*REPORTS[i].field = "x.tsv";
        ReportPlan plan;
        std::string err;
        CHECK(plan_reports(&cfg, 1, false, plan, err));
        for (const auto &r : rows) {
            resume_reports(plan, r[0], r[1], r[2]);
            CHECK(plan.pair_run[PREP_EVIDENCE] == r[3]);
            for (int i = 0; i < N_REPORTS; ++i) CHECK(plan.run[i] == (beside && r[3]));   // exactly when the others run
            CHECK(plan.any_run() == r[3] && plan.rows_run() == r[3]);                       // the pair report alone: any_run, and it follows the rows
        }
    }
    // the per-strain reports alone: the pair report neither wanted nor run
    pantax_hip_profiling_config cfg{};
    cfg.read_strain_file = "rs.tsv";
    ReportPlan plan;
    std::string err;
    CHECK(plan_reports(&cfg, 1, false, plan, err));
    resume_reports(plan, true, true, false);
    CHECK(plan.run[REP_READ_STRAINS] && !plan.pair_run[PREP_EVIDENCE] && plan.any_run() && !plan.rows_run());
}

// the block as the kernel leaves it: the block pairs wa <= wb written, the rest zero; value of entry (a, b), column q
static uint64_t val(uint64_t a, uint64_t b, uint32_t q) { return 1000003ull * (a < b ? a : b) + 1009ull * (a < b ? b : a) + 7ull * q + 1ull; }
static void mirror() {
    for (const uint32_t cols : {2u, 4u})
        for (const uint64_t K : {0ull, 1ull, 64ull, 65ull, 130ull, 256ull}) {
            std::vector<uint64_t> block(K * K * cols + 1, 0), was;
            const uint64_t guard = 0xA5A5A5A5A5A5A5A5ull;
            block[K * K * cols] = guard;
            for (uint64_t a = 0; a < K; ++a)
                for (uint64_t b = 0; b < K; ++b)
                    if (a / 64 <= b / 64)
                        for (uint32_t q = 0; q < cols; ++q) block[(a * K + b) * cols + q] = val(a, b, q);
            was = block;
            if (cols == 2) hap_pairs_mirror(block.data(), K); else hap_pairs_mirror(block.data(), K, cols);   // (two columns: the default)
            CHECK(block[K * K * cols] == guard);
            for (uint64_t a = 0; a < K; ++a)
                for (uint64_t b = 0; b < K; ++b)
                    for (uint32_t q = 0; q < cols; ++q) {
                        CHECK(block[(a * K + b) * cols + q] == val(a, b, q));                                    // whole and symmetric, every column its own
                        if (a / 64 <= b / 64) CHECK(block[(a * K + b) * cols + q] == was[(a * K + b) * cols + q]);   // what the kernel wrote is left alone
                    }
        }
}

int main() {
    table();
    off_and_refused();
    first_failure();
    resume();
    mirror();
    std::printf("pair_report_plan_check: ok\n");
    return 0;
}
