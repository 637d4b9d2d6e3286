// report_plan_check.cpp -- the per-strain reports' plan (pantax_amd/csrc/report_plan.hpp) at its edges.  A program of its own: tests/test_report_plan.py
// compiles it with report_plan.cpp by the host compiler under -fsanitize=address,undefined and runs it; it returns non-zero at the first mismatch.
// The refusal texts are the literal strings the seam's argument check spelled out report by report before the table existed.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "report_plan.hpp"

using namespace ptx;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "report_plan_check:%d: %s\n", __LINE__, #cond);    \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

static const char *const REFUSAL_W2[N_REPORTS] = {
    "profile: the per-read strain report (read_strain_file) needs one rank and an unsharded ingest (world_size 2)",
    "profile: the per-strain coverage track (strain_coverage_file) needs one rank and an unsharded ingest (world_size 2)",
    "profile: the per-strain node evidence report (strain_evidence_file) needs one rank and an unsharded ingest (world_size 2)",
    "profile: the per-strain read support report (strain_read_support_file) needs one rank and an unsharded ingest (world_size 2)",
    "profile: the per-strain depth distribution report (strain_depth_file) needs one rank and an unsharded ingest (world_size 2)",
    "profile: the unreported-strain near-miss report (strain_near_miss_file) needs one rank and an unsharded ingest (world_size 2)",
};
static const char *const REFUSAL_SHARDED[N_REPORTS] = {
    "profile: the per-read strain report (read_strain_file) needs one rank and an unsharded ingest (world_size 1, sharded)",
    "profile: the per-strain coverage track (strain_coverage_file) needs one rank and an unsharded ingest (world_size 1, sharded)",
    "profile: the per-strain node evidence report (strain_evidence_file) needs one rank and an unsharded ingest (world_size 1, sharded)",
    "profile: the per-strain read support report (strain_read_support_file) needs one rank and an unsharded ingest (world_size 1, sharded)",
    "profile: the per-strain depth distribution report (strain_depth_file) needs one rank and an unsharded ingest (world_size 1, sharded)",
    "profile: the unreported-strain near-miss report (strain_near_miss_file) needs one rank and an unsharded ingest (world_size 1, sharded)",
};

static pantax_hip_profiling_config with(int i, const char *path) {
    pantax_hip_profiling_config cfg{};
    cfg.*REPORTS[i].field = path;
    return cfg;
}

static void table() {
    // the table's order is the enum's; every row names the field it points to
    CHECK(REPORTS[REP_READ_STRAINS].field == &pantax_hip_profiling_config::read_strain_file && std::string(REPORTS[REP_READ_STRAINS].name) == "read_strain_file");
    CHECK(REPORTS[REP_COVERAGE].field == &pantax_hip_profiling_config::strain_coverage_file && std::string(REPORTS[REP_COVERAGE].name) == "strain_coverage_file");
    CHECK(REPORTS[REP_EVIDENCE].field == &pantax_hip_profiling_config::strain_evidence_file && std::string(REPORTS[REP_EVIDENCE].name) == "strain_evidence_file");
    CHECK(REPORTS[REP_READ_SUPPORT].field == &pantax_hip_profiling_config::strain_read_support_file && std::string(REPORTS[REP_READ_SUPPORT].name) == "strain_read_support_file");
    CHECK(REPORTS[REP_DEPTH].field == &pantax_hip_profiling_config::strain_depth_file && std::string(REPORTS[REP_DEPTH].name) == "strain_depth_file");
    CHECK(REPORTS[REP_NEAR_MISS].field == &pantax_hip_profiling_config::strain_near_miss_file && std::string(REPORTS[REP_NEAR_MISS].name) == "strain_near_miss_file");
    CHECK(N_REPORTS == 6);
}

static void paths_and_refusals() {
    for (int i = 0; i < N_REPORTS; ++i) {
        for (const char *off : {(const char *)nullptr, "", "None"})
            for (const int W : {1, 2})
                for (const bool sharded : {false, true}) {   // a report that is off is never refused
                    const pantax_hip_profiling_config cfg = with(i, off);
                    ReportPlan plan;
                    std::string err = "untouched";
                    CHECK(plan_reports(&cfg, W, sharded, plan, err) && err == "untouched");
                    for (int j = 0; j < N_REPORTS; ++j) CHECK(!plan.want[j] && !plan.run[j]);
                    CHECK(plan.path[i] == (off ? off : "") && plan.ct_window == 10000 && plan.nm_top == 5u && !plan.any_run() && !plan.rows_run());
                }
        const pantax_hip_profiling_config cfg = with(i, "out/report.tsv");
        ReportPlan plan;
        std::string err;
        CHECK(plan_reports(&cfg, 1, false, plan, err) && err.empty());
        for (int j = 0; j < N_REPORTS; ++j) CHECK(plan.want[j] == (j == i) && !plan.run[j] && plan.path[j] == (j == i ? "out/report.tsv" : ""));
        CHECK(plan.ct_window == 10000 && plan.nm_top == 5u);
        CHECK(!plan_reports(&cfg, 2, false, plan, err) && err == REFUSAL_W2[i]);
        CHECK(!plan_reports(&cfg, 1, true, plan, err) && err == REFUSAL_SHARDED[i]);
    }
}

static void parameters() {
    ReportPlan plan;
    std::string err;
    // the window: checked only when the track is wanted
    pantax_hip_profiling_config cfg = with(REP_COVERAGE, "ct.tsv");
    cfg.strain_coverage_window = -1;
    CHECK(!plan_reports(&cfg, 1, false, plan, err) && err == "profile: strain_coverage_window -1");
    cfg.strain_coverage_window = 0;
    CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.ct_window == 10000);
    cfg.strain_coverage_window = 7;
    CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.ct_window == 7);
    cfg.strain_coverage_file = "None";
    cfg.strain_coverage_window = -1;
    CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.ct_window == 10000 && !plan.want[REP_COVERAGE]);
    cfg.strain_coverage_window = 7;   // not wanted: the default stands
    CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.ct_window == 10000);
    // the top
    cfg = with(REP_NEAR_MISS, "nm.tsv");
    cfg.strain_near_miss_top = -1;
    CHECK(!plan_reports(&cfg, 1, false, plan, err) && err == "profile: strain_near_miss_top -1");
    cfg.strain_near_miss_top = 0;
    CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.nm_top == 5u);
    cfg.strain_near_miss_top = 3;
    CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.nm_top == 3u);
    cfg.strain_near_miss_file = nullptr;
    cfg.strain_near_miss_top = -1;
    CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.nm_top == 5u && !plan.want[REP_NEAR_MISS]);
    cfg.strain_near_miss_top = 3;
    CHECK(plan_reports(&cfg, 1, false, plan, err) && plan.nm_top == 5u);
}

static void first_failure() {
    ReportPlan plan;
    std::string err;
    for (int a = 0; a < N_REPORTS; ++a)
        for (int b = a + 1; b < N_REPORTS; ++b) {   // two refused reports: the earlier one's message
            pantax_hip_profiling_config cfg = with(a, "a.tsv");
            cfg.*REPORTS[b].field = "b.tsv";
            CHECK(!plan_reports(&cfg, 2, false, plan, err) && err == REFUSAL_W2[a]);
            CHECK(!plan_reports(&cfg, 1, true, plan, err) && err == REFUSAL_SHARDED[a]);
        }
    pantax_hip_profiling_config cfg = with(REP_READ_STRAINS, "rs.tsv");   // read strains refused together with a negative window
    cfg.strain_coverage_file = "ct.tsv";
    cfg.strain_coverage_window = -1;
    CHECK(!plan_reports(&cfg, 2, false, plan, err) && err == REFUSAL_W2[REP_READ_STRAINS]);
    cfg.read_strain_file = nullptr;   // the track's refusal comes before its own window
    CHECK(!plan_reports(&cfg, 2, false, plan, err) && err == REFUSAL_W2[REP_COVERAGE]);
    cfg.strain_near_miss_file = "nm.tsv";   // on one rank: the window before the top
    cfg.strain_near_miss_top = -1;
    CHECK(!plan_reports(&cfg, 1, false, plan, err) && err == "profile: strain_coverage_window -1");
    cfg.strain_coverage_window = 0;
    CHECK(!plan_reports(&cfg, 1, false, plan, err) && err == "profile: strain_near_miss_top -1");
    cfg.strain_evidence_file = "ev.tsv";   // a negative window with a later report refused: the track comes first in the table
    cfg.strain_coverage_window = -1;
    cfg.strain_coverage_file = "";
    CHECK(!plan_reports(&cfg, 2, false, plan, err) && err == REFUSAL_W2[REP_EVIDENCE]);
}

static void resume() {
    pantax_hip_profiling_config cfg{};
    for (int i = 0; i < N_REPORTS; ++i) cfg.*REPORTS[i].field = i == REP_DEPTH ? "None" : "x.tsv";
    ReportPlan plan;
    std::string err;
    CHECK(plan_reports(&cfg, 1, false, plan, err));
    // a wanted report runs with the strain level unless a full run finds the strain table done: {strain, full_path, strain_done} -> runs
    const bool rows[8][4] = {{false, false, false, false}, {false, false, true, false}, {false, true, false, false}, {false, true, true, false},
                             {true, false, false, true},   {true, false, true, true},   {true, true, false, true},   {true, true, true, false}};
    for (const auto &r : rows) {
        resume_reports(plan, r[0], r[1], r[2]);
        for (int i = 0; i < N_REPORTS; ++i) CHECK(plan.run[i] == (r[3] && i != REP_DEPTH));
        CHECK(plan.any_run() == r[3] && plan.rows_run() == r[3]);
    }
    for (int i = 0; i < N_REPORTS; ++i) {   // rows_run: exactly the four reports that follow the rows of the strain table
        const pantax_hip_profiling_config one = with(i, "x.tsv");
        CHECK(plan_reports(&one, 1, false, plan, err));
        CHECK(!plan.any_run() && !plan.rows_run());
        resume_reports(plan, true, true, false);
        const bool rows = i == REP_COVERAGE || i == REP_EVIDENCE || i == REP_READ_SUPPORT || i == REP_DEPTH;
        CHECK(plan.any_run() && plan.rows_run() == rows && REPORTS[i].rows == rows);
    }
}

int main() {
    table();
    paths_and_refusals();
    parameters();
    first_failure();
    resume();
    std::printf("report_plan_check: ok\n");
    return 0;
}
