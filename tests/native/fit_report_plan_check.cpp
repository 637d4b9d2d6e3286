// fit_report_plan_check.cpp -- the third id space of the file seam's report plan (pantax_amd/csrc/report_plan.hpp: EXT_REPORTS, the reports whose file is
// named in the sized extension pantax_hip_profile_ext) at its edges.  A program of its own: tests/test_fit_report_plan.py compiles it with
// report_plan.cpp by the host compiler under -fsanitize=address,undefined and runs it; it returns non-zero at the first mismatch.  The stated order of
// refusals: REPORTS, then PAIR_REPORTS, then EXT_REPORTS.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "report_plan.hpp"

using namespace ptx;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "fit_report_plan_check:%d: %s\n", __LINE__, #cond);    \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

static const char *const FIT_W2 = "profile: the model fit report (strain_fit_file) needs one rank and an unsharded ingest (world_size 2)";
static const char *const FIT_SHARDED = "profile: the model fit report (strain_fit_file) needs one rank and an unsharded ingest (world_size 1, sharded)";

static pantax_hip_profile_ext ext_with(const char *path) {
    pantax_hip_profile_ext ext{};
    ext.struct_size = sizeof(ext);
    ext.strain_fit_file = path;
    return ext;
}
// plan_reports, then plan_ext_reports on the same plan: what the seam's argument check does
static bool plan_both(const pantax_hip_profiling_config &cfg, const pantax_hip_profile_ext *ext, int W, bool sharded, ReportPlan &plan, std::string &err) {
    return plan_reports(&cfg, W, sharded, plan, err) && plan_ext_reports(ext, W, sharded, plan, err);
}

static void table() {
    CHECK(N_EXT_REPORTS == 1 && N_REPORTS == 6 && N_PAIR_REPORTS == 1);
    CHECK(EXT_REPORTS[XREP_FIT].field == &pantax_hip_profile_ext::strain_fit_file);
    CHECK(std::string(EXT_REPORTS[XREP_FIT].name) == "strain_fit_file" && std::string(EXT_REPORTS[XREP_FIT].what) == "model fit report" && EXT_REPORTS[XREP_FIT].rows);
    // the config keeps its size: its last field is still the pair report's
    CHECK(sizeof(pantax_hip_profiling_config) == offsetof(pantax_hip_profiling_config, strain_pair_evidence_file) + sizeof(const char *));
    // the extension: the size first, then one pointer a report
    CHECK(offsetof(pantax_hip_profile_ext, struct_size) == 0 && sizeof(((pantax_hip_profile_ext *)nullptr)->struct_size) == 8);
    CHECK(offsetof(pantax_hip_profile_ext, strain_fit_file) == 8 && sizeof(pantax_hip_profile_ext) == 16);
}

static void off_and_refused() {
    const pantax_hip_profiling_config cfg{};
    for (const int W : {1, 2})
        for (const bool sharded : {false, true}) {   // off: never refused, never wanted
            for (const char *off : {(const char *)nullptr, "", "None"}) {
                const pantax_hip_profile_ext ext = ext_with(off);
                ReportPlan plan;
                std::string err = "untouched";
                CHECK(plan_both(cfg, &ext, W, sharded, plan, err) && err == "untouched");
                CHECK(!plan.ext_want[XREP_FIT] && !plan.ext_run[XREP_FIT] && plan.ext_path[XREP_FIT] == (off ? off : ""));
                resume_reports(plan, true, true, false);
                CHECK(!plan.ext_run[XREP_FIT] && !plan.any_run() && !plan.rows_run());
            }
            ReportPlan plan;   // no extension at all
            std::string err = "untouched";
            CHECK(plan_both(cfg, nullptr, W, sharded, plan, err) && err == "untouched");
            CHECK(!plan.ext_want[XREP_FIT] && plan.ext_path[XREP_FIT].empty());
            resume_reports(plan, true, true, false);
            CHECK(!plan.any_run() && !plan.rows_run());
        }
    const pantax_hip_profile_ext ext = ext_with("out/fit.tsv");
    ReportPlan plan;
    std::string err;
    CHECK(plan_both(cfg, &ext, 1, false, plan, err) && err.empty());
    CHECK(plan.ext_want[XREP_FIT] && !plan.ext_run[XREP_FIT] && plan.ext_path[XREP_FIT] == "out/fit.tsv");
    for (int j = 0; j < N_REPORTS; ++j) CHECK(!plan.want[j] && !plan.run[j] && plan.path[j].empty());
    CHECK(!plan.pair_want[PREP_EVIDENCE] && !plan.any_run() && !plan.rows_run());
    CHECK(!plan_both(cfg, &ext, 2, false, plan, err) && err == FIT_W2);
    CHECK(!plan_both(cfg, &ext, 1, true, plan, err) && err == FIT_SHARDED);
    CHECK(!plan_both(cfg, &ext, 3, true, plan, err) && err.find("strain_fit_file") != std::string::npos && err.find("world_size 3, sharded") != std::string::npos);
    // a plan that held the report forgets it when planned again without the extension
    CHECK(plan_both(cfg, &ext, 1, false, plan, err) && plan.ext_want[XREP_FIT]);
    CHECK(plan_ext_reports(nullptr, 1, false, plan, err) && !plan.ext_want[XREP_FIT] && plan.ext_path[XREP_FIT].empty());
}

static void sizes() {
    const pantax_hip_profiling_config cfg{};
    ReportPlan plan;
    std::string err;
    // a caller whose header ends before the field: it reads as off, on any number of ranks -- the object really is that short (the sanitizer watches)
    unsigned char *small = static_cast<unsigned char *>(std::malloc(8));
    CHECK(small != nullptr);
    const uint64_t eight = 8;
    std::memcpy(small, &eight, sizeof(eight));
    for (const int W : {1, 2}) {
        err = "untouched";
        CHECK(plan_both(cfg, reinterpret_cast<const pantax_hip_profile_ext *>(small), W, W > 1, plan, err) && err == "untouched");
        CHECK(!plan.ext_want[XREP_FIT] && plan.ext_path[XREP_FIT].empty());
    }
    std::free(small);
    // a caller whose header is longer: the fields this library knows are read
    struct Longer { pantax_hip_profile_ext known; const char *later[3]; } longer{};
    longer.known = ext_with("fit.tsv");
    longer.known.struct_size = sizeof(longer);
    CHECK(plan_both(cfg, &longer.known, 1, false, plan, err) && plan.ext_want[XREP_FIT] && plan.ext_path[XREP_FIT] == "fit.tsv");
    // a size that cannot be a struct of this family: refused whatever the field says, on one rank too
    for (const uint64_t bad : {(uint64_t)0, (uint64_t)4, (uint64_t)7, (uint64_t)12, (uint64_t)15, (uint64_t)17}) {
        for (const char *path : {(const char *)nullptr, "fit.tsv"}) {
            pantax_hip_profile_ext ext = ext_with(path);
            ext.struct_size = bad;
            CHECK(!plan_both(cfg, &ext, 1, false, plan, err));
            CHECK(err.find("struct_size " + std::to_string((unsigned long long)bad)) != std::string::npos && err.find("strain_fit_file") == std::string::npos);
            CHECK(!plan.ext_want[XREP_FIT]);
        }
    }
}

static void first_failure() {
    const pantax_hip_profile_ext ext = ext_with("fit.tsv");
    // a per-strain report and the fit report both refused: the per-strain one's message, whichever it is
    for (int a = 0; a < N_REPORTS; ++a) {
        pantax_hip_profiling_config cfg{};
        cfg.*REPORTS[a].field = "a.tsv";
        ReportPlan plan;
        std::string err;
        CHECK(!plan_both(cfg, &ext, 2, false, plan, err));
        CHECK(err.find(REPORTS[a].name) != std::string::npos && err.find("strain_fit_file") == std::string::npos);
        CHECK(!plan_both(cfg, &ext, 1, true, plan, err));
        CHECK(err.find(REPORTS[a].name) != std::string::npos && err.find("strain_fit_file") == std::string::npos);
        CHECK(plan_both(cfg, &ext, 1, false, plan, err) && plan.want[a] && plan.ext_want[XREP_FIT]);
    }
    // the pair report comes before it too; with the pair report off, the fit report's refusal stands
    pantax_hip_profiling_config cfg{};
    cfg.strain_pair_evidence_file = "pe.tsv";
    ReportPlan plan;
    std::string err;
    CHECK(!plan_both(cfg, &ext, 2, false, plan, err) && err.find("strain_pair_evidence_file") != std::string::npos && err.find("strain_fit_file") == std::string::npos);
    cfg.strain_pair_evidence_file = "None";
    CHECK(!plan_both(cfg, &ext, 2, false, plan, err) && err == FIT_W2);
    // a parameter of the per-strain table fails before the extension is looked at, a bad size included
    cfg.strain_coverage_file = "ct.tsv";
    cfg.strain_coverage_window = -1;
    pantax_hip_profile_ext bad = ext;
    bad.struct_size = 4;
    CHECK(!plan_both(cfg, &bad, 1, false, plan, err) && err == "profile: strain_coverage_window -1");
}

static void resume() {
    // {strain, full_path, strain_done} -> runs: the truth table of report_plan_check.cpp, on the fit report alone and beside the others
    const bool rows[8][4] = {{false, false, false, false}, {false, false, true, false}, {false, true, false, false}, {false, true, true, false},
                             {true, false, false, true},   {true, false, true, true},   {true, true, false, true},   {true, true, true, false}};
    const pantax_hip_profile_ext ext = ext_with("fit.tsv");
    for (const bool beside : {false, true}) {
        pantax_hip_profiling_config cfg{};
        if (beside) {
            for (int i = 0; i < N_REPORTS; ++i) cfg.*REPORTS[i].field = "x.tsv";
            cfg.strain_pair_evidence_file = "pe.tsv";
        }
        ReportPlan plan;
        std::string err;
        CHECK(plan_both(cfg, &ext, 1, false, plan, err));
        for (const auto &r : rows) {
            resume_reports(plan, r[0], r[1], r[2]);
            CHECK(plan.ext_run[XREP_FIT] == r[3]);
            for (int i = 0; i < N_REPORTS; ++i) CHECK(plan.run[i] == (beside && r[3]));
            CHECK(plan.pair_run[PREP_EVIDENCE] == (beside && r[3]));
            CHECK(plan.any_run() == r[3] && plan.rows_run() == r[3]);   // the fit report alone: any_run, and it follows the rows
        }
    }
    // the others alone: the fit report neither wanted nor run
    pantax_hip_profiling_config cfg{};
    cfg.read_strain_file = "rs.tsv";
    ReportPlan plan;
    std::string err;
    CHECK(plan_both(cfg, nullptr, 1, false, plan, err));
    resume_reports(plan, true, true, false);
    CHECK(plan.run[REP_READ_STRAINS] && !plan.ext_run[XREP_FIT] && plan.any_run() && !plan.rows_run());
}

int main() {
    table();
    off_and_refused();
    sizes();
    first_failure();
    resume();
    std::printf("fit_report_plan_check: ok\n");
    return 0;
}
