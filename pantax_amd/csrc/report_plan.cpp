// report_plan.cpp -- see report_plan.hpp
#include "report_plan.hpp"

namespace ptx {

bool plan_reports(const pantax_hip_profiling_config *cfg, int W, bool sharded, ReportPlan &plan, std::string &err) {
    plan = ReportPlan();
    for (int i = 0; i < N_REPORTS; ++i) {
        const char *path = cfg->*REPORTS[i].field;
        plan.path[i] = path ? path : "";
        plan.want[i] = !plan.path[i].empty() && plan.path[i] != "None";
        if (!plan.want[i]) continue;
        if (W > 1 || sharded) {
            err = std::string("profile: the ") + REPORTS[i].what + " (" + REPORTS[i].name + ") needs one rank and an unsharded ingest (world_size " + std::to_string(W) +
                  (sharded ? ", sharded)" : ")");
            return false;
        }
        if (i == REP_COVERAGE) {
            if (cfg->strain_coverage_window < 0) { err = "profile: strain_coverage_window " + std::to_string((long long)cfg->strain_coverage_window); return false; }
            if (cfg->strain_coverage_window > 0) plan.ct_window = (uint64_t)cfg->strain_coverage_window;
        }
        if (i == REP_NEAR_MISS) {
            if (cfg->strain_near_miss_top < 0) { err = "profile: strain_near_miss_top " + std::to_string((int)cfg->strain_near_miss_top); return false; }
            if (cfg->strain_near_miss_top > 0) plan.nm_top = (uint32_t)cfg->strain_near_miss_top;
        }
    }
    return true;
}

void resume_reports(ReportPlan &plan, bool strain, bool full_path, bool strain_done) {
    for (int i = 0; i < N_REPORTS; ++i) plan.run[i] = plan.want[i] && strain && !(full_path && strain_done);
}

}  // namespace ptx
