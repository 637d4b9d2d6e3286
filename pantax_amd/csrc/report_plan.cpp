// report_plan.cpp -- see report_plan.hpp
#include "report_plan.hpp"
#include <algorithm>
#include <cstring>

namespace ptx {

namespace {
// the one rule of a row of any of the tables: its path, whether it is wanted, and the refusal of a wanted report on several ranks or a sharded ingest
template <class Row> bool plan_path(const Row &row, const char *path, int W, bool sharded, std::string &path_out, bool &want, std::string &err) {
    path_out = path ? path : "";
    want = !path_out.empty() && path_out != "None";
    if (want && (W > 1 || sharded)) {
        err = std::string("profile: the ") + row.what + " (" + row.name + ") needs one rank and an unsharded ingest (world_size " + std::to_string(W) + (sharded ? ", sharded)" : ")");
        return false;
    }
    return true;
}
bool plan_row(const ReportRow &row, const pantax_hip_profiling_config *cfg, int W, bool sharded, std::string &path_out, bool &want, std::string &err) {
    return plan_path(row, cfg->*row.field, W, sharded, path_out, want, err);
}
// a field of the sized extension, read only where the caller's struct holds all of it (the caller's object may be shorter than this header's struct: the
// offset comes from an object of our own, the value through a copy of its bytes)
template <class Ext, class T> bool ext_value(const pantax_hip_profile_ext *ext, T Ext::*field, T &value) {
    if (!ext) return false;
    static const Ext layout{};
    const size_t at = (size_t)(reinterpret_cast<const char *>(&(layout.*field)) - reinterpret_cast<const char *>(&layout));
    if (at + sizeof(T) > ext->struct_size) return false;
    std::memcpy(&value, reinterpret_cast<const char *>(ext) + at, sizeof(value));
    return true;
}
// (Ext: pantax_hip_profile_ext, or pantax_hip_profile_ext2 / _ext3 / _ext4 / _ext5 / _ext6 / _ext7 / _ext8 / _ext9 / _ext10 / _ext11 / _ext12, which begin with it)
template <class Ext> const char *ext_field(const pantax_hip_profile_ext *ext, const char *Ext::*field) {
    const char *value = nullptr;
    return ext_value(ext, field, value) ? value : nullptr;
}
// ... and when a wanted report runs
bool runs(bool want, bool strain, bool full_path, bool strain_done) { return want && strain && !(full_path && strain_done); }
}  // namespace

bool plan_reports(const pantax_hip_profiling_config *cfg, int W, bool sharded, ReportPlan &plan, std::string &err) {
    plan = ReportPlan();
    for (int i = 0; i < N_REPORTS; ++i) {
        if (!plan_row(REPORTS[i], cfg, W, sharded, plan.path[i], plan.want[i], err)) return false;
        if (!plan.want[i]) continue;
        if (i == REP_COVERAGE) {
            if (cfg->strain_coverage_window < 0) { err = "profile: strain_coverage_window " + std::to_string((long long)cfg->strain_coverage_window); return false; }
            if (cfg->strain_coverage_window > 0) plan.ct_window = (uint64_t)cfg->strain_coverage_window;
        }
        if (i == REP_NEAR_MISS) {
            if (cfg->strain_near_miss_top < 0) { err = "profile: strain_near_miss_top " + std::to_string((int)cfg->strain_near_miss_top); return false; }
            if (cfg->strain_near_miss_top > 0) plan.nm_top = (uint32_t)cfg->strain_near_miss_top;
        }
    }
    for (int i = 0; i < N_PAIR_REPORTS; ++i)
        if (!plan_row(PAIR_REPORTS[i], cfg, W, sharded, plan.pair_path[i], plan.pair_want[i], err)) return false;
    return true;
}

bool plan_ext_reports(const pantax_hip_profile_ext *ext, int W, bool sharded, ReportPlan &plan, std::string &err) {
    for (int i = 0; i < N_EXT_REPORTS; ++i) { plan.ext_path[i].clear(); plan.ext_want[i] = plan.ext_run[i] = false; }
    for (int i = 0; i < N_EXT2_REPORTS; ++i) { plan.ext2_path[i].clear(); plan.ext2_want[i] = plan.ext2_run[i] = false; }
    for (int i = 0; i < N_EXT3_REPORTS; ++i) { plan.ext3_path[i].clear(); plan.ext3_want[i] = plan.ext3_run[i] = false; }
    for (int i = 0; i < N_EXT4_REPORTS; ++i) { plan.ext4_path[i].clear(); plan.ext4_want[i] = plan.ext4_run[i] = false; }
    for (int i = 0; i < N_EXT5_REPORTS; ++i) { plan.ext5_path[i].clear(); plan.ext5_want[i] = plan.ext5_run[i] = false; }
    for (int i = 0; i < N_EXT6_REPORTS; ++i) { plan.ext6_path[i].clear(); plan.ext6_want[i] = plan.ext6_run[i] = false; }
    for (int i = 0; i < N_EXT7_REPORTS; ++i) { plan.ext7_path[i].clear(); plan.ext7_want[i] = plan.ext7_run[i] = false; }
    for (int i = 0; i < N_EXT8_REPORTS; ++i) { plan.ext8_path[i].clear(); plan.ext8_want[i] = plan.ext8_run[i] = false; }
    for (int i = 0; i < N_EXT9_REPORTS; ++i) { plan.ext9_path[i].clear(); plan.ext9_want[i] = plan.ext9_run[i] = false; }
    for (int i = 0; i < N_EXT10_REPORTS; ++i) { plan.ext10_path[i].clear(); plan.ext10_want[i] = plan.ext10_run[i] = false; }
    for (int i = 0; i < N_EXT11_REPORTS; ++i) { plan.ext11_path[i].clear(); plan.ext11_want[i] = plan.ext11_run[i] = false; }
    for (int i = 0; i < N_EXT12_REPORTS; ++i) { plan.ext12_path[i].clear(); plan.ext12_want[i] = plan.ext12_run[i] = false; }
    if (ext && (ext->struct_size < 8 || ext->struct_size % 8 != 0)) {
        err = "profile: pantax_hip_profile_ext.struct_size " + std::to_string((unsigned long long)ext->struct_size) + " (a multiple of 8, at least 8)";
        return false;
    }
    for (int i = 0; i < N_EXT_REPORTS; ++i)
        if (!plan_path(EXT_REPORTS[i], ext_field(ext, EXT_REPORTS[i].field), W, sharded, plan.ext_path[i], plan.ext_want[i], err)) return false;
    for (int i = 0; i < N_EXT2_REPORTS; ++i)
        if (!plan_path(EXT2_REPORTS[i], ext_field(ext, EXT2_REPORTS[i].field), W, sharded, plan.ext2_path[i], plan.ext2_want[i], err)) return false;
    for (int i = 0; i < N_EXT3_REPORTS; ++i)
        if (!plan_path(EXT3_REPORTS[i], ext_field(ext, EXT3_REPORTS[i].field), W, sharded, plan.ext3_path[i], plan.ext3_want[i], err)) return false;
    for (int i = 0; i < N_EXT4_REPORTS; ++i)
        if (!plan_path(EXT4_REPORTS[i], ext_field(ext, EXT4_REPORTS[i].field), W, sharded, plan.ext4_path[i], plan.ext4_want[i], err)) return false;
    for (int i = 0; i < N_EXT5_REPORTS; ++i)
        if (!plan_path(EXT5_REPORTS[i], ext_field(ext, EXT5_REPORTS[i].field), W, sharded, plan.ext5_path[i], plan.ext5_want[i], err)) return false;
    for (int i = 0; i < N_EXT6_REPORTS; ++i)
        if (!plan_path(EXT6_REPORTS[i], ext_field(ext, EXT6_REPORTS[i].field), W, sharded, plan.ext6_path[i], plan.ext6_want[i], err)) return false;
    for (int i = 0; i < N_EXT7_REPORTS; ++i)
        if (!plan_path(EXT7_REPORTS[i], ext_field(ext, EXT7_REPORTS[i].field), W, sharded, plan.ext7_path[i], plan.ext7_want[i], err)) return false;
    for (int i = 0; i < N_EXT8_REPORTS; ++i)
        if (!plan_path(EXT8_REPORTS[i], ext_field(ext, EXT8_REPORTS[i].field), W, sharded, plan.ext8_path[i], plan.ext8_want[i], err)) return false;
    for (int i = 0; i < N_EXT9_REPORTS; ++i)
        if (!plan_path(EXT9_REPORTS[i], ext_field(ext, EXT9_REPORTS[i].field), W, sharded, plan.ext9_path[i], plan.ext9_want[i], err)) return false;
    for (int i = 0; i < N_EXT10_REPORTS; ++i)
        if (!plan_path(EXT10_REPORTS[i], ext_field(ext, EXT10_REPORTS[i].field), W, sharded, plan.ext10_path[i], plan.ext10_want[i], err)) return false;
    for (int i = 0; i < N_EXT11_REPORTS; ++i)
        if (!plan_path(EXT11_REPORTS[i], ext_field(ext, EXT11_REPORTS[i].field), W, sharded, plan.ext11_path[i], plan.ext11_want[i], err)) return false;
    for (int i = 0; i < N_EXT12_REPORTS; ++i)
        if (!plan_path(EXT12_REPORTS[i], ext_field(ext, EXT12_REPORTS[i].field), W, sharded, plan.ext12_path[i], plan.ext12_want[i], err)) return false;
    plan.bs_replicates = 100; plan.bs_seed = 42; plan.ai_top = 5; plan.em_classes = 10; plan.em_iterations = 1000;
    plan.sg_min = 1000; plan.sg_bridge = 100; plan.sg_peak = 10; plan.mo_top = 10; plan.rs_top = 5; plan.lk_top = 10;
    plan.rf_levels = 5; plan.rf_replicates = 5; plan.rf_seed = 42;
    plan.gr_window = 5000; plan.gr_min_own = 500; plan.gr_trim = 100;
    if (plan.ext2_want[X2REP_BOOTSTRAP]) {
        uint64_t n = 0, seed = 42;
        if (ext_value(ext, &pantax_hip_profile_ext2::strain_bootstrap_replicates, n) && n > 0xFFFFFFFEull) {
            err = "profile: strain_bootstrap_replicates " + std::to_string((unsigned long long)n) + " (at most 2^32 - 2)";
            return false;
        }
        if (n) plan.bs_replicates = (uint32_t)n;
        if (ext_value(ext, &pantax_hip_profile_ext2::strain_bootstrap_seed, seed)) plan.bs_seed = seed;
    }
    if (plan.ext4_want[X4REP_ADDIN]) {
        uint64_t top = 0;
        if (ext_value(ext, &pantax_hip_profile_ext4::strain_addin_top, top) && top) plan.ai_top = (uint32_t)std::min<uint64_t>(top, 0xFFFFFFFFull);
    }
    if (plan.ext5_want[X5REP_EM]) {
        uint64_t n = 0, it = 0;
        if (ext_value(ext, &pantax_hip_profile_ext5::strain_em_classes, n) && n) plan.em_classes = n;
        if (ext_value(ext, &pantax_hip_profile_ext5::strain_em_iterations, it) && it) plan.em_iterations = (uint32_t)std::min<uint64_t>(it, 0xFFFFFFFFull);
    }
    if (plan.ext6_want[X6REP_SEGMENTS]) {
        uint64_t n = 0, b = 0, f = 0;
        if (ext_value(ext, &pantax_hip_profile_ext6::strain_segments_min, n) && n) plan.sg_min = n;
        if (ext_value(ext, &pantax_hip_profile_ext6::strain_segments_bridge, b) && b) plan.sg_bridge = b - 1;   // the field holds bridge + 1
        if (ext_value(ext, &pantax_hip_profile_ext6::strain_segments_peak, f) && f) plan.sg_peak = f == PANTAX_HIP_SEGMENTS_PEAK_OFF ? 0 : f;
    }
    if (plan.ext7_want[X7REP_MOSAIC]) {
        uint64_t top = 0;
        if (ext_value(ext, &pantax_hip_profile_ext7::strain_mosaic_top, top) && top) plan.mo_top = top == PANTAX_HIP_MOSAIC_TOP_OFF ? 0 : top;
    }
    if (plan.ext8_want[X8REP_RESCUE]) {
        uint64_t top = 0;
        if (ext_value(ext, &pantax_hip_profile_ext8::strain_rescue_top, top) && top) plan.rs_top = (uint32_t)std::min<uint64_t>(top, 0xFFFFFFFFull);
    }
    if (plan.ext9_want[X9REP_LINKS]) {
        uint64_t top = 0;
        if (ext_value(ext, &pantax_hip_profile_ext9::strain_links_top, top) && top) plan.lk_top = top;
    }
    if (plan.ext10_want[X10REP_RAREFY]) {
        uint64_t n = 0, r = 0, seed = 42;
        if (ext_value(ext, &pantax_hip_profile_ext10::strain_rarefy_levels, n) && n > 16) {
            err = "profile: strain_rarefy_levels " + std::to_string((unsigned long long)n) + " (at most 16)";
            return false;
        }
        if (n) plan.rf_levels = (uint32_t)n;
        if (ext_value(ext, &pantax_hip_profile_ext10::strain_rarefy_replicates, r) && r > 0xFFFFFFFFull / 16) {
            err = "profile: strain_rarefy_replicates " + std::to_string((unsigned long long)r) + " (at most 2^28 - 1)";
            return false;
        }
        if (r) plan.rf_replicates = (uint32_t)r;
        if (ext_value(ext, &pantax_hip_profile_ext10::strain_rarefy_seed, seed)) plan.rf_seed = seed;
    }
    if (plan.ext12_want[X12REP_GROWTH]) {
        uint64_t w = 0, own = 0, trim = 0;
        if (ext_value(ext, &pantax_hip_profile_ext12::strain_growth_window, w) && w) plan.gr_window = w;
        if (ext_value(ext, &pantax_hip_profile_ext12::strain_growth_min_own_permille, own) && own > 1000) {
            err = "profile: strain_growth_min_own_permille " + std::to_string((unsigned long long)own) + " (at most 1000)";
            return false;
        }
        if (own) plan.gr_min_own = own;
        if (ext_value(ext, &pantax_hip_profile_ext12::strain_growth_trim_permille, trim) && trim >= 500) {
            err = "profile: strain_growth_trim_permille " + std::to_string((unsigned long long)trim) + " (below 500)";
            return false;
        }
        if (trim) plan.gr_trim = trim;
    }
    return true;
}

void resume_reports(ReportPlan &plan, bool strain, bool full_path, bool strain_done) {
    for (int i = 0; i < N_REPORTS; ++i) plan.run[i] = runs(plan.want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_PAIR_REPORTS; ++i) plan.pair_run[i] = runs(plan.pair_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT_REPORTS; ++i) plan.ext_run[i] = runs(plan.ext_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT2_REPORTS; ++i) plan.ext2_run[i] = runs(plan.ext2_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT3_REPORTS; ++i) plan.ext3_run[i] = runs(plan.ext3_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT4_REPORTS; ++i) plan.ext4_run[i] = runs(plan.ext4_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT5_REPORTS; ++i) plan.ext5_run[i] = runs(plan.ext5_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT6_REPORTS; ++i) plan.ext6_run[i] = runs(plan.ext6_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT7_REPORTS; ++i) plan.ext7_run[i] = runs(plan.ext7_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT8_REPORTS; ++i) plan.ext8_run[i] = runs(plan.ext8_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT9_REPORTS; ++i) plan.ext9_run[i] = runs(plan.ext9_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT10_REPORTS; ++i) plan.ext10_run[i] = runs(plan.ext10_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT11_REPORTS; ++i) plan.ext11_run[i] = runs(plan.ext11_want[i], strain, full_path, strain_done);
    for (int i = 0; i < N_EXT12_REPORTS; ++i) plan.ext12_run[i] = runs(plan.ext12_want[i], strain, full_path, strain_done);
}

}  // namespace ptx
