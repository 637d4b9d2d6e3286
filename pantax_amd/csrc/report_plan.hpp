// report_plan.hpp -- the per-strain reports of the file seam (pantax_hip_profile) as one table: which config field switches a report on, what its refusal
// calls it, whether it follows the rows of strain_abundance.txt.  plan_reports / resume_reports decide from plain values which reports this call wants
// and runs; nothing else in the seam spells a report's field name or repeats the rule.  pantax_hip.h and standard headers only:
// tests/native/report_plan_check.cpp, pair_report_plan_check.cpp, fit_report_plan_check.cpp, bootstrap_plan_check.cpp, dropout_plan_check.cpp, addin_plan_check.cpp, read_em_check.cpp, segments_check.cpp, mosaic_check.cpp, rescue_check.cpp, links_check.cpp, rarefy_check.cpp, fragments_plan_check.cpp and growth_plan_check.cpp compile this with the host compiler alone.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/pantax_hip.h"

namespace ptx {

// in the order of the device calls within a group and of the files written
enum ReportId { REP_READ_STRAINS, REP_COVERAGE, REP_EVIDENCE, REP_READ_SUPPORT, REP_DEPTH, REP_NEAR_MISS, N_REPORTS };
struct ReportRow {
    const char *pantax_hip_profiling_config::*field;   // the report's file: null, "" or "None" = off
    const char *name;                                  // the field's name ...
    const char *what;                                  // ... and the report's noun phrase, both for the refusal
    bool rows;                                         // follows the rows of the strain table (a TrackRow consumer)
};
constexpr ReportRow REPORTS[N_REPORTS] = {
    {&pantax_hip_profiling_config::read_strain_file, "read_strain_file", "per-read strain report", false},
    {&pantax_hip_profiling_config::strain_coverage_file, "strain_coverage_file", "per-strain coverage track", true},
    {&pantax_hip_profiling_config::strain_evidence_file, "strain_evidence_file", "per-strain node evidence report", true},
    {&pantax_hip_profiling_config::strain_read_support_file, "strain_read_support_file", "per-strain read support report", true},
    {&pantax_hip_profiling_config::strain_depth_file, "strain_depth_file", "per-strain depth distribution report", true},
    {&pantax_hip_profiling_config::strain_near_miss_file, "strain_near_miss_file", "unreported-strain near-miss report", false},
};
// A second id space: the reports about PAIRS of rows of the strain table.  Same row type, same rule (plan_reports / resume_reports apply it to both
// tables through one helper), own want / run / path in the plan.  In the stated order of refusals the per-strain table comes first, then this one.
enum PairReportId { PREP_EVIDENCE, N_PAIR_REPORTS };
constexpr ReportRow PAIR_REPORTS[N_PAIR_REPORTS] = {
    {&pantax_hip_profiling_config::strain_pair_evidence_file, "strain_pair_evidence_file", "pairwise strain evidence report", true},
};
// A third id space: the reports whose file is named in the sized extension of the seam (pantax_hip_profile_ext; pantax_hip_profiling_config keeps its
// size, and the two tables above their rows).  Same columns but for the struct the member pointer goes into, same rule (plan_ext_reports); checked after
// the two tables above.  A later report is a field appended to pantax_hip_profile_ext and a row here.
enum ExtReportId { XREP_FIT, N_EXT_REPORTS };
struct ExtReportRow {
    const char *pantax_hip_profile_ext::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr ExtReportRow EXT_REPORTS[N_EXT_REPORTS] = {
    {&pantax_hip_profile_ext::strain_fit_file, "strain_fit_file", "model fit report", true},
};
// ... and its continuation: pantax_hip_profile_ext is closed at strain_fit_file as well (a committed host check pins its 16 bytes and N_EXT_REPORTS = 1), so
// the reports named behind it are fields of pantax_hip_profile_ext2, which begins with the first version, and rows of this table.  Same columns, same rule,
// same refusal wording (plan_ext_reports, which is handed the first version and reads the longer struct's fields where struct_size holds them); checked
// after EXT_REPORTS.  A later report is a field appended to pantax_hip_profile_ext2 and a row here.
enum Ext2ReportId { X2REP_BOOTSTRAP, N_EXT2_REPORTS };
struct Ext2ReportRow {
    const char *pantax_hip_profile_ext2::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext2ReportRow EXT2_REPORTS[N_EXT2_REPORTS] = {
    {&pantax_hip_profile_ext2::strain_bootstrap_file, "strain_bootstrap_file", "bootstrap report", true},
};
// ... and once more: pantax_hip_profile_ext2 is closed at strain_bootstrap_seed (a committed host check pins its 40 bytes and N_EXT2_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext3, which begins with the second version, and rows of this table, checked after EXT2_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext3 and a row here.
enum Ext3ReportId { X3REP_DROPOUT, N_EXT3_REPORTS };
struct Ext3ReportRow {
    const char *pantax_hip_profile_ext3::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext3ReportRow EXT3_REPORTS[N_EXT3_REPORTS] = {
    {&pantax_hip_profile_ext3::strain_dropout_file, "strain_dropout_file", "leave-one-out report", true},
};
// ... and once more: pantax_hip_profile_ext3 is closed at strain_dropout_file (a committed host check pins its 48 bytes and N_EXT3_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext4, which begins with the third version, and rows of this table, checked after EXT3_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext4 and a row here.
enum Ext4ReportId { X4REP_ADDIN, N_EXT4_REPORTS };
struct Ext4ReportRow {
    const char *pantax_hip_profile_ext4::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext4ReportRow EXT4_REPORTS[N_EXT4_REPORTS] = {
    {&pantax_hip_profile_ext4::strain_addin_file, "strain_addin_file", "add-one report", false},
};
// ... and once more: pantax_hip_profile_ext4 is closed at strain_addin_top (a committed host check pins its 64 bytes and N_EXT4_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext5, which begins with the fourth version, and rows of this table, checked after EXT4_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext5 and a row here.
enum Ext5ReportId { X5REP_EM, N_EXT5_REPORTS };
struct Ext5ReportRow {
    const char *pantax_hip_profile_ext5::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext5ReportRow EXT5_REPORTS[N_EXT5_REPORTS] = {
    {&pantax_hip_profile_ext5::strain_em_file, "strain_em_file", "read class report", true},
};
// ... and once more: pantax_hip_profile_ext5 is closed at strain_em_iterations (a committed host check pins its 88 bytes and N_EXT5_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext6, which begins with the fifth version, and rows of this table, checked after EXT5_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext6 and a row here.
enum Ext6ReportId { X6REP_SEGMENTS, N_EXT6_REPORTS };
struct Ext6ReportRow {
    const char *pantax_hip_profile_ext6::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext6ReportRow EXT6_REPORTS[N_EXT6_REPORTS] = {
    {&pantax_hip_profile_ext6::strain_segments_file, "strain_segments_file", "segment report", true},
};
// ... and once more: pantax_hip_profile_ext6 is closed at strain_segments_peak (a committed host check pins its 120 bytes and N_EXT6_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext7, which begins with the sixth version, and rows of this table, checked after EXT6_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext7 and a row here.
enum Ext7ReportId { X7REP_MOSAIC, N_EXT7_REPORTS };
struct Ext7ReportRow {
    const char *pantax_hip_profile_ext7::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext7ReportRow EXT7_REPORTS[N_EXT7_REPORTS] = {
    {&pantax_hip_profile_ext7::strain_mosaic_file, "strain_mosaic_file", "mosaic read report", true},
};
// ... and once more: pantax_hip_profile_ext7 is closed at strain_mosaic_top (a committed host check pins its 136 bytes and N_EXT7_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext8, which begins with the seventh version, and rows of this table, checked after EXT7_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext8 and a row here.
enum Ext8ReportId { X8REP_RESCUE, N_EXT8_REPORTS };
struct Ext8ReportRow {
    const char *pantax_hip_profile_ext8::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext8ReportRow EXT8_REPORTS[N_EXT8_REPORTS] = {
    {&pantax_hip_profile_ext8::strain_rescue_file, "strain_rescue_file", "read rescue report", false},
};
// ... and once more: pantax_hip_profile_ext8 is closed at strain_rescue_top (a committed host check pins its 152 bytes and N_EXT8_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext9, which begins with the eighth version, and rows of this table, checked after EXT8_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext9 and a row here.
enum Ext9ReportId { X9REP_LINKS, N_EXT9_REPORTS };
struct Ext9ReportRow {
    const char *pantax_hip_profile_ext9::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext9ReportRow EXT9_REPORTS[N_EXT9_REPORTS] = {
    {&pantax_hip_profile_ext9::strain_links_file, "strain_links_file", "link support report", true},   // (its strain and break rows follow the rows of strain_abundance.txt)
};
// ... and once more: pantax_hip_profile_ext9 is closed at strain_links_top (a committed host check pins its 168 bytes and N_EXT9_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext10, which begins with the ninth version, and rows of this table, checked after EXT9_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext10 and a row here.
enum Ext10ReportId { X10REP_RAREFY, N_EXT10_REPORTS };
struct Ext10ReportRow {
    const char *pantax_hip_profile_ext10::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext10ReportRow EXT10_REPORTS[N_EXT10_REPORTS] = {
    {&pantax_hip_profile_ext10::strain_rarefy_file, "strain_rarefy_file", "rarefaction report", true},
};
// ... and once more: pantax_hip_profile_ext10 is closed at strain_rarefy_seed (a committed host check pins its 200 bytes and N_EXT10_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext11, which begins with the tenth version, and rows of this table, checked after EXT10_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext11 and a row here.
enum Ext11ReportId { X11REP_FRAGMENTS, N_EXT11_REPORTS };
struct Ext11ReportRow {
    const char *pantax_hip_profile_ext11::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext11ReportRow EXT11_REPORTS[N_EXT11_REPORTS] = {
    {&pantax_hip_profile_ext11::strain_fragments_file, "strain_fragments_file", "fragment support report", true},
};
// ... and once more: pantax_hip_profile_ext11 is closed at strain_fragments_file (a committed host check pins its 208 bytes and N_EXT11_REPORTS = 1); the reports
// named behind it are fields of pantax_hip_profile_ext12, which begins with the eleventh version, and rows of this table, checked after EXT11_REPORTS.  A later
// report is a field appended to pantax_hip_profile_ext12 and a row here.
enum Ext12ReportId { X12REP_GROWTH, N_EXT12_REPORTS };
struct Ext12ReportRow {
    const char *pantax_hip_profile_ext12::*field;
    const char *name;
    const char *what;
    bool rows;
};
constexpr Ext12ReportRow EXT12_REPORTS[N_EXT12_REPORTS] = {
    {&pantax_hip_profile_ext12::strain_growth_file, "strain_growth_file", "replication index report", true},
};
struct ReportPlan {
    std::string path[N_REPORTS], pair_path[N_PAIR_REPORTS], ext_path[N_EXT_REPORTS], ext2_path[N_EXT2_REPORTS], ext3_path[N_EXT3_REPORTS], ext4_path[N_EXT4_REPORTS], ext5_path[N_EXT5_REPORTS], ext6_path[N_EXT6_REPORTS], ext7_path[N_EXT7_REPORTS], ext8_path[N_EXT8_REPORTS], ext9_path[N_EXT9_REPORTS], ext10_path[N_EXT10_REPORTS], ext11_path[N_EXT11_REPORTS], ext12_path[N_EXT12_REPORTS];
    bool want[N_REPORTS] = {}, run[N_REPORTS] = {};   // want: the caller named a file; run: this call runs a strain step and writes it
    bool pair_want[N_PAIR_REPORTS] = {}, pair_run[N_PAIR_REPORTS] = {};
    bool ext_want[N_EXT_REPORTS] = {}, ext_run[N_EXT_REPORTS] = {};
    bool ext2_want[N_EXT2_REPORTS] = {}, ext2_run[N_EXT2_REPORTS] = {};
    bool ext3_want[N_EXT3_REPORTS] = {}, ext3_run[N_EXT3_REPORTS] = {};
    bool ext4_want[N_EXT4_REPORTS] = {}, ext4_run[N_EXT4_REPORTS] = {};
    bool ext5_want[N_EXT5_REPORTS] = {}, ext5_run[N_EXT5_REPORTS] = {};
    bool ext6_want[N_EXT6_REPORTS] = {}, ext6_run[N_EXT6_REPORTS] = {};
    bool ext7_want[N_EXT7_REPORTS] = {}, ext7_run[N_EXT7_REPORTS] = {};
    bool ext8_want[N_EXT8_REPORTS] = {}, ext8_run[N_EXT8_REPORTS] = {};
    bool ext9_want[N_EXT9_REPORTS] = {}, ext9_run[N_EXT9_REPORTS] = {};
    bool ext10_want[N_EXT10_REPORTS] = {}, ext10_run[N_EXT10_REPORTS] = {};
    bool ext11_want[N_EXT11_REPORTS] = {}, ext11_run[N_EXT11_REPORTS] = {};
    bool ext12_want[N_EXT12_REPORTS] = {}, ext12_run[N_EXT12_REPORTS] = {};
    uint64_t ct_window = 10000;                       // window of the coverage track in bases
    uint32_t nm_top = 5;                              // candidates the near-miss report prints per species
    uint32_t bs_replicates = 100;                     // resamples of the bootstrap report
    uint64_t bs_seed = 42;                            // their seed (the row sampler's)
    uint32_t ai_top = 5;                              // candidates the add-one report tests per species
    uint64_t em_classes = 10;                         // classes the read class report prints per species
    uint32_t em_iterations = 1000;                    // iterations of its estimate at most
    uint64_t sg_min = 1000;                           // bases a chain of the segment report spans at least
    uint64_t sg_bridge = 100;                         // bases between two segments of a chain at most
    uint64_t sg_peak = 10;                            // the factor F of its peak depth; 0: no peak class
    uint64_t mo_top = 10;                             // junctions the mosaic read report prints per species; 0: none, and none are collected
    uint32_t rs_top = 5;                              // candidates the read rescue report prints per species
    uint64_t lk_top = 10;                             // breaks the link support report prints per strain
    uint32_t rf_levels = 5, rf_replicates = 5;        // thinned levels and replicates per level of the rarefaction report
    uint64_t rf_seed = 42;                            // ... and the seed of its thinning rule
    uint64_t gr_window = 5000;                        // window of the replication index report in bases
    uint64_t gr_min_own = 500, gr_trim = 100;         // own bases a window needs, in thousandths of the window; windows trimmed from each end, in thousandths
    bool any_run() const {
        for (const bool r : run) if (r) return true;
        for (const bool r : pair_run) if (r) return true;
        for (const bool r : ext_run) if (r) return true;
        for (const bool r : ext2_run) if (r) return true;
        for (const bool r : ext3_run) if (r) return true;
        for (const bool r : ext4_run) if (r) return true;
        for (const bool r : ext5_run) if (r) return true;
        for (const bool r : ext6_run) if (r) return true;
        for (const bool r : ext7_run) if (r) return true;
        for (const bool r : ext8_run) if (r) return true;
        for (const bool r : ext9_run) if (r) return true;
        for (const bool r : ext10_run) if (r) return true;
        for (const bool r : ext11_run) if (r) return true;
        for (const bool r : ext12_run) if (r) return true;
        return false;
    }
    bool rows_run() const {
        for (int i = 0; i < N_REPORTS; ++i) if (run[i] && REPORTS[i].rows) return true;
        for (int i = 0; i < N_PAIR_REPORTS; ++i) if (pair_run[i] && PAIR_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT_REPORTS; ++i) if (ext_run[i] && EXT_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT2_REPORTS; ++i) if (ext2_run[i] && EXT2_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT3_REPORTS; ++i) if (ext3_run[i] && EXT3_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT4_REPORTS; ++i) if (ext4_run[i] && EXT4_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT5_REPORTS; ++i) if (ext5_run[i] && EXT5_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT6_REPORTS; ++i) if (ext6_run[i] && EXT6_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT7_REPORTS; ++i) if (ext7_run[i] && EXT7_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT8_REPORTS; ++i) if (ext8_run[i] && EXT8_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT9_REPORTS; ++i) if (ext9_run[i] && EXT9_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT10_REPORTS; ++i) if (ext10_run[i] && EXT10_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT11_REPORTS; ++i) if (ext11_run[i] && EXT11_REPORTS[i].rows) return true;
        for (int i = 0; i < N_EXT12_REPORTS; ++i) if (ext12_run[i] && EXT12_REPORTS[i].rows) return true;
        return false;
    }
};
// cfg -> path, want and the two parameters.  A wanted report needs one rank and an unsharded ingest: its rows live on the rank that owns the species, the
// rows of the GAF on the rank of their byte range -- not joined here.  false: the first failing check in table order (REPORTS, then
// PAIR_REPORTS), its message in err (E_INVALID)
bool plan_reports(const pantax_hip_profiling_config *cfg, int W, bool sharded, ReportPlan &plan, std::string &err);
// behind plan_reports, on the same plan: ext -> ext_path and ext_want, then ext2_path and ext2_want (the fields of pantax_hip_profile_ext2 behind it), then ext3_path and ext3_want (pantax_hip_profile_ext3), then ext4_path and ext4_want (pantax_hip_profile_ext4), then ext5_path and ext5_want (pantax_hip_profile_ext5), then ext6_path and ext6_want (pantax_hip_profile_ext6), then ext7_path and ext7_want (pantax_hip_profile_ext7), then ext8_path and ext8_want (pantax_hip_profile_ext8), then ext9_path and ext9_want (pantax_hip_profile_ext9), then ext10_path and ext10_want (pantax_hip_profile_ext10), then ext11_path and ext11_want (pantax_hip_profile_ext11), then ext12_path and ext12_want (pantax_hip_profile_ext12), by the same rule and with the same refusal wording.  ext == null: all off; a field
// that does not lie wholly inside ext->struct_size reads as off (the bootstrap report's replicates: 100, its seed: 42; the add-one report's top: 5; the read class report's classes: 10, its iterations: 1000; the segment report's min: 1000, its bridge: 100, its peak factor: 10; the mosaic read report's top: 10; the read rescue report's top: 5; the link support report's top: 10; the rarefaction report's levels: 5, its replicates: 5, its seed: 42; the replication index report's window: 5000, its min_own: 500, its trim: 100); false also for a struct_size below 8
// or not a multiple of 8, for more than 2^32 - 2 replicates of a wanted bootstrap report, and for more than 16 levels or 2^28 - 1 replicates of a wanted rarefaction report, and for a min_own above 1000 or a trim of 500 or more thousandths of a wanted replication index report
bool plan_ext_reports(const pantax_hip_profile_ext *ext, int W, bool sharded, ReportPlan &plan, std::string &err);
// run[] from want[]: a wanted report is written by a call that runs a strain step
void resume_reports(ReportPlan &plan, bool strain, bool full_path, bool strain_done);

}  // namespace ptx
