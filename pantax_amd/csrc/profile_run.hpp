// profile_run.hpp -- internal to the file seam (api_profile.cpp, profile_shard.cpp, profile_reports.cpp, profile_pure.cpp): the state of one
// pantax_hip_profile call as plain structs, cut along what each phase reads and writes (the per-strain reports: one member each, report_plan.hpp and
// profile_reports.hpp); the helpers that decide without a ctx, a HIP call or file I/O.
#pragma once
#include <sys/stat.h>
#include <string>
#include <vector>
#include "common.hpp"
#include "host_io.hpp"
#include "profile_comm.hpp"
#include "profile_pure.hpp"
#include "profile_reports.hpp"

namespace ptx {
inline bool is_file(const std::string &p) { struct stat st; return !p.empty() && stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }
// modification time in ns, 0 if the file is missing
inline int64_t file_mtime(const std::string &p) { struct stat st; return (!p.empty() && stat(p.c_str(), &st) == 0) ? (int64_t)st.st_mtim.tv_sec * 1000000000ll + st.st_mtim.tv_nsec : 0; }
inline std::string path_join(const std::string &a, const std::string &b) { return a.empty() ? b : (a.back() == '/' ? a + b : a + "/" + b); }
struct DbHolder { pantax_hip_ctx *ctx; pantax_hip_db *db = nullptr; ~DbHolder() { if (db) pantax_hip_db_free(ctx, db); } };
struct ReadsHolder { pantax_hip_ctx *ctx; pantax_hip_reads *rd = nullptr; ~ReadsHolder() { if (rd) pantax_hip_reads_free(ctx, rd); } };
// everything decided from cfg and the work directory before the first device call
struct RunPlan {
    bool sharded = false;                                               // the ingest is sharded too (an alltoallv callback); W, rk, use_comm: RankComm
    bool full_path = false, strain_only = false, strain_done = false;   // rank 0's look at the work directory, followed by every rank
    bool want_report = false;                                           // a full run that writes the binning report
    ReportPlan rep;                                                     // the per-strain reports: wanted, run by this call, their two parameters (report_plan.hpp)
    std::string db_dir, wd, out_dir, zip, species_file, strain_file, report, gaf_path;
};
// what every phase is handed: the two handles, the sized extension of cfg (or null), the plan, the ranks, the trace clock
struct Run { pantax_hip_ctx *ctx; const pantax_hip_profiling_config *cfg; const pantax_hip_profile_ext *ext; RunPlan p; RankComm comm; Lap lap; };
// a1 - a3: depends on the sample (and the ranges of the DB)
struct Ingest {
    std::vector<RangeRow> ranges; uint32_t S = 0;
    MappedFile mf; HostReads hr;
    ReadsHolder reads;                 // resident reads: this rank's byte range; behind the routing, the reads of its species
    DbHolder bin_db;                   // ranges-only db of ALL species
    uint64_t R = 0, text_begin = 0;
    std::vector<int32_t> sp_idx;       // species of every read (file order), with the host columns of hr: fetched once, on request (host_cols)
    bool have_cols = false;
    std::vector<int64_t> rc, bs, lm, uq, rs, re;   // the four counters per species (merged over the ranks when sharded); range starts / ends
    std::vector<uint32_t> head;        // read lengths of the first (up to 1000) binned rows of the file
    uint64_t read_base = 0, R_all = 0; // this rank's first read in file order; reads of the whole file
    explicit Ingest(pantax_hip_ctx *c) : reads{c}, bin_db{c} {}
};
struct SpeciesProfileRow { std::string species; double abundance, coverage; };
// a4 / a5 and the species -> rank table
struct Selection {
    std::vector<uint32_t> sel;         // indices into `ranges`, in species-profile order
    std::vector<double> sel_cov;
    std::vector<int> owner;            // rank of every selected species
    std::vector<uint8_t> flags;        // drop flags of every read (null field, duplicate id); empty when no host column was fetched
    bool flags_dirty = false;          // ... differ from what the tokenizer left on the device
};
// one pass over this rank's species: nothing in here survives a second pass
struct ShardResult {
    int rc = 0;
    std::vector<uint32_t> use;         // this rank's selected species with a loaded graph (indices into sel)
    std::vector<uint64_t> hap_off{0}; std::vector<std::string> hap_names;
    std::vector<pantax_hip_hap_metrics> met; std::vector<pantax_hip_solve_info> info;
    ReportData rep;                    // what the running per-strain reports collected, group after group (profile_reports.hpp)
    bool image_fault = false;          // rc is the load-time refusal of a group that holds images ...
    std::string fault_images;          // ... these (the check names a haplotype, not a file), for the warning
};
// profile_shard.cpp: everything a rank does on its own shard (sources, groups, loader, device sequence, the per-strain reports' turn, image write-back)
ShardResult run_shard(Run &run, Ingest &in, const Selection &sn, bool use_images);
}  // namespace ptx
