// profile_run.hpp -- internal to the file seam (api_profile.cpp, profile_shard.cpp, profile_pure.cpp): the state of one pantax_hip_profile call
// as plain structs, cut along what each phase reads and writes; the helpers that decide without a ctx, a HIP call or file I/O.
#pragma once
#include <sys/stat.h>
#include <string>
#include <vector>
#include "common.hpp"
#include "host_io.hpp"
#include "profile_comm.hpp"
#include "profile_pure.hpp"

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
    bool want_report = false, want_rs = false, rs_run = false;          // rs_run: this call runs a strain step and writes the --read-strains report
    bool want_ct = false, ct_run = false;                               // ct_run: ... and writes the --strain-coverage track
    uint64_t ct_window = 0;                                             // its window W in bases
    bool want_ev = false, ev_run = false;                               // ev_run: ... and writes the --strain-evidence report
    bool want_sup = false, sup_run = false;                             // sup_run: ... and writes the --strain-read-support report
    bool want_dp = false, dp_run = false;                               // dp_run: ... and writes the --strain-depth report
    bool want_nm = false, nm_run = false;                               // nm_run: ... and writes the --strain-near-miss report
    uint32_t nm_top = 5;                                                // candidates it prints per species
    std::string db_dir, wd, out_dir, zip, species_file, strain_file, report, rs_path, ct_path, ev_path, sup_path, dp_path, nm_path, gaf_path;
};
// what every phase is handed: the two handles, the plan, the ranks, the trace clock
struct Run { pantax_hip_ctx *ctx; const pantax_hip_profiling_config *cfg; RunPlan p; RankComm comm; Lap lap; };
// a1 - a3: depends on the sample (and the ranges of the DB)
struct Ingest {
    std::vector<RangeRow> ranges; uint32_t S = 0;
    MappedFile mf; HostReads hr;
    ReadsHolder reads;                 // resident reads: this rank's byte range; behind the routing, the reads of its species
    DbHolder bin_db;                   // ranges-only db of ALL species
    uint64_t R = 0, text_begin = 0;
    std::vector<int32_t> sp_idx;       // species of every read (file order), with the host columns of hr: fetched once, on request (host_cols)
    bool have_cols = false, reads_grouped = false;   // reads_grouped: the locus-grouped copy of the resident reads exists (built once, beside the first graph load)
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
    // --read-strains, file order: global haplotype index (into hap_names) of the assigned strain or ~0, |C(r)| or -1 (not counted), posterior
    std::vector<uint64_t> rs_hap;
    std::vector<int32_t> rs_n;
    std::vector<double> rs_post;
    // --strain-coverage: the windows of every haplotype among the rows of strain_abundance.txt, group after group.  ct_entry[h] = its entry or -1 ([hap_names]);
    // entry e owns the windows [ct_win_off[e], ct_win_off[e + 1]) of the four arrays
    std::vector<int64_t> ct_entry;
    std::vector<uint64_t> ct_win_off{0}, ct_len, ct_covered, ct_bases;
    std::vector<uint32_t> ct_n_nodes;
    // --strain-evidence: the sums of every haplotype among the rows of strain_abundance.txt, group after group, and of every species of the shard.
    // ev_entry[h] = its entry or -1 ([hap_names]); entry e owns ev_hap[8e .. 8e + 8) = {all, private}; species k owns ev_species[12k .. 12k + 12) = {total, orphan, core}
    std::vector<int64_t> ev_entry;
    std::vector<uint64_t> ev_hap, ev_species;
    // --strain-read-support: the same for the read support.  sup_entry[h] = its entry or -1; entry e owns sup_hap[9e .. 9e + 9) = {compatible, unique, assigned};
    // species k owns sup_species[12k .. 12k + 12) = {counted, unexplained, ambiguous, uninformative} and, when it has 1..64 rows, the K x K block of shared
    // reads sup_pair[sup_pair_off[k] ..) over its entries in ascending order (K = sup_K[k])
    std::vector<int64_t> sup_entry;
    std::vector<uint64_t> sup_hap, sup_species, sup_pair, sup_pair_off;
    std::vector<uint32_t> sup_K;
    // --strain-depth: the depth histograms ([96]{n_nodes, len} = 192 u64 each) of every haplotype among the rows of strain_abundance.txt, group after group,
    // and of every species of the shard.  dp_entry[h] = its entry or -1 ([hap_names]); entry e owns dp_hap[384e .. 384e + 384) = {all, private}; species k
    // owns dp_species[384k .. 384k + 384) = {total, orphan}
    std::vector<int64_t> dp_entry;
    std::vector<uint64_t> dp_hap, dp_species;
    // --strain-near-miss: species k owns nm_species[12k .. 12k + 12) = {orphan, claimed, contested} and the printed candidates nm_rows[nm_row_off[k] ..
    // nm_row_off[k + 1]) in rank order: the haplotype ([hap_names]) and q = {novel, exclusive, all} x {n_nodes, len, covered, bases}
    struct NearMissRow { uint64_t hap; uint64_t q[12]; };
    std::vector<uint64_t> nm_species, nm_row_off;
    std::vector<NearMissRow> nm_rows;
    bool image_fault = false;          // rc is the load-time refusal of a group that holds images ...
    std::string fault_images;          // ... these (the check names a haplotype, not a file), for the warning
};
// profile_shard.cpp: everything a rank does on its own shard (sources, groups, loader, device sequence, read strains, coverage track, node evidence, read support, depth distribution, near misses, image write-back)
ShardResult run_shard(Run &run, Ingest &in, const Selection &sn, bool use_images);
}  // namespace ptx
