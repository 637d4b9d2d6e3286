// profile_pure.hpp -- the decisions of the file seam on plain values: no ctx, no HIP call, no file (profile_pure.cpp)
#pragma once
#include <set>
#include "common.hpp"    // for its types alone
#include "host_io.hpp"   // RangeRow, GenomeRow, fmt_f64

namespace ptx {
bool species_wanted(int mode, const std::set<std::string> &designated, const RangeRow &row);   // mode 0 keeps is_pan == 0, mode 1 is_pan == 1; a non-empty designated set keeps its members only (profile.rs:583-594)
std::vector<int> lpt_owner(const std::vector<double> &weight, int W);   // longest-processing-time packing: heaviest first onto the least loaded rank
std::vector<std::pair<uint32_t, uint32_t>> cut_groups(const std::vector<uint64_t> &steps, const std::vector<uint64_t> &nodes, uint64_t steps_max, int db_groups);   // contiguous groups [k0, k1) of species for one resident db each
bool mixed_ids(const std::vector<uint64_t> &hash, const std::vector<uint64_t> &value, std::vector<uint64_t> &mixed);   // records sorted by hash, value = complete << 32 | species: the hashes whose complete records span species -> mixed; returns "some hash repeats"
std::string strain_row_text(const std::string &species, const GenomeRow *gr, const pantax_hip_hap_metrics &m, double abund, bool has_abund, bool rnd);   // one row of (ori_)strain_abundance.txt
const char *near_miss_stage(const pantax_hip_hap_metrics &m);   // where an unreported haplotype left the path: first_filter / second_filter / table_filter
// one row of the --strain-near-miss report.  m = the candidate's metrics, or null for a species row (strain, rank, stage and metric columns "-"; gr is not
// looked at); q = {n_nodes, len, covered, bases}; share = q.bases / orphan_bases where with_share and orphan_bases > 0, else "-"
std::string near_miss_row_text(const std::string &species, const GenomeRow *gr, const pantax_hip_hap_metrics *m, uint32_t rank, const char *cls, const uint64_t *q,
                               bool with_share, uint64_t orphan_bases);
// class of a pair of haplotypes from the bases only one of them walks: identical, nested or distinct (the --db-pairs table and the pair evidence report)
const char *hap_pair_class(uint64_t only_a_len, uint64_t only_b_len);
}  // namespace ptx
