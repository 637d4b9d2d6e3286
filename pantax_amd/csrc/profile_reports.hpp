// profile_reports.hpp -- what the per-strain reports (report_plan.hpp) do in the file seam besides being planned: the data they collect group by group
// while a group's coverage result is resident (ReportData, a member of ShardResult) and the three places the seam calls them from.  A new report is a field
// of pantax_hip_profile_ext12 with its row of EXT12_REPORTS (REPORTS, PAIR_REPORTS, EXT_REPORTS, EXT2_REPORTS, EXT3_REPORTS, EXT4_REPORTS, EXT5_REPORTS, EXT6_REPORTS, EXT7_REPORTS, EXT8_REPORTS, EXT9_REPORTS, EXT10_REPORTS and EXT11_REPORTS are closed: the structs they point into keep their size), a sub-struct
// here, and a line in each of begin / collect_group / write (profile_reports.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "report_plan.hpp"

namespace ptx {
struct Run; struct Ingest; struct Selection; struct ShardResult; struct GenomeRow;

// A row of strain_abundance.txt as the row-following reports see it: its sort key, its species (into ShardResult::use), its haplotype (into hap_names), its
// joined genome or null
struct TrackRow { double key; uint32_t k; uint64_t hap; const GenomeRow *gr; };
// Filled group after group.  The haplotypes among the rows of strain_abundance.txt are numbered in the order the groups select them: entry[h] = the number
// of selected haplotypes before h over all groups so far, or -1 ([hap_names]).  Per-entry arrays of every report are indexed by it, per-species arrays by
// the species' position k in ShardResult::use
struct ReportData {
    std::vector<int64_t> entry;
    uint64_t n_entries = 0;
    // --read-strains, file order: global haplotype index (into hap_names) of the assigned strain or ~0, |C(r)| or -1 (not counted), posterior
    struct { std::vector<uint64_t> hap; std::vector<int32_t> n; std::vector<double> post; } rs;
    // --strain-coverage: entry e owns the windows [win_off[e], win_off[e + 1]) of the four arrays
    struct { std::vector<uint64_t> win_off{0}, len, covered, bases; std::vector<uint32_t> n_nodes; } ct;
    // sums over nodes, n u64 a class: hap[2n e ..) = {all, private}; species[2n k ..) = {total, orphan} or species[3n k ..) = {total, orphan, core}
    struct NodeSums { std::vector<uint64_t> hap, species; };
    NodeSums ev;   // --strain-evidence: n = 4 {n_nodes, len, covered, bases}, three species classes
    NodeSums dp;   // --strain-depth: n = 192, a depth histogram of [96]{n_nodes, len}, two species classes
    // --strain-fit: n = 8 {n_nodes, len, bases, expected, excess, deficit, blind_nodes, blind_expected}, three species classes {total, explained, orphan}
    NodeSums ft;
    // --strain-bootstrap: R = replicates + 1 values a quantity, replicate 0 first: x[R e ..) of entry e; obj[R k ..), rows[R k ..), status[R k ..) of species k
    struct { uint64_t R = 0; std::vector<double> x, obj; std::vector<uint64_t> rows; std::vector<int32_t> status; } bs;
    // --strain-dropout: per entry e the refit x, the objective without it, its four counts, the status of its LP, the entry of its substitute (-1: none) with
    // its gain, and the shift; per species k the rows, the objective and the status of the refit and K[k] = its rows of the table
    struct { std::vector<double> refit, obj_without, gain, shift, obj; std::vector<uint64_t> cnt, rows; std::vector<int32_t> st, status; std::vector<int64_t> sub;
             std::vector<uint32_t> K; } dr;
    // --strain-addin: the tested candidates rows[row_off[k] .. row_off[k + 1]) of species k in rank order: the haplotype ([hap_names]), the objective with it,
    // the status of its LP, its coverage, its four counts, the haplotype of its donor (-1: none) with its loss, and the shift; per species k the rows, the
    // objective and the status of entry 0, the rows no reported strain walks and K[k] = its rows of the table
    struct AddinRow { uint64_t hap; double obj_with, coverage, loss, shift; uint64_t cnt[4]; int32_t st; int64_t donor; };
    struct { std::vector<AddinRow> cand; std::vector<uint64_t> row_off, rows, novel; std::vector<double> obj; std::vector<int32_t> status; std::vector<uint32_t> K; } ai;
    // --strain-read-support: hap[9e ..) = {compatible, unique, assigned}; species[12k ..) = {counted, unexplained, ambiguous, uninformative}; a species of
    // K[k] = 1..64 rows owns the K x K block of shared reads pair[pair_off[k] ..) over its entries in ascending order
    struct { std::vector<uint64_t> hap, species, pair, pair_off; std::vector<uint32_t> K; } sup;
    // --strain-em: per entry e its G and its x; per species k {counted, unexplained} in species[6k ..), its classes cls[cls_off[k] .. cls_off[k + 1]) in ascending
    // mask (bit i = the species' i-th entry), the iterations, converged and delta of its estimate and K[k] = its rows of the table
    struct EmClass { uint64_t mask, q[3]; };
    struct { std::vector<uint64_t> len, species, cls_off; std::vector<double> x, delta; std::vector<EmClass> cls; std::vector<uint32_t> K, iter; std::vector<int32_t> conv; } em;
    // --strain-segments: per entry e its peak_depth, G_h and the run totals {gap, peak} at [2e ..); its kept segments [seg_off[e], seg_off[e + 1]) in ascending start
    struct { std::vector<uint64_t> peak, hap_len, n_runs, run_len, run_max, seg_off{0}, step, start, len, bases; std::vector<uint32_t> n_steps; std::vector<uint8_t> cls; } sg;
    // --strain-mosaic: species[18k ..) = the six classes of Q, extra[3k ..) = {n_segments, n_breaks, foreign_steps}, hap[2e ..) = {segments, steps}; K[k] = the
    // species' rows of the table and its K x K switch counts from pair[pair_off[k]] on; its distinct junctions [jn_off[k], jn_off[k + 1]) as species-local
    // {node_a, node_b} with their counts, in ascending (node_a, node_b)
    struct { std::vector<uint64_t> species, extra, hap, pair, pair_off, jn_off, jn_count; std::vector<uint32_t> K, jn_a, jn_b; } mo;
    // --strain-rescue: species[27k ..) = the nine classes of Q, step[3k ..) = {foreign_steps, claimed_steps, novel_steps}, open[k] = the species went through
    // the call with K_s + J_s <= 64; the printed candidates rows[row_off[k] .. row_off[k + 1]) in rank order: the haplotype ([hap_names]), q = {rescued,
    // alone, from_foreign} x Q and its steps
    struct RescueRow { uint64_t hap; uint64_t q[9]; uint64_t steps; };
    struct { std::vector<uint64_t> species, step, row_off; std::vector<uint8_t> open; std::vector<RescueRow> rows; } rc;
    // --strain-links: species[6k ..) and link[4k ..) as pantax_hip_strain_links writes them, open[k] = the species went through the call with K_s <= 64;
    // per entry e its eight counters hap[8e ..) and its break records [brk_off[e], brk_off[e + 1]) in ascending step (node_a / node_b species-local)
    struct { std::vector<uint64_t> species, link, hap, brk_off{0}, start, flank, mask; std::vector<uint32_t> node_a, node_b; std::vector<uint8_t> open; } lk;
    // --strain-rarefy: E = 1 + replicates x levels entries (entry 0 the full sample, 1 + (b - 1) levels + (l - 1) level l of replicate b); per selection
    // entry e its E values x[E e ..) and member[2 E e ..) = {n_member, n_only}; per species k obj / rows / status [E k ..) and reads[2 E k ..) = {counted
    // reads, bases added}
    struct { uint64_t E = 1; std::vector<double> x, obj; std::vector<uint64_t> rows, reads, member; std::vector<int32_t> status; } rf;
    // --strain-fragments: mate [R] in file order, formed once per run before the first group (have_mate); hap[12e ..) = {compatible, unique, unique_by_pair,
    // assigned}, species[27k ..) = the nine classes and status[k] as pantax_hip_strain_fragments writes them; a species of K[k] = 1..64 rows owns the K x K
    // block of discordant fragments pair[pair_off[k] ..) over its entries in ascending order
    struct { bool have_mate = false; std::vector<uint32_t> mate, K; std::vector<uint64_t> hap, species, pair, pair_off; std::vector<int32_t> status; } fr;
    // --strain-growth: entry e owns the windows [win_off[e], win_off[e + 1]) of the three arrays (len: every step, for G_h; len_own and bases_own: own steps)
    struct { std::vector<uint64_t> win_off{0}, len, len_own, bases_own; } gr;
    // --strain-near-miss: species[12k ..) = {orphan, claimed, contested}; the printed candidates rows[row_off[k] .. row_off[k + 1]) in rank order: the
    // haplotype ([hap_names]) and q = {novel, exclusive, all} x {n_nodes, len, covered, bases}
    struct NearMissRow { uint64_t hap; uint64_t q[12]; };
    struct { std::vector<uint64_t> species, row_off; std::vector<NearMissRow> rows; } nm;
    // --strain-pair-evidence: a species of K[k] = 2..256 rows owns the K x K block of {n_nodes, len, covered, bases} from entry pair_off[k] of pair (four u64
    // an entry) over its entries in ascending order; K[k] is the species' number of rows whether or not it has a block
    struct { std::vector<uint64_t> pair, pair_off; std::vector<uint32_t> K; } pe;
};

namespace reports {
// sizes what the running reports index by read (R), haplotype (H) and species (Su) of the shard
void begin(const ReportPlan &plan, uint32_t Su, uint64_t H, uint64_t R, ReportData &rep);
// the species [k0, k1) of the db that has just gone through its strain step: the group's rows of the strain table selected once, then each running report
int collect_group(Run &run, const Ingest &in, const Selection &sn, pantax_hip_db *db, uint32_t k0, uint32_t k1, ShardResult &sh);
// behind the tables: the files of the running reports; `rows` come from strain_tables and are put into the table's order here
int write(Run &run, const Ingest &in, const Selection &sn, const ShardResult &sh, const std::vector<GenomeRow> &genomes, std::vector<TrackRow> &rows);
}  // namespace reports
}  // namespace ptx
