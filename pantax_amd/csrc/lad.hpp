// lad.hpp -- device-side pieces of the strain step (a9 - a13), one source file per stage: per-hap trio statistics and the first filter
// (stage_hap_stats.hip), node statistics and a11 (stage_node_stats.hip), candidate-path masks + path_cov_ratio and the LP rows
// (stage_lp_rows.hip), the batched exact LAD solver with the second filter (stage_lad.hip), the objectives (stage_objective.hip).
#pragma once
#include "common.hpp"

namespace ptx {

// a9: per-hap unique-trio statistics (zscore_filter profile.rs:1028-1051; :1114-1147)
int hap_trio_stats_launch(Ctx *ctx, Db *db, DevBuf<uint32_t> &d_ntrio_nz /*[H]*/, DevBuf<double> &d_mean /*[H]*/,
                          const uint8_t *d_active /* device [S] or null: species the coverage pass skipped are not read */,
                          bool readers_clean /* the pass zeroes the trio_bases it reads (cov_clean_plan, cov_state.hpp) */);
// node abundance + per-species stats
int node_stats_launch(Ctx *ctx, Db *db, LadBatch *lb, int64_t min_depth, const uint8_t *d_active, bool readers_clean /* ... bases, bit vector, full-node flags */);
// Which route the LP rows take: a pure function of the options and of the db's host-side tables (h_node_off, h_hap_off, the node -> haplotype state).
// node_pass_fused_eligible (before the step's first kernel) and lad_prepare (later) both decide from it.
struct RowRoute {
    uint64_t max_vs;       // nodes of the largest species
    uint32_t max_haps;     // haplotypes of the largest species
    bool wide;             // some species has more than LAD_MAXP haplotypes
    bool by_node;          // masks from the node -> haplotype words (mask_nodes_kernel), not from the path walk
    bool use_nodes;        // the rows are sorted straight from the node arrays (sample_sort_nodes), no compaction
    bool use_sample;       // the compacted rows fit the whole-batch sample sort (otherwise: radix)
    bool ratio_by_node;    // the path_cov_ratio sums ride on the by-node mask pass
    bool masks_in_sort;    // the masks are formed inside the node sort: no mask array, no pass of its own
};
RowRoute row_route(const Ctx *ctx, const Db *db);
int row_pack_shift(const RowRoute &rt, uint32_t S, int pmax_bound);   // >= 0: two-word rows {species << shift | mask, a}; -1: three words
// the resident step's fused node pass (node_rows_kernel in place of node_cov_stats_kernel + ssn_hist_kernel<true>): can THIS step take it?  Host-known only.
bool node_pass_fused_eligible(const Ctx *ctx, const Db *db, const pantax_hip_strain_config *cfg, bool readers_clean);
// Which LDS shape the <= 16-column LAD solver launches with (stage_lad.hip: LadRoomy / LadCompact): a pure function of the option lad_shape ("" / "auto",
// "roomy", "compact"), the number of solver workgroups of the launch (one per species), the device's CU count and the launch's column bound.
//   auto: compact when the batch has more workgroups than the device has CUs -- they would queue for a CU one at a time under the roomy shape, while four
//   compact ones share it; roomy otherwise (a single or a few large LPs: residency buys nothing, the finer row index does).  More than 16 columns: always
//   roomy (the 17..64-column and the wide instances have one shape).  The results are the same bits under either shape.
enum class LadShape { roomy, compact };
LadShape lad_shape(const std::string &option, uint32_t n_workgroups, int n_cu, int pmax_bound);
const char *lad_shape_name(LadShape s);
// a11: species with more valid rows than sample_nodes keep the rows rand 0.9.2's choose_multiple(seed 42) would keep
int row_sample_apply(Ctx *ctx, const Db *db, LadBatch *lb, int64_t sample_nodes);
// a10: masks, ratios; then LP rows sorted and grouped into patterns.  What the caller has decided goes in as LadRequest, what the solver and the objective
// have to know about the rows comes back as LadRows -- nothing of either is kept in the LadBatch.
struct FusedNodePass { double min_depth; const uint8_t *active; };   // active: the species flags the coverage pass skipped by (device [S] or null)
struct LadRequest {
    bool cand_on_device;         // lb->d_hap_bit / d_p were written by first_filter_kernel; else they are uploaded from lb->h_p / h_cand (solver seam)
    int pmax_bound;              // upper bound of the candidates per species
    bool zeroed;                 // the result arena and d_mask were zeroed ahead of the step (strain_prezero)
    const FusedNodePass *fused;  // the row sort also forms abundances, covered bases and node statistics (node_rows_kernel): d_ab and the db's d_cov hold nothing.
                                 // strain_enqueue decides (node_pass_fused_eligible); null: the two-kernel path has run
};
struct LadRows {
    bool c0_valid;       // lb->d_c0 (the objective's part without rows) is there for the rows just sorted
    bool masks_in_sort;  // the masks were formed inside the row sort: lb->d_mask holds nothing
    bool fused;          // ... and so were the abundances: lb->d_ab holds nothing
};
int lad_prepare(Ctx *ctx, Db *db, LadBatch *lb, const LadRequest &rq, LadRows *rows);
// a12: one workgroup per species (those with d_p[s] > 0 and need[s], when given); variables with fixed[s*64+k]
// are pinned to 0.  Writes x, obj, status, iters for the solved species.  Nothing is read back.
int lad_solve_launch(Ctx *ctx, const Db *db, LadBatch *lb, const LadRows &rows, int pmax_bound, const uint8_t *d_need, const uint8_t *d_fixed, double *d_x,
                     double *d_obj, int32_t *d_status, int32_t *d_iters);
// the strain step's LP1 -> second filter -> LP2 (+ both objectives) as two launches
struct FilterCfg;
int lad_pair_launch(Ctx *ctx, const Db *db, LadBatch *lb, const LadRows &rows, int pmax_bound, const FilterCfg &fc);
// both objectives of the solved species (x2 / need2 null: one solution), from the sorted rows or from the nodes
int objective_launch(Ctx *ctx, const Db *db, LadBatch *lb, const LadRows &rows, const uint8_t *d_need2, const double *d_x1, const double *d_x2, double *d_obj1,
                     double *d_obj2);
// a9 / a13 decisions on the device (the host redoes only the reporting arithmetic at the end of the step)
struct FilterCfg { double fr, fc, sr; int shift; };
int first_filter_launch(Ctx *ctx, const Db *db, LadBatch *lb, const uint8_t *d_active, const FilterCfg &fc);

// the strain step in two halves (api_strain.cpp): everything enqueued / the one wait + host reporting
int strain_prezero(Ctx *ctx, Db *db, bool *zeroed);   // optional, ahead of strain_enqueue: its two zero-fills, issued where the stream has slack; the caller hands *zeroed on
// slot: which pinned result buffer / event (0 or 1); zeroed: strain_prezero has run in this call, behind everything that wrote the arena and the masks
int strain_enqueue(Ctx *ctx, Db *db, const pantax_hip_strain_config *cfg, const uint8_t *d_active, int slot, bool zeroed = false);
int strain_finish(Ctx *ctx, Db *db, const pantax_hip_strain_config *cfg, const uint8_t *species_active, const double *species_coverage,
                  pantax_hip_hap_metrics *met, pantax_hip_solve_info *info_out, void (*after_wait)(void *), void *after_wait_arg, int slot);

}  // namespace ptx
