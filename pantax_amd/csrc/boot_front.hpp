// boot_front.hpp -- the front half that pantax_hip_strain_bootstrap (stage_bootstrap.hip) and pantax_hip_strain_dropout (stage_dropout.hip) share: the host
// tables of the selection, the rows of the call compacted by one chained scan (scan_chained_kernel<BootRows>), the radix sort over (species, mask, a) and the
// base pattern tables (scan_chained_kernel<BootPat>, boot_sp_pat_off_kernel).  Defined in stage_bootstrap.hip; the same kernels in the same order for both
// callers, so a row sits where it sat before the two stages shared it.
#pragma once
#include <functional>
#include <string>
#include <vector>
#include "common.hpp"
#include "member_device.hpp"

namespace ptx {

constexpr int32_t BOOT_PENDING = 0x7FFFFFFF;   // pre-status of an entry the solver decides

struct BootSpecies { MemberRow m; uint64_t hash; };   // hash: boot_species_hash(seed, sp_key[s]) (0 where the caller draws no weights)

struct BootFront {
    // host
    std::vector<int32_t> pre_host;   // [S] per species: PANTAX_HIP_E_LIMIT (more than 64 columns), 1 (nothing selected) or BOOT_PENDING
    uint64_t k_max = 0;              // most columns of a served species
    uint64_t N = 0;                  // rows of the call; 0: nothing to solve (no node, nothing selected or no row) and nothing below is set
    uint32_t P = 0;                  // base patterns: runs of equal (species, mask) in the sorted rows
    // device: the sorted rows ...
    const uint64_t *row_sp = nullptr, *row_mask = nullptr;   // [N]
    const double *base_a = nullptr;                           // [N]
    const uint32_t *vloc = nullptr;                           // [N] node of the row, counted from the species' first
    // ... and what holds them
    WalkMasks wm;
    DevBuf<BootSpecies> d_tab;
    DevBuf<uint8_t> d_bit_col;
    DevBuf<uint32_t> d_node_off, d_counts /*[4]: rows, patterns, two free words*/, d_va, d_vb, d_table, d_scan_tmp;
    DevBuf<uint64_t> d_sel_off, ka[3], kb[3];
    DevBuf<uint64_t> d_bpat_mask;                                   // [P]
    DevBuf<uint32_t> d_bpat_start /*[P + 1], the last = N*/, d_bpat_species /*[P]*/, d_bsp_pat_off /*[S + 1]*/;
};

// d_bases [V]: the per-node bases the row source reads -- the db's own (Db::d_bases) for the bootstrap, the leave-one-out and the add-one test, a thinned
// level's for the rarefaction.  sp_key null: no weight hash (seed unread).  route_opt: the caller's membership route option.  `sized` is called once with N > 0, behind the row scan and
// ahead of everything that is sized by N: the caller's plan; a non-zero return ends the call with it.  `what` heads the messages.
int boot_front_build(Ctx *ctx, Db *db, const unsigned long long *d_bases, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *sp_key, uint64_t seed,
                     const std::string &route_opt, const char *what, const std::function<int(uint64_t)> &sized, BootFront &F);

// bootstrap_launch (common.hpp) on the per-node bases array d_bases [V] instead of the db's own, under the membership route option route_opt, `what` heading
// the messages.  front_built (may be null) is called once with the front half when it holds rows (F.N > 0), ahead of the replicates: a caller's own pass
// over the base patterns.  Outputs as bootstrap_launch's, written only on success.
int bootstrap_launch_on(Ctx *ctx, Db *db, const unsigned long long *d_bases, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *sp_key, uint64_t seed,
                        uint32_t n_replicates, const std::string &route_opt, const char *what, const std::function<int(const BootFront &)> *front_built, double *x_out,
                        double *obj_out, uint64_t *rows_out, int32_t *status_out);

// boot_objective_kernel over the entries [0, nq) of plain solver tables (lad_args.hpp): obj[q] = the sum over the entry's rows of |m . x - a|, a workgroup per
// entry, a wave per pattern; part [patterns] is scratch.  The bootstrap's objective pass, and the yardstick the leave-one-out pass is measured against.
int boot_objective_launch(Ctx *ctx, uint32_t nq, const int32_t *sp_p, const uint32_t *sp_pat_off, const uint64_t *pat_mask, const uint32_t *pat_start, const double *row_a,
                          const uint64_t *col_off, const double *x, double *part, double *obj, const char *timer_name);

}  // namespace ptx
