// lad_args.hpp -- what a solver workgroup of stage_lad.hip is handed: the sorted rows, the pattern tables, the per-pattern scratch and the outputs as plain
// device arrays.  Everyone fills it through lad_plain_args below: the strain step from its LadBatch (lad_args, stage_lad.hip, which adds the tables of
// the wide species); pantax_hip_strain_bootstrap and pantax_hip_strain_dropout from the tables of their replicates / rounds, launching through
// lad_args_launch.
#pragma once
#include <cstdint>
#include "common.hpp"

namespace ptx {

struct LadArgs {
    unsigned long long *prof;   // LAD_PROFILE builds only (null otherwise)
    const double *row_a;
    const uint64_t *pat_mask;
    const uint32_t *pat_start;
    const uint32_t *sp_pat_off;
    double *pat_eps, *sc_s, *sc_rho;
    uint32_t *sc_lo, *sc_up, *ls_lo, *ls_hi, *ls_mid;
    const int32_t *sp_p;
    const uint8_t *need;    // [S] or null: solve only species with need[s] != 0
    const uint8_t *fixed;   // [H] at col_off[s] + k, or null: variables pinned to zero
    const double *amax;
    double *x_out;          // [H] at col_off[s] + k
    int32_t *status, *iters;
    const uint64_t *col_off;   // [S+1] first column slot of every species (= its first haplotype)
    // wide species (more than LAD_MAXP columns): the mask words of pattern k of species s are
    // pat_or[(wide_off[s] + k - sp_pat_off[s]) * NW ..]; W / G live in global scratch, slot wide_slot[s]
    const uint32_t *wide_list, *wide_off, *wide_slot;
    const uint64_t *pat_or, *pat_and;
    double *wide_W, *wide_G;
    // wide_off counts groups of LAD_WIDE_NW words; a species of more than LAD_WIDEP haplotypes ("huge") has wide_nw[s] > LAD_WIDE_NW
    // words per node and per pattern.  W of wide slot i starts at wide_woff[i] (G at twice that), rows of 64 * wide_nw doubles;
    // the column state of a huge species (x, c, d, ub, ... of lad_solve_body) at wide_coff[i] columns into huge_f64 (x 8) / huge_i32 (x 5);
    // pat_act[k] = the basis slot that holds pattern k, or -1 (huge species only)
    const uint32_t *wide_nw;
    const uint64_t *wide_woff, *wide_coff;
    double *huge_f64;
    int *huge_i32, *pat_act;
};

// LadPatScratch (common.hpp): the eight per-pattern arrays, allocated in the order the solver's users always have
inline int LadPatScratch::alloc(Ctx *ctx, uint64_t n_patterns) {
    PTX_HIP(ctx, pat_eps.alloc(n_patterns)); PTX_HIP(ctx, sc_s.alloc(n_patterns)); PTX_HIP(ctx, sc_rho.alloc(n_patterns));
    PTX_HIP(ctx, sc_lo.alloc(n_patterns)); PTX_HIP(ctx, sc_up.alloc(n_patterns)); PTX_HIP(ctx, ls_lo.alloc(n_patterns));
    PTX_HIP(ctx, ls_hi.alloc(n_patterns)); PTX_HIP(ctx, ls_mid.alloc(n_patterns));
    return 0;
}
inline void LadPatScratch::bind(LadArgs &A) const {
    A.pat_eps = pat_eps.p; A.sc_s = sc_s.p; A.sc_rho = sc_rho.p;
    A.sc_lo = sc_lo.p; A.sc_up = sc_up.p; A.ls_lo = ls_lo.p; A.ls_hi = ls_hi.p; A.ls_mid = ls_mid.p;
}

// The plain-array part of a LadArgs from named arguments; the wide fields stay null (no entry may then have more than LAD_MAXP columns).
struct LadRowTables { const double *row_a; const uint64_t *pat_mask; const uint32_t *pat_start, *sp_pat_off; };            // sorted rows, pattern tables
struct LadLpTables { const int32_t *sp_p; const double *amax; const uint64_t *col_off; const uint8_t *need, *fixed; };     // per LP (need, fixed: or null)
struct LadOutputs { double *x; int32_t *status, *iters; };
inline LadArgs lad_plain_args(const LadRowTables &rows, const LadLpTables &lps, const LadOutputs &out, const LadPatScratch &scratch) {
    LadArgs A = {};
    A.row_a = rows.row_a; A.pat_mask = rows.pat_mask; A.pat_start = rows.pat_start; A.sp_pat_off = rows.sp_pat_off;
    A.sp_p = lps.sp_p; A.amax = lps.amax; A.col_off = lps.col_off; A.need = lps.need; A.fixed = lps.fixed;
    A.x_out = out.x; A.status = out.status; A.iters = out.iters;
    scratch.bind(A);
    return A;
}

// stage_lad.hip: lad_solve_kernel<16, 1> (pmax_bound <= 16) or <LAD_MAXP, 1> over the entries [0, n_lps) of A.sp_p, on ctx->stream; an entry with
// sp_p <= 0 gets status 0 and nothing else.  The wide fields of A are not read (no entry has more than LAD_MAXP columns): null is fine.
int lad_args_launch(Ctx *ctx, const LadArgs &A, uint32_t n_lps, int pmax_bound, const char *timer_name);

}  // namespace ptx
