// lad_args.hpp -- what a solver workgroup of stage_lad.hip is handed: the sorted rows, the pattern tables, the per-pattern scratch and the outputs as plain
// device arrays.  The strain step fills it from its LadBatch (lad_args, stage_lad.hip); pantax_hip_strain_bootstrap fills it from the tables of its
// replicates and launches through lad_args_launch.
#pragma once
#include <cstdint>

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

struct Ctx;
// stage_lad.hip: lad_solve_kernel<16, 1> (pmax_bound <= 16) or <LAD_MAXP, 1> over the entries [0, n_lps) of A.sp_p, on ctx->stream; an entry with
// sp_p <= 0 gets status 0 and nothing else.  The wide fields of A are not read (no entry has more than LAD_MAXP columns): null is fine.
int lad_args_launch(Ctx *ctx, const LadArgs &A, uint32_t n_lps, int pmax_bound, const char *timer_name);

}  // namespace ptx
