// stage_lad.hip -- a12 on device: the batched exact LAD solver that replaces the Gurobi/HiGHS/CBC/GLPK
// backends (profile.rs:1297-1511, 2689-2882), with the second filter (a13) between its two solves.
//
// The reference LP per species (gurobi_opt, profile.rs:1312-1460):
//     min (1/n) sum_{v: a_v>0} y_v,   y_v >= +-(sum_k A_vk x_k - a_v),   0 <= x_k <= 1.05*max(a)
// with A_vk = 1 iff node v lies on candidate path k (:1333-1342); the binary indicators are inert
// (SURVEY.md 8c).  That is a least-absolute-deviation fit in p <= 64 variables.  Rows with the
// same membership pattern m (a p-bit mask) only see s_m = sum_{k in m} x_k, so after ONE
// HBM-bound pass that sorts the n covered nodes by (species, mask, a) the objective is
//     f(x) = (1/n) sum_patterns F_m(s_m),  F_m(s) = sum_{rows of m} |s - a|,
// and f, its sub-gradient and exact line searches cost O(#patterns * log n) binary searches.
// The solver is an exact active-set (Bloomfield-Steiger / Barrodale-Roberts) descent on that
// representation, one workgroup per species, all species of the batch in one launch.
#include <algorithm>
#include <cstdio>
#include <vector>
#include "lad.hpp"
#include "lad_solver.hpp"
#include "second_filter.hpp"
#include "primitives.hpp"

namespace ptx {

// NW == 1: one workgroup per species of the db, species with more than LAD_MAXP columns are left to the wide launches;
// NW == LAD_WIDE_NW / 0: one workgroup per entry of wide_list; the instance takes the species with more than LAD_MAXP columns
// whose mask has LAD_WIDE_NW words / more words ("huge": more than LAD_WIDEP haplotypes).
template <int NW>
__device__ __forceinline__ bool lad_instance_takes(const LadArgs &A, int s, int p) {
    if (NW == 1) return p <= LAD_MAXP;
    if (p <= LAD_MAXP) return false;
    return (NW == 0) == (A.wide_nw[s] > (uint32_t)LAD_WIDE_NW);
}
template <int PS, int NW, class SH = LadRoomy>
__global__ void __launch_bounds__(LAD_BLOCK) __attribute__((amdgpu_waves_per_eu(SH::WAVES))) lad_solve_kernel(LadArgs A) {
    __shared__ LadLds<PS, NW, SH> m;
    const int s = NW == 1 ? (int)blockIdx.x : (int)A.wide_list[blockIdx.x];
    const int p = A.sp_p[s];
    if (!lad_instance_takes<NW>(A, s, p)) return;
    if (A.need && !A.need[s]) return;
    if (p <= 0) { if (threadIdx.x == 0) { A.status[s] = 0; A.iters[s] = 0; } return; }
    const uint32_t k0 = A.sp_pat_off[s], k1 = A.sp_pat_off[s + 1];
    if constexpr (NW == 1) {
        if (k1 - k0 <= (uint32_t)SH::KLDS) lad_solve_body<PS, true, 1, SH>(A, m, s, p, k0, k1);
        else lad_solve_body<PS, false, 1, SH>(A, m, s, p, k0, k1);
    } else lad_solve_body<PS, false, NW, SH>(A, m, s, p, k0, k1);
}

// Both LP solves of the strain step in ONE launch: solve, take the second-filter decision of this species
// (one thread), and solve again with the dropped columns pinned to zero -- only where a column was dropped;
// elsewhere LP2 == LP1 (m.reset() + no new constraint, profile.rs:1482-1490).
template <int PS, int NW, class SH = LadRoomy>
__global__ void __launch_bounds__(LAD_BLOCK) __attribute__((amdgpu_waves_per_eu(SH::WAVES))) lad_pair_kernel(LadArgs A1, LadArgs A2, SecondFilterArgs F) {
    __shared__ LadLds<PS, NW, SH> m;
    const int s = NW == 1 ? (int)blockIdx.x : (int)A1.wide_list[blockIdx.x];
    const int p = A1.sp_p[s];
    if (!lad_instance_takes<NW>(A1, s, p)) return;
    const uint32_t k0 = A1.sp_pat_off[s], k1 = A1.sp_pat_off[s + 1];
    const bool lds_state = NW == 1 && k1 - k0 <= (uint32_t)SH::KLDS;
    if (p > 0) {
        if constexpr (NW == 1) {
            if (lds_state) lad_solve_body<PS, true, 1, SH>(A1, m, s, p, k0, k1);
            else lad_solve_body<PS, false, 1, SH>(A1, m, s, p, k0, k1);
        } else lad_solve_body<PS, false, NW, SH>(A1, m, s, p, k0, k1);
    } else if (threadIdx.x == 0) { A1.status[s] = 0; A1.iters[s] = 0; }
    __syncthreads();   // x1 / status1 of this species are visible to the workgroup
    if (threadIdx.x == 0) second_filter_species(F, (uint32_t)s);
    __syncthreads();
    if (p <= 0 || !F.need2[s]) return;
    if constexpr (NW == 1) {
        if (lds_state) lad_solve_body<PS, true, 1, SH>(A2, m, s, p, k0, k1);
        else lad_solve_body<PS, false, 1, SH>(A2, m, s, p, k0, k1);
    } else lad_solve_body<PS, false, NW, SH>(A2, m, s, p, k0, k1);
}

// the shape of this launch (lad_shape), or PANTAX_HIP_E_INVALID for an option value that names none
static int lad_shape_checked(Ctx *ctx, uint32_t S, int pmax_bound, LadShape *out) {
    const std::string &opt = ctx->cfg.lad_shape;
    if (!opt.empty() && opt != "auto" && opt != "roomy" && opt != "compact")
        return fail(ctx, PANTAX_HIP_E_INVALID, "lad solver: option lad_shape is \"auto\", \"roomy\" or \"compact\", not \"%s\"", opt.c_str());
    *out = lad_shape(opt, S, ctx->n_cu, pmax_bound);
    return 0;
}

static SecondFilterArgs second_filter_args(const Db *db, LadBatch *lb, const FilterCfg &fc, const double *d_x1, const int32_t *d_status1,
                                           uint8_t *d_fixed2, uint8_t *d_need2) {
    SecondFilterArgs F;
    F.hap_off = db->d_hap_off.p; F.hap_nt = lb->d_hap_nt.p; F.sp_trio = lb->d_sp_trio.p; F.hap_bit = lb->d_hap_bit.p; F.sp_p = lb->d_p.p; F.nnz = db->d_hap_nnz.p;
    F.meanf = db->d_hap_mean.p; F.ratio = lb->d_ratio.p; F.x1 = d_x1; F.status1 = d_status1; F.fc = fc.fc; F.sr = fc.sr;
    F.fixed2 = d_fixed2; F.need2 = d_need2;
    return F;
}
static LadArgs lad_args(const Db *db, LadBatch *lb, const uint8_t *d_need, const uint8_t *d_fixed, double *d_x, int32_t *d_status, int32_t *d_iters) {
    LadArgs A = lad_plain_args(LadRowTables{lb->row_a, lb->d_pat_mask.p, lb->d_pat_start.p, lb->d_sp_pat_off.p},
                               LadLpTables{lb->d_p.p, lb->d_amax.p, db->d_hap_off.p, d_need, d_fixed}, LadOutputs{d_x, d_status, d_iters}, lb->pat_scratch);
    A.wide_list = lb->d_wide_list.p; A.wide_off = lb->d_wide_off.p; A.wide_slot = lb->d_wide_slot.p;
    A.pat_or = lb->d_pat_or.p; A.pat_and = lb->d_pat_and.p; A.wide_W = lb->d_wide_W.p; A.wide_G = lb->d_wide_G.p;
    A.wide_nw = lb->d_wide_nw.p; A.wide_woff = lb->d_wide_woff.p; A.wide_coff = lb->d_wide_woff.p + lb->n_wide;
    A.huge_f64 = lb->d_huge_f64.p; A.huge_i32 = lb->d_huge_i32.p; A.pat_act = lb->d_pat_act.p;
    return A;
}

// The launches of one solve over a LadBatch, for either kernel family: the <= 64-column species by the compact, the roomy 16-column or the 64-column
// instance (one workgroup per species), then the wide and the huge species (one workgroup per entry of wide_list).
struct LadPairFamily { template <int PS, int NW, class SH = LadRoomy> static constexpr auto kernel() { return &lad_pair_kernel<PS, NW, SH>; } };
struct LadSolveFamily { template <int PS, int NW, class SH = LadRoomy> static constexpr auto kernel() { return &lad_solve_kernel<PS, NW, SH>; } };
template <class Family, class... Args>
static void lad_ladder_launch(Ctx *ctx, const LadBatch *lb, uint32_t S, LadShape shape, int pmax_bound, const Args &...args) {
    const auto launch = [&](auto kernel, uint32_t n_workgroups) { hipLaunchKernelGGL(kernel, dim3(n_workgroups), dim3(LAD_BLOCK), 0, ctx->stream, args...); };
    if (shape == LadShape::compact) launch(Family::template kernel<16, 1, LadCompact>(), S);
    else if (pmax_bound <= 16) launch(Family::template kernel<16, 1>(), S);
    else launch(Family::template kernel<LAD_MAXP, 1>(), S);
    if (lb->n_wide > lb->n_huge) launch(Family::template kernel<LAD_WIDEP, LAD_WIDE_NW>(), lb->n_wide);
    if (lb->n_huge) launch(Family::template kernel<1, 0>(), lb->n_wide);
}

#ifdef LAD_PROFILE
// phase table of the solver workgroups (profiling builds): zeroed before the launch, printed after it
static const char *const LAD_PHASE_NAMES[8] = {"vertex+pattern pass", "multipliers+choice", "line-search setup", "bracket", "wide rounds",
                                               "binary rounds", "walk", "basis update"};
static int lad_prof_begin(Ctx *ctx, uint32_t S, DevBuf<unsigned long long> &buf, LadArgs &A) {
    PTX_HIP(ctx, buf.alloc((size_t)S * 16));
    PTX_HIP(ctx, hipMemsetAsync(buf.p, 0, buf.bytes(), ctx->stream));
    A.prof = buf.p;
    return 0;
}
static int lad_prof_end(Ctx *ctx, uint32_t S, DevBuf<unsigned long long> &buf, const int32_t *d_iters) {
    std::vector<unsigned long long> h((size_t)S * 16);
    std::vector<int32_t> it(S);
    PTX_TRY(download(ctx, h.data(), buf.p, h.size()));
    PTX_TRY(download(ctx, it.data(), d_iters, S));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t s = 0; s < S && s < 4; ++s) {
        unsigned long long tot = 0;
        for (int ph = 0; ph < 8; ++ph) tot += h[(size_t)s * 16 + ph];
        if (!tot) continue;
        std::fprintf(stderr, "[lad profile] species %u: %d pivots, %.1f us in the pivot loop (%.1f us per pivot)\n", s, it[s], tot * 0.01, it[s] ? tot * 0.01 / it[s] : 0.0);
        for (int ph = 0; ph < 8; ++ph)
            std::fprintf(stderr, "    %-22s %9.1f us  %5.1f %%  (%llu visits, %.2f us each)\n", LAD_PHASE_NAMES[ph], h[(size_t)s * 16 + ph] * 0.01,
                         100.0 * h[(size_t)s * 16 + ph] / tot, h[(size_t)s * 16 + 8 + ph], h[(size_t)s * 16 + 8 + ph] ? h[(size_t)s * 16 + ph] * 0.01 / h[(size_t)s * 16 + 8 + ph] : 0.0);
    }
    return 0;
}
#endif

// the strain step's two solves + second filter + both objectives: two launches
int lad_pair_launch(Ctx *ctx, const Db *db, LadBatch *lb, const LadRows &rows, int pmax_bound, const FilterCfg &fc) {
    const uint32_t S = db->S;
    LadShape shape;
    PTX_TRY(lad_shape_checked(ctx, S, pmax_bound, &shape));
    LadArgs A1 = lad_args(db, lb, nullptr, nullptr, lb->d_x.p, lb->d_status.p, lb->d_iters.p);
    LadArgs A2 = lad_args(db, lb, nullptr, lb->d_fixed2.p, lb->d_x2.p, lb->d_status2.p, lb->d_iters2.p);
    SecondFilterArgs F = second_filter_args(db, lb, fc, lb->d_x.p, lb->d_status.p, lb->d_fixed2.p, lb->d_need2.p);
#ifdef LAD_PROFILE
    DevBuf<unsigned long long> prof;
    PTX_TRY(lad_prof_begin(ctx, S, prof, A1));   // the first solve only
#endif
    {
        KTimer t(ctx, "lad_pair_kernel");
        lad_ladder_launch<LadPairFamily>(ctx, lb, S, shape, pmax_bound, A1, A2, F);
    }
    PTX_HIP(ctx, hipGetLastError());
#ifdef LAD_PROFILE
    PTX_TRY(lad_prof_end(ctx, S, prof, lb->d_iters.p));
#endif
    return objective_launch(ctx, db, lb, rows, lb->d_need2.p, lb->d_x.p, lb->d_x2.p, lb->d_obj.p, lb->d_obj2.p);
}

int lad_solve_launch(Ctx *ctx, const Db *db, LadBatch *lb, const LadRows &rows, int pmax_bound, const uint8_t *d_need, const uint8_t *d_fixed, double *d_x,
                     double *d_obj, int32_t *d_status, int32_t *d_iters) {
    const uint32_t S = db->S;
    LadShape shape;
    PTX_TRY(lad_shape_checked(ctx, S, pmax_bound, &shape));
    LadArgs A = lad_args(db, lb, d_need, d_fixed, d_x, d_status, d_iters);
#ifdef LAD_PROFILE
    DevBuf<unsigned long long> prof;
    PTX_TRY(lad_prof_begin(ctx, S, prof, A));
#endif
    {
        KTimer t(ctx, "lad_solve_kernel");
        lad_ladder_launch<LadSolveFamily>(ctx, lb, S, shape, pmax_bound, A);
    }
    PTX_HIP(ctx, hipGetLastError());
#ifdef LAD_PROFILE
    PTX_TRY(lad_prof_end(ctx, S, prof, d_iters));
#endif
    return objective_launch(ctx, db, lb, rows, nullptr, d_x, nullptr, d_obj, nullptr);
}

// The solver on plain arrays (lad_args.hpp): one workgroup per entry of A.sp_p, n_lps of them, every one with at most LAD_MAXP columns -- the caller's
// tables stand where a LadBatch's do (pantax_hip_strain_bootstrap: a (replicate, species) pair is one entry).  The two one-word instances only; no
// objective pass behind it.
int lad_args_launch(Ctx *ctx, const LadArgs &A, uint32_t n_lps, int pmax_bound, const char *timer_name) {
    if (n_lps == 0) return 0;
    if (pmax_bound > LAD_MAXP) return fail(ctx, PANTAX_HIP_E_LIMIT, "lad solver: %d columns through the plain-array entry (at most %d)", pmax_bound, LAD_MAXP);
    {
        KTimer t(ctx, timer_name);
        if (pmax_bound <= 16) hipLaunchKernelGGL((lad_solve_kernel<16, 1>), dim3(n_lps), dim3(LAD_BLOCK), 0, ctx->stream, A);
        else hipLaunchKernelGGL((lad_solve_kernel<LAD_MAXP, 1>), dim3(n_lps), dim3(LAD_BLOCK), 0, ctx->stream, A);
    }
    PTX_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace ptx
