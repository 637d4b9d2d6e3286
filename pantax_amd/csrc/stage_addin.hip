// stage_addin.hip -- add-one test of the strain fit (pantax_hip_strain_addin): would the L1 fit of the sample be better with an unreported haplotype in the
// LP, what coverage would it get, and from which reported strain?  The false-negative test beside the leave-one-out test of stage_dropout.hip.  Not a stage
// of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Add-one test of the strain fit"): the columns of a species are its K reported haplotypes and behind them its J
// candidates, W = K + J; the rows are those of the bootstrap's replicate 0 over all W columns; entry 0 pins every candidate column to zero, entry c + 1 frees
// candidate c alone; per entry x, the objective (a sum) and four row counts.
//
// Once per call:
//   front half        boot_front.hpp over the list Sel_s ++ Cand_s: the rows compacted, sorted by (species, mask, a), the base pattern tables;
//   drop_species      (restated as addin_species_kernel) a wave per species: max a (the box of every entry), the first row.
// Per chunk of rounds (addin_plan.hpp; round e holds entry e of every species over ONE copy of the base tables, as in stage_dropout.hip):
//   addin_fill        the replicated pat_mask / pat_start / sp_pat_off, sp_p (0 for a species of fewer than e candidates, one that is not served, or the
//                     all-pinned entry 0 of a species without reported strains), amax, col_off, and the pin bytes: every candidate column but c = e - 1;
//   solver            lad_solve_kernel<16, 1> / <LAD_MAXP, 1> through lad_args_launch (stage_lad.hip); x goes straight to its place in the species' block.
// Once behind the last chunk -- the hot path:
//   addin_objective   work item = (species, fixed slice of its sorted rows): ONE pass over the rows gives the partial objective and counts of all E_s entries.
//                     <TABLE> (W <= 7): the predictions of every entry for every possible mask (2^W <= 128) go to LDS once per slice; a thread takes rows
//                     r, r + 256, .. with its E_s <= 8 accumulators in registers and reads {mask, a} of a row (16 bytes).
//                     <FEW>   (W > 7, E <= 8; slices of a quarter of the length): the same walk over the rows; the entries' x in LDS, and a thread forms
//                     the E predictions of a mask only when the mask of its row differs from the one before (the rows are sorted by mask: once per run).
//                     <WIDE>  (E > 8): the entries' x in LDS, entries across lanes; a wave takes every fourth pattern of the slice, forms the prediction of
//                     its entry once per pattern and takes the pattern's rows 64 at a time; the four waves' sums are added in wave order.
//   addin_finish      a wave per (species, entry): lane l adds the slices l, l + 64, .. in ascending order, one fixed-shape wave reduction.
// The order of every sum is a function of the species' sorted rows and its column counts alone: the same bits under every chunking, route and position.
#include <algorithm>
#include <cmath>
#include <vector>
#include "common.hpp"
#include "addin_plan.hpp"
#include "boot_front.hpp"
#include "lad_args.hpp"
#include "lad_device.hpp"
#include "primitives.hpp"

namespace ptx {

namespace {

// per species: amax = the largest a of its rows (rows are sorted by a inside a pattern), row_off = its first sorted row ([S + 1], the last = N)
__global__ void __launch_bounds__(64) addin_species_kernel(uint32_t S, const uint32_t *__restrict__ bsp_pat_off, const uint32_t *__restrict__ bpat_start,
                                                           const double *__restrict__ base_a, double *__restrict__ amax_sp, uint32_t *__restrict__ row_off) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (s == S) { if (lane == 0) row_off[S] = bpat_start[bsp_pat_off[S]]; return; }
    const uint32_t k0 = bsp_pat_off[s], k1 = bsp_pat_off[s + 1];
    double amax = 0.0;
    for (uint32_t k = k0 + lane; k < k1; k += 64u) amax = fmax(amax, base_a[bpat_start[k + 1] - 1]);
    amax = wave_reduce(amax, [](double x, double y) { return fmax(x, y); });
    if (lane == 0) { amax_sp[s] = amax; row_off[s] = bpat_start[k0]; }
}

struct AddinFill {   // what addin_fill_kernel reads and writes
    const uint64_t *bpat_mask;                // [P]
    const uint32_t *bpat_start;               // [P + 1]
    const uint32_t *bsp_pat_off;              // [S + 1]
    const uint64_t *k_off, *w_off, *x_off;    // [S + 1] reported haplotypes, columns, x blocks
    const double *amax_sp;                    // [S]
    uint32_t S, P;
    uint64_t *pat_mask;                       // [rounds of the chunk][P + 1]
    uint32_t *pat_start;                      // [rounds of the chunk][P + 1]
    uint32_t *sp_pat_off;                     // [rounds of the chunk][S + 1]
    int32_t *sp_p;
    double *amax;
    uint64_t *col_off;
    uint8_t *fixed;                           // [X], zero where no column is pinned
};
// rounds e0 .. e0 + nr - 1
__global__ void __launch_bounds__(256) addin_fill_kernel(AddinFill T, uint32_t e0, uint32_t nr) {
    const uint64_t t0 = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    const uint64_t np = (uint64_t)nr * (T.P + 1), nq = (uint64_t)nr * (T.S + 1);
    for (uint64_t i = t0; i < np; i += stride) {
        const uint32_t k = (uint32_t)(i % (T.P + 1));
        T.pat_start[i] = T.bpat_start[k];
        T.pat_mask[i] = k < T.P ? T.bpat_mask[k] : 0ull;
    }
    for (uint64_t i = t0; i < nq; i += stride) {
        const uint32_t rl = (uint32_t)(i / (T.S + 1)), s = (uint32_t)(i % (T.S + 1)), e = e0 + rl;
        T.sp_pat_off[i] = rl * (T.P + 1) + T.bsp_pat_off[s];   // (the closing entry s == S: the round's closing pattern slot)
        bool solve = false;
        uint64_t K = 0, W = 0;
        if (s < T.S) {
            K = T.k_off[s + 1] - T.k_off[s];
            W = T.w_off[s + 1] - T.w_off[s];
            // K == 0, e == 0: every column is pinned -- x = 0 is the one point of the box and no LP is solved
            solve = W >= 1 && W <= ADDIN_MAX_W && e <= W - K && T.bsp_pat_off[s + 1] > T.bsp_pat_off[s] && !(K == 0 && e == 0);
        }
        T.sp_p[i] = solve ? (int32_t)W : 0;
        T.amax[i] = s < T.S ? T.amax_sp[s] : 0.0;
        T.col_off[i] = solve ? T.x_off[s] + (uint64_t)e * W : 0ull;
        if (solve) {
            uint8_t *f = T.fixed + T.x_off[s] + (uint64_t)e * W + K;   // the candidate columns of the entry: all pinned but c = e - 1
            for (uint64_t c = 0; c < W - K; ++c) if (c + 1 != e) f[c] = 1;
        }
    }
}

// ---- the objective and count pass
struct AddinObj {
    const uint32_t *sl_sp, *sl_row0;   // [slices] species and first row of the slice
    const uint64_t *sl_part;           // [slices] first partial of the slice (one per entry of its species)
    const uint32_t *row_off;           // [S + 1]
    const uint32_t *bsp_pat_off, *bpat_start;
    const uint64_t *bpat_mask, *row_mask;
    const double *base_a;
    const uint64_t *k_off, *w_off, *x_off;
    const double *x;
    double *part_obj;                  // [partials]
    uint32_t *part_cnt;                // [partials][4] = member, novel, better, worse (a slice holds fewer than 2^32 rows); entry 0: rows, rows without a reported bit, 0, 0
};
constexpr int ADDIN_LD_MAX = 65;   // row length of the entries' x in LDS: W | 1, odd -- lanes e, e + 1 read different banks

template <int INST>
__global__ void __launch_bounds__(256) addin_objective_kernel(AddinObj T) {
    const uint32_t sl = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t s = T.sl_sp[sl];
    const uint32_t K = (uint32_t)(T.k_off[s + 1] - T.k_off[s]), W = (uint32_t)(T.w_off[s + 1] - T.w_off[s]), E = W - K + 1;
    if ((int)addin_instance(W, E) != INST) return;   // (block-uniform) another instance takes the slice
    const uint32_t r0 = T.sl_row0[sl], r1 = (uint32_t)min((uint64_t)r0 + addin_slice_rows(W, E), (uint64_t)T.row_off[s + 1]);
    const double *xg = T.x + T.x_off[s];
    double *out_obj = T.part_obj + T.sl_part[sl];
    uint32_t *out_cnt = T.part_cnt + T.sl_part[sl] * 4;
    const uint64_t low = K >= 64u ? ~0ull : (1ull << K) - 1ull;   // the reported columns
    if constexpr (INST != (int)ADDIN_WIDE) {
        constexpr int NE = (int)ADDIN_FEW_E;
        constexpr int NPRED = INST == (int)ADDIN_TABLE ? 128 * NE : NE * ADDIN_LD_MAX;
        __shared__ double pred[NPRED];   // TABLE: [mask][entry]; FEW: the entries' x, [entry][W | 1]
        __shared__ double red_d[4][NE];
        __shared__ uint32_t red_u[4][NE][4];
        const uint32_t ld = W | 1u;
        if constexpr (INST == (int)ADDIN_TABLE) {
            for (uint32_t i = tid; i < 128u * NE; i += 256u) {
                const uint32_t m = i / NE, e = i % NE;
                pred[i] = (e < E && m < (1u << W)) ? mdot((uint64_t)m, xg + (size_t)e * W) : 0.0;
            }
        } else {
            for (uint32_t i = tid; i < E * W; i += 256u) pred[(i / W) * ld + (i % W)] = xg[i];
        }
        __syncthreads();
        double acc[NE], p[NE];
        uint32_t member[NE], novel[NE], better[NE], worse[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) { acc[e] = 0.0; p[e] = 0.0; member[e] = novel[e] = better[e] = worse[e] = 0u; }
        uint64_t prev = 0ull;   // (no row has an empty mask)
        for (uint32_t r = r0 + tid; r < r1; r += 256u) {
            const uint64_t m = T.row_mask[r];
            const double a = T.base_a[r];
            if constexpr (INST == (int)ADDIN_TABLE) {
                const double *pm = pred + ((uint32_t)m & 127u) * NE;
#pragma unroll
                for (int e = 0; e < NE; ++e) p[e] = pm[e];
            } else if (m != prev) {
#pragma unroll
                for (int e = 0; e < NE; ++e) p[e] = (uint32_t)e < E ? mdot(m, pred + e * ld) : 0.0;
                prev = m;
            }
            const uint32_t cm = K >= 64u ? 0u : (uint32_t)((m >> K) & 0x7Full);   // candidate bits (at most seven here)
            const uint32_t nolow = (m & low) == 0ull ? 1u : 0u;
            const double res0 = fabs(p[0] - a);
            acc[0] += res0; member[0] += 1u; novel[0] += nolow;
#pragma unroll
            for (int e = 1; e < NE; ++e) {
                const double res = fabs(p[e] - a);
                const uint32_t bit = (cm >> (e - 1)) & 1u;
                acc[e] += res;
                member[e] += bit; novel[e] += bit & nolow;
                better[e] += res < res0 ? 1u : 0u;
                worse[e] += res > res0 ? 1u : 0u;
            }
        }
        const auto addu = [](uint32_t x, uint32_t y) { return x + y; };
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const double a_ = wave_reduce(acc[e], [](double x, double y) { return x + y; });
            const uint32_t c0 = wave_reduce(member[e], addu), c1 = wave_reduce(novel[e], addu), c2 = wave_reduce(better[e], addu), c3 = wave_reduce(worse[e], addu);
            if (lane == 0) { red_d[wave][e] = a_; red_u[wave][e][0] = c0; red_u[wave][e][1] = c1; red_u[wave][e][2] = c2; red_u[wave][e][3] = c3; }
        }
        __syncthreads();
        if (tid < E) {
            double t = 0.0;
            for (int w = 0; w < 4; ++w) t += red_d[w][tid];   // wave order: fixed
            out_obj[tid] = t;
            for (int c = 0; c < 4; ++c) out_cnt[tid * 4 + c] = red_u[0][tid][c] + red_u[1][tid][c] + red_u[2][tid][c] + red_u[3][tid][c];
        }
    } else {
        __shared__ double xs[ADDIN_LD_MAX * ADDIN_LD_MAX];
        __shared__ double red_d[4][ADDIN_LD_MAX];
        __shared__ uint32_t red_u[4][ADDIN_LD_MAX][4];
        const uint32_t ld = W | 1u;
        for (uint32_t i = tid; i < E * W; i += 256u) xs[(i / W) * ld + (i % W)] = xg[i];
        __syncthreads();
        // the patterns that meet the slice: kA = the last one that starts at or before r0, kB = one beyond the last that starts before r1
        uint32_t kA, kB;
        {
            uint32_t lo = T.bsp_pat_off[s], hi = T.bsp_pat_off[s + 1];   // first pattern that starts beyond r0
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (T.bpat_start[mid] <= r0) lo = mid + 1; else hi = mid; }
            kA = lo - 1;
            hi = T.bsp_pat_off[s + 1];                                  // first pattern that starts at or beyond r1
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (T.bpat_start[mid] < r1) lo = mid + 1; else hi = mid; }
            kB = lo;
        }
        // lane l holds entry l, and lane 0 entry 64 beside it (J = 64)
        const uint32_t e0 = lane, e1 = lane + 64u;
        const bool on0 = e0 < E, on1 = e1 < E;
        double acc0 = 0.0, acc1 = 0.0;
        uint32_t cnt0[4] = {0u, 0u, 0u, 0u}, cnt1[4] = {0u, 0u, 0u, 0u};
        for (uint32_t k = kA + wave; k < kB; k += 4u) {
            const uint64_t mask = T.bpat_mask[k];
            const uint32_t a = max(T.bpat_start[k], r0), b = min(T.bpat_start[k + 1], r1), n = b - a;
            const uint32_t nolow = (mask & low) == 0ull ? n : 0u;
            // the predictions, once per pattern
            const double p_ref = mdot(mask, xs);
            const double p0 = on0 ? mdot(mask, xs + e0 * ld) : 0.0, p1 = on1 ? mdot(mask, xs + e1 * ld) : 0.0;
            if (e0 == 0u) { cnt0[0] += n; cnt0[1] += nolow; }
            else if (on0) { const uint32_t bit = (uint32_t)((mask >> (K + e0 - 1u)) & 1ull); cnt0[0] += bit * n; cnt0[1] += bit * nolow; }   // (K + e0 - 1 < W <= 64)
            if (on1) { const uint32_t bit = (uint32_t)((mask >> (K + e1 - 1u)) & 1ull); cnt1[0] += bit * n; cnt1[1] += bit * nolow; }
            for (uint32_t base = a; base < b; base += 64u) {
                const uint32_t cnt = min(64u, b - base);
                const double al = lane < cnt ? T.base_a[base + lane] : 0.0;
                for (uint32_t i = 0; i < cnt; ++i) {
                    const double av = __shfl(al, (int)i);
                    const double res_ref = fabs(p_ref - av), res0 = fabs(p0 - av), res1 = fabs(p1 - av);
                    acc0 += res0; cnt0[2] += res0 < res_ref ? 1u : 0u; cnt0[3] += res0 > res_ref ? 1u : 0u;
                    acc1 += res1; cnt1[2] += res1 < res_ref ? 1u : 0u; cnt1[3] += res1 > res_ref ? 1u : 0u;
                }
            }
        }
        if (on0) { red_d[wave][e0] = acc0; for (int c = 0; c < 4; ++c) red_u[wave][e0][c] = cnt0[c]; }
        if (on1) { red_d[wave][e1] = acc1; for (int c = 0; c < 4; ++c) red_u[wave][e1][c] = cnt1[c]; }
        __syncthreads();
        if (tid < E) {
            double t = 0.0;
            for (int w = 0; w < 4; ++w) t += red_d[w][tid];   // wave order: fixed
            out_obj[tid] = t;
            for (int c = 0; c < 4; ++c) out_cnt[tid * 4 + c] = red_u[0][tid][c] + red_u[1][tid][c] + red_u[2][tid][c] + red_u[3][tid][c];
        }
    }
}

// obj[q] and count[q][4] of every entry of a species with slices: the slice partials in ascending order
__global__ void __launch_bounds__(256) addin_finish_kernel(const uint32_t *__restrict__ sp_sl_off, const uint64_t *__restrict__ sl_part, const uint64_t *__restrict__ cand_off,
                                                           const double *__restrict__ part_obj, const uint32_t *__restrict__ part_cnt, double *__restrict__ obj,
                                                           unsigned long long *__restrict__ cnt) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t l0 = sp_sl_off[s], l1 = sp_sl_off[s + 1];
    if (l1 == l0) return;
    const uint32_t E = (uint32_t)(cand_off[s + 1] - cand_off[s]) + 1u;
    const uint64_t p0 = sl_part[l0];   // the species' partials: slice l - l0 at p0 + (l - l0) * E
    const auto addu = [](unsigned long long x, unsigned long long y) { return x + y; };
    for (uint32_t e = wave; e < E; e += 4u) {
        double t = 0.0;
        unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};
        for (uint32_t l = l0 + lane; l < l1; l += 64u) {
            const uint64_t i = p0 + (uint64_t)(l - l0) * E + e;
            t += part_obj[i];
            for (int j = 0; j < 4; ++j) c[j] += part_cnt[i * 4 + j];
        }
        t = wave_reduce(t, [](double x, double y) { return x + y; });
        for (int j = 0; j < 4; ++j) c[j] = wave_reduce(c[j], addu);
        if (lane == 0) {
            const uint64_t q = cand_off[s] + s + e;
            obj[q] = t;
            for (int j = 0; j < 4; ++j) cnt[q * 4 + j] = c[j];
        }
    }
}

}  // namespace

// both sets validated by the caller
int addin_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *cand_off, const uint32_t *cand_hap, double *x_out, double *obj_out,
                 int32_t *status_out, uint64_t *rows_out, uint64_t *count_out) {
    const uint32_t S = db->S;
    if (S == 0) return 0;
    const uint64_t J = cand_off[S], Q = J + S;
    std::vector<uint64_t> x_off((size_t)S + 1), w_off((size_t)S + 1, 0);
    if (!addin_x_offsets(S, sel_off, cand_off, x_off.data()))
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_addin: the x blocks of %llu reported and %llu candidate entries exceed 64-bit positions", (unsigned long long)sel_off[S], (unsigned long long)J);
    const uint64_t X = x_off[S];
    // ---- the columns of every species: Sel_s, then Cand_s
    std::vector<uint32_t> w_hap;
    w_hap.reserve((size_t)(sel_off[S] + J));
    for (uint32_t s = 0; s < S; ++s) {
        w_hap.insert(w_hap.end(), sel_hap + sel_off[s], sel_hap + sel_off[s + 1]);
        w_hap.insert(w_hap.end(), cand_hap + cand_off[s], cand_hap + cand_off[s + 1]);
        w_off[s + 1] = w_hap.size();
    }
    BootFront F;
    PTX_TRY(boot_front_build(ctx, db, (const unsigned long long *)db->d_bases.p, w_off.data(), w_hap.data(), nullptr, 0, ctx->cfg.addin_route, "strain_addin", [](uint64_t) { return 0; }, F));
    // results on the host; the caller's arrays are written at the very end
    std::vector<double> hx((size_t)X, 0.0), hobj((size_t)Q, 0.0);
    std::vector<int32_t> hstatus((size_t)Q, 1);
    std::vector<uint64_t> hrows(S, 0), hcnt((size_t)Q * 4, 0);
    uint64_t j_max = 0;   // most candidates of a served species
    for (uint32_t s = 0; s < S; ++s) {
        if (F.pre_host[s] == PANTAX_HIP_E_LIMIT) std::fill(hstatus.begin() + (cand_off[s] + s), hstatus.begin() + (cand_off[s + 1] + s + 1), (int32_t)PANTAX_HIP_E_LIMIT);
        else j_max = std::max(j_max, cand_off[s + 1] - cand_off[s]);
    }
    const auto deliver = [&]() {
        std::copy(hx.begin(), hx.end(), x_out); std::copy(hobj.begin(), hobj.end(), obj_out); std::copy(hstatus.begin(), hstatus.end(), status_out);
        std::copy(hrows.begin(), hrows.end(), rows_out); std::copy(hcnt.begin(), hcnt.end(), count_out);
        return 0;
    };
    if (F.N == 0) return deliver();
    const uint32_t P = F.P, N = (uint32_t)F.N;
    const uint64_t rounds = j_max + 1;
    // ---- per species: the box and the rows
    DevBuf<double> d_amax_sp;
    DevBuf<uint32_t> d_row_off;
    PTX_HIP(ctx, d_amax_sp.alloc(S)); PTX_HIP(ctx, d_row_off.alloc((size_t)S + 1));
    {
        KTimer tm(ctx, "addin_species_kernel");
        hipLaunchKernelGGL(addin_species_kernel, dim3(S + 1), dim3(64), 0, ctx->stream, S, F.d_bsp_pat_off.p, F.d_bpat_start.p, F.base_a, d_amax_sp.p, d_row_off.p);
    }
    PTX_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> row_off((size_t)S + 1);
    PTX_TRY(download(ctx, row_off.data(), d_row_off.p, (size_t)S + 1));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (row_off[S] != N) return fail(ctx, PANTAX_HIP_E_STATE, "strain_addin: internal (the species' rows end at %u of %u)", row_off[S], N);
    // ---- the plan of the chunks
    uint64_t cap = ctx->cfg.addin_patterns_max;
    if (cap == 0) {
        size_t free_b = 0, total_b = 0;
        PTX_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        cap = addin_default_cap(free_b);
    }
    AddinPlan plan;
    std::string why;
    if (!addin_plan(P, S, rounds, cap, plan, why)) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s", why.c_str());
    // ---- the slices of the objective pass
    std::vector<uint32_t> sl_sp, sl_row0, sp_sl_off((size_t)S + 1, 0);
    std::vector<uint64_t> sl_part;
    uint64_t n_part = 0;
    bool any[3] = {false, false, false};
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = sel_off[s + 1] - sel_off[s], Js = cand_off[s + 1] - cand_off[s], rows = row_off[s + 1] - row_off[s];
        sp_sl_off[s] = (uint32_t)sl_sp.size();
        hrows[s] = rows;
        if (F.pre_host[s] != BOOT_PENDING || rows == 0) continue;   // (a species beyond the limit or without a column has no rows)
        for (uint64_t e = 0; e <= Js; ++e) hstatus[cand_off[s] + s + e] = BOOT_PENDING;
        if (K == 0) hstatus[cand_off[s] + s] = 0;                   // every column pinned: nothing to solve, x = 0
        const uint64_t E = Js + 1, L = addin_slice_rows(K + Js, E);
        any[addin_instance(K + Js, E)] = true;
        for (uint64_t r = row_off[s]; r < row_off[s + 1]; r += L) { sl_sp.push_back(s); sl_row0.push_back((uint32_t)r); sl_part.push_back(n_part); n_part += E; }
    }
    sp_sl_off[S] = (uint32_t)sl_sp.size();
    const uint32_t n_slices = (uint32_t)sl_sp.size();
    // ---- all scratch, once; nothing is allocated inside the loop
    const uint64_t cp = plan.chunk_patterns, ce = plan.chunk_entries;
    DevBuf<uint32_t> d_pat_start, d_sp_pat_off, d_sl_sp, d_sl_row0, d_sp_sl_off, d_part_cnt;
    DevBuf<uint64_t> d_pat_mask, d_col_off, d_x_off, d_k_off, d_cand_off, d_sl_part;
    DevBuf<unsigned long long> d_cnt;
    DevBuf<double> d_amax, d_x, d_obj, d_part_obj;
    DevBuf<int32_t> d_sp_p, d_status, d_iters;
    DevBuf<uint8_t> d_fixed;
    LadPatScratch pat_scratch;
    PTX_HIP(ctx, d_pat_start.alloc(cp + 1)); PTX_HIP(ctx, d_pat_mask.alloc(cp)); PTX_HIP(ctx, d_sp_pat_off.alloc(ce + 1));
    PTX_TRY(pat_scratch.alloc(ctx, cp));
    PTX_HIP(ctx, d_sp_p.alloc(ce)); PTX_HIP(ctx, d_amax.alloc(ce)); PTX_HIP(ctx, d_col_off.alloc(ce)); PTX_HIP(ctx, d_status.alloc(ce)); PTX_HIP(ctx, d_iters.alloc(ce));
    PTX_HIP(ctx, d_x.alloc(std::max<uint64_t>(X, 1))); PTX_HIP(ctx, d_fixed.alloc(std::max<uint64_t>(X, 1)));
    PTX_HIP(ctx, d_obj.alloc(Q)); PTX_HIP(ctx, d_cnt.alloc(Q * 4));
    PTX_HIP(ctx, d_part_obj.alloc(std::max<uint64_t>(n_part, 1))); PTX_HIP(ctx, d_part_cnt.alloc(std::max<uint64_t>(n_part, 1) * 4));
    DevBuf<double> d_yard;
    if (ctx->cfg.addin_yardstick) PTX_HIP(ctx, d_yard.alloc(ce));
    PTX_TRY(upload(ctx, d_x_off, x_off.data(), x_off.size()));
    PTX_TRY(upload(ctx, d_k_off, sel_off, (size_t)S + 1)); PTX_TRY(upload(ctx, d_cand_off, cand_off, (size_t)S + 1));
    PTX_TRY(upload(ctx, d_sl_sp, sl_sp.data(), sl_sp.size())); PTX_TRY(upload(ctx, d_sl_row0, sl_row0.data(), sl_row0.size()));
    PTX_TRY(upload(ctx, d_sl_part, sl_part.data(), sl_part.size())); PTX_TRY(upload(ctx, d_sp_sl_off, sp_sl_off.data(), sp_sl_off.size()));
    PTX_HIP(ctx, hipMemsetAsync(d_x.p, 0, std::max<uint64_t>(X, 1) * sizeof(double), ctx->stream));
    PTX_HIP(ctx, hipMemsetAsync(d_fixed.p, 0, std::max<uint64_t>(X, 1), ctx->stream));
    PTX_HIP(ctx, hipMemsetAsync(d_obj.p, 0, Q * sizeof(double), ctx->stream));
    PTX_HIP(ctx, hipMemsetAsync(d_cnt.p, 0, Q * 4 * sizeof(unsigned long long), ctx->stream));
    AddinFill T;
    T.bpat_mask = F.d_bpat_mask.p; T.bpat_start = F.d_bpat_start.p; T.bsp_pat_off = F.d_bsp_pat_off.p; T.k_off = d_k_off.p; T.w_off = F.d_sel_off.p; T.x_off = d_x_off.p;
    T.amax_sp = d_amax_sp.p; T.S = S; T.P = P;
    T.pat_mask = d_pat_mask.p; T.pat_start = d_pat_start.p; T.sp_pat_off = d_sp_pat_off.p; T.sp_p = d_sp_p.p; T.amax = d_amax.p; T.col_off = d_col_off.p;
    T.fixed = d_fixed.p;
    std::vector<int32_t> c_status((size_t)ce);
    for (uint64_t e0 = 0; e0 < rounds; e0 += plan.per_chunk) {
        const uint32_t nr = (uint32_t)std::min<uint64_t>(plan.per_chunk, rounds - e0), nq = nr * (S + 1);
        {
            KTimer tm(ctx, "addin_fill_kernel");
            hipLaunchKernelGGL(addin_fill_kernel, dim3(grid_for((uint64_t)nr * (std::max<uint64_t>(P, S) + 1), 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, T, (uint32_t)e0, nr);
        }
        PTX_HIP(ctx, hipGetLastError());
        PTX_HIP(ctx, hipMemsetAsync(d_status.p, 0, (size_t)nq * sizeof(int32_t), ctx->stream));
        const LadArgs LA = lad_plain_args(LadRowTables{F.base_a, d_pat_mask.p, d_pat_start.p, d_sp_pat_off.p}, LadLpTables{d_sp_p.p, d_amax.p, d_col_off.p, nullptr, d_fixed.p},
                                          LadOutputs{d_x.p, d_status.p, d_iters.p}, pat_scratch);
        PTX_TRY(lad_args_launch(ctx, LA, nq, (int)F.k_max, "lad_solve_kernel<addin>"));
        // measurement only (option addin_yardstick): the bootstrap's objective pass over the same rows, a pass per round; its sums are not delivered
        if (ctx->cfg.addin_yardstick)
            PTX_TRY(boot_objective_launch(ctx, nq, d_sp_p.p, d_sp_pat_off.p, d_pat_mask.p, d_pat_start.p, F.base_a, d_col_off.p, d_x.p, pat_scratch.sc_s.p, d_yard.p, "boot_objective_kernel<addin>"));
        PTX_TRY(download(ctx, c_status.data(), d_status.p, (size_t)nq));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t rl = 0; rl < nr; ++rl)
            for (uint32_t s = 0; s < S; ++s) {
                const uint64_t Js = cand_off[s + 1] - cand_off[s], e = e0 + rl;
                if (e > Js || F.pre_host[s] != BOOT_PENDING) continue;
                int32_t &st = hstatus[cand_off[s] + s + e];
                if (st == BOOT_PENDING) st = c_status[(size_t)rl * (S + 1) + s] == 0 ? 0 : PANTAX_HIP_E_SOLVER;
            }
    }
    // ---- objectives and counts of all entries: one pass over the rows
    if (n_slices) {
        AddinObj O;
        O.sl_sp = d_sl_sp.p; O.sl_row0 = d_sl_row0.p; O.sl_part = d_sl_part.p; O.row_off = d_row_off.p; O.bsp_pat_off = F.d_bsp_pat_off.p; O.bpat_start = F.d_bpat_start.p;
        O.bpat_mask = F.d_bpat_mask.p; O.row_mask = F.row_mask; O.base_a = F.base_a; O.k_off = d_k_off.p; O.w_off = F.d_sel_off.p; O.x_off = d_x_off.p; O.x = d_x.p;
        O.part_obj = d_part_obj.p; O.part_cnt = d_part_cnt.p;
        if (any[ADDIN_TABLE]) {
            KTimer tm(ctx, "addin_objective_kernel<table>");
            hipLaunchKernelGGL((addin_objective_kernel<(int)ADDIN_TABLE>), dim3(n_slices), dim3(256), 0, ctx->stream, O);
        }
        if (any[ADDIN_FEW]) {
            KTimer tm(ctx, "addin_objective_kernel<few>");
            hipLaunchKernelGGL((addin_objective_kernel<(int)ADDIN_FEW>), dim3(n_slices), dim3(256), 0, ctx->stream, O);
        }
        if (any[ADDIN_WIDE]) {
            KTimer tm(ctx, "addin_objective_kernel<wide>");
            hipLaunchKernelGGL((addin_objective_kernel<(int)ADDIN_WIDE>), dim3(n_slices), dim3(256), 0, ctx->stream, O);
        }
        PTX_HIP(ctx, hipGetLastError());
        {
            KTimer tm(ctx, "addin_finish_kernel");
            hipLaunchKernelGGL(addin_finish_kernel, dim3(S), dim3(256), 0, ctx->stream, d_sp_sl_off.p, d_sl_part.p, d_cand_off.p, d_part_obj.p, d_part_cnt.p, d_obj.p, d_cnt.p);
        }
        PTX_HIP(ctx, hipGetLastError());
    }
    if (X) PTX_TRY(download(ctx, hx.data(), d_x.p, (size_t)X));
    PTX_TRY(download(ctx, hobj.data(), d_obj.p, (size_t)Q));
    PTX_TRY(download(ctx, (unsigned long long *)hcnt.data(), (const unsigned long long *)d_cnt.p, (size_t)Q * 4));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t s = 0; s < S; ++s) {   // a pinned column is exactly +0.0 (the solver clamps to [0, 0] and may leave the sign bit)
        const uint64_t K = sel_off[s + 1] - sel_off[s], Js = cand_off[s + 1] - cand_off[s], W = K + Js;
        for (uint64_t e = 0; e <= Js; ++e)
            for (uint64_t c = 0; c < Js; ++c) if (c + 1 != e) hx[x_off[s] + e * W + K + c] = 0.0;
    }
    return deliver();
}

}  // namespace ptx
