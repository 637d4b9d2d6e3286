// stage_objective.hip -- the LP objective (1/n) sum |m_v . x - a_v| of both solutions of the strain step (profile.rs:1440-1450): from the nodes,
// or from the sorted rows and the patterns' predictions.
#include <algorithm>
#include <cstdio>
#include <vector>
#include "lad.hpp"
#include "lad_device.hpp"
#include "primitives.hpp"
#include "wave.hpp"

namespace ptx {

// chunks per species actually used: ~2048 workgroups in all (one species: 256 chunks; a hundred species: 20)
static inline uint32_t stat_chunks(uint32_t S, uint32_t target = 2048u) { uint32_t c = target / (S ? S : 1u); return c < 1u ? 1u : (c > (uint32_t)STAT_CHUNKS ? (uint32_t)STAT_CHUNKS : c); }

// objective (1/n) sum_{a_v>0} |m_v . x - a_v| over the nodes of each solved species (profile.rs:1440-1450),
// for the first solution and -- where need2 says there was a second solve -- the second one, in one pass over
// the nodes.  The workgroup that finishes a species last adds the chunk partials in fixed order.
__global__ void __launch_bounds__(256) objective_kernel(const int32_t *__restrict__ sp_p, const uint8_t *__restrict__ need2,
                                                        const uint32_t *__restrict__ node_base, const double *__restrict__ ab,
                                                        const unsigned long long *__restrict__ mask, const uint64_t *__restrict__ col_off,
                                                        const uint32_t *__restrict__ wide_off, const uint32_t *__restrict__ wide_nw,
                                                        const unsigned long long *__restrict__ maskw, const double *__restrict__ x1,
                                                        const double *__restrict__ x2, double *part /*[S][STAT_CHUNKS][2]*/,
                                                        uint32_t *__restrict__ done /*[S], zero between launches*/,
                                                        const uint32_t *__restrict__ nvalid, double *__restrict__ obj1, double *__restrict__ obj2, uint32_t nch) {
    __shared__ double red[4];
    __shared__ double xs1[LAD_WIDEP], xs2[LAD_WIDEP];
    __shared__ int s_last;
    const int s = blockIdx.x / nch;
    const int p = sp_p[s];
    if (p <= 0) return;
    const bool two = x2 && need2 && need2[s];
    const uint32_t ch = blockIdx.x % nch;
    static_assert(LAD_WIDEP <= 256, "one column per thread");
    if ((int)threadIdx.x < p && p <= LAD_WIDEP) { xs1[threadIdx.x] = x1[col_off[s] + threadIdx.x]; xs2[threadIdx.x] = two ? x2[col_off[s] + threadIdx.x] : 0.0; }
    __syncthreads();
    const uint32_t b = node_base[s], e = node_base[s + 1];
    const uint32_t per = (e - b + nch - 1) / nch;
    uint32_t lo = b + ch * per, hi = lo + per;
    if (hi > e) hi = e;
    double acc1 = 0.0, acc2 = 0.0;
    if (p > LAD_MAXP && wide_nw[s] > (uint32_t)LAD_WIDE_NW) {   // huge species: any number of mask words, x read where the solver left it
        const unsigned long long *mw = maskw + (size_t)wide_off[s] * LAD_WIDE_NW;
        const int nw = (int)wide_nw[s];
        const double *X1 = x1 + col_off[s], *X2 = two ? x2 + col_off[s] : nullptr;
        for (uint32_t v = lo + threadIdx.x; v < hi; v += 256) {
            const double a = ab[v];
            if (a > 0.0) {
                const uint64_t *mn = (const uint64_t *)(mw + (size_t)(v - b) * nw);
                acc1 += fabs(mdotx<0>(mn, nw, X1) - a);
                if (two) acc2 += fabs(mdotx<0>(mn, nw, X2) - a);
            }
        }
    } else if (p > LAD_MAXP) {   // wide species: the mask words of the node
        const unsigned long long *mw = maskw + (size_t)wide_off[s] * LAD_WIDE_NW;
        for (uint32_t v = lo + threadIdx.x; v < hi; v += 256) {
            const double a = ab[v];
            if (a > 0.0) {
                const uint64_t *m4 = (const uint64_t *)(mw + (size_t)(v - b) * LAD_WIDE_NW);
                acc1 += fabs(mdotw<LAD_WIDE_NW>(m4, xs1) - a);
                if (two) acc2 += fabs(mdotw<LAD_WIDE_NW>(m4, xs2) - a);
            }
        }
    } else
    for (uint32_t v = lo + threadIdx.x; v < hi; v += 256) {
        const double a = ab[v];
        if (a > 0.0) {
            const unsigned long long mk = mask[v];
            acc1 += fabs(mdot(mk, xs1) - a);
            if (two) acc2 += fabs(mdot(mk, xs2) - a);
        }
    }
    acc1 = block_sum_f64<256>(acc1, red);
    acc2 = block_sum_f64<256>(acc2, red);
    if (threadIdx.x == 0) {
        part[((size_t)s * nch + ch) * 2] = acc1;
        part[((size_t)s * nch + ch) * 2 + 1] = acc2;
        // release: the partials are visible device-wide before the count; acquire: the last arriver sees all of them
        s_last = __hip_atomic_fetch_add(&done[s], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nch - 1;
    }
    __syncthreads();
    if (!s_last) return;
    // the last workgroup adds the partials: thread c takes chunk c (nch <= block size), fixed-shape block sum
    static_assert(STAT_CHUNKS <= 256, "one partial per thread");
    double t1 = 0.0, t2 = 0.0;
    if (threadIdx.x < nch) { t1 = part[((size_t)s * nch + threadIdx.x) * 2]; t2 = part[((size_t)s * nch + threadIdx.x) * 2 + 1]; }
    t1 = block_sum_f64<256>(t1, red);
    t2 = block_sum_f64<256>(t2, red);
    if (threadIdx.x != 0) return;
    obj1[s] = nvalid[s] ? t1 / (double)nvalid[s] : 0.0;
    if (two) obj2[s] = nvalid[s] ? t2 / (double)nvalid[s] : 0.0;
    done[s] = 0;
}

// The same objective from the SORTED ROWS (the many-species step, species of at most 64 columns): every row of a pattern has the pattern's
// prediction, so the pass reads 8 bytes per row -- 1.6 GB at cfg4 where the pass over the nodes reads abundance and mask of every node,
// 5.1 GB; the nodes with a > 0 and an empty mask, which are no rows, contribute the constant c0[s] that the row sort's histogram pass
// summed on its way (fixed order).  The sums run in another order than objective_kernel's: equal to the last bits of a double, not bit for bit.
__global__ void __launch_bounds__(256) pattern_pred_kernel(const int32_t *__restrict__ sp_p, const uint8_t *__restrict__ need2, const uint32_t *__restrict__ sp_pat_off,
                                                           const uint64_t *__restrict__ pat_mask, const uint64_t *__restrict__ col_off, const double *__restrict__ x1,
                                                           const double *__restrict__ x2, double *__restrict__ pred1, double *__restrict__ pred2) {
    __shared__ double xs1[LAD_MAXP], xs2[LAD_MAXP];
    const int s = blockIdx.x, p = sp_p[s];
    if (p <= 0 || p > LAD_MAXP) return;
    const bool two = x2 && need2 && need2[s];
    if ((int)threadIdx.x < p) { xs1[threadIdx.x] = x1[col_off[s] + threadIdx.x]; xs2[threadIdx.x] = two ? x2[col_off[s] + threadIdx.x] : 0.0; }
    __syncthreads();
    for (uint32_t k = sp_pat_off[s] + threadIdx.x; k < sp_pat_off[s + 1]; k += 256) {
        const uint64_t mk = pat_mask[k];
        pred1[k] = mdot(mk, xs1);
        if (two) pred2[k] = mdot(mk, xs2);
    }
}
__global__ void __launch_bounds__(256) objective_rows_kernel(const int32_t *__restrict__ sp_p, const uint8_t *__restrict__ need2, const uint32_t *__restrict__ sp_pat_off,
                                                             const uint32_t *__restrict__ pat_start, const double *__restrict__ row_a, const double *__restrict__ pred1,
                                                             const double *__restrict__ pred2, const double *__restrict__ c0, double *part /*[S][STAT_CHUNKS][2]*/,
                                                             uint32_t *__restrict__ done /*[S], zero between launches*/, const uint32_t *__restrict__ nvalid,
                                                             double *__restrict__ obj1, double *__restrict__ obj2, uint32_t nch, bool have2) {
    __shared__ double red[4];
    __shared__ int s_last;
    const int s = blockIdx.x / nch;
    const int p = sp_p[s];
    if (p <= 0) return;
    const bool two = have2 && need2 && need2[s];
    const uint32_t ch = blockIdx.x % nch;
    const uint32_t k0 = sp_pat_off[s], k1 = sp_pat_off[s + 1];
    const uint32_t r0 = pat_start[k0], r1 = pat_start[k1];              // the species' rows (pat_start[K] = all rows)
    const uint32_t per = (r1 - r0 + nch - 1) / nch;
    uint32_t lo = r0 + ch * per, hi = lo + per;
    if (lo > r1) lo = r1;
    if (hi > r1) hi = r1;
    double acc1 = 0.0, acc2 = 0.0;
    constexpr uint32_t KL = 256;                                          // patterns whose starts and predictions ride in LDS (a species has a handful)
    __shared__ uint32_t s_ps[KL + 1];
    __shared__ double s_p1[KL], s_p2[KL];
    const uint32_t K = k1 - k0;
    if (K <= KL) {                                                        // (block-uniform)
        for (uint32_t q = threadIdx.x; q <= K; q += 256) s_ps[q] = pat_start[k0 + q];
        for (uint32_t q = threadIdx.x; q < K; q += 256) { s_p1[q] = pred1[k0 + q]; s_p2[q] = two ? pred2[k0 + q] : 0.0; }
        __syncthreads();
        uint32_t a = 0;                                                   // last pattern that starts at or before row i: searched for the thread's first row,
        {                                                                 // walked on from there (its rows ascend: round 6 -- a search per row was eight dependent LDS reads)
            const uint32_t i0 = lo + threadIdx.x;
            uint32_t b = K;
            while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (s_ps[m] <= i0) a = m; else b = m; }
        }
        for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
            while (a + 1 < K && s_ps[a + 1] <= i) ++a;
            const double av = row_a[i];
            acc1 += fabs(s_p1[a] - av);
            if (two) acc2 += fabs(s_p2[a] - av);
        }
    } else
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
        uint32_t a = k0, b = k1;
        while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (pat_start[m] <= i) a = m; else b = m; }
        const double av = row_a[i];
        acc1 += fabs(pred1[a] - av);
        if (two) acc2 += fabs(pred2[a] - av);
    }
    acc1 = block_sum_f64<256>(acc1, red);
    acc2 = block_sum_f64<256>(acc2, red);
    if (threadIdx.x == 0) {
        part[((size_t)s * nch + ch) * 2] = acc1;
        part[((size_t)s * nch + ch) * 2 + 1] = acc2;
        s_last = __hip_atomic_fetch_add(&done[s], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nch - 1;
    }
    __syncthreads();
    if (!s_last) return;
    double t1 = 0.0, t2 = 0.0;
    if (threadIdx.x < nch) { t1 = part[((size_t)s * nch + threadIdx.x) * 2]; t2 = part[((size_t)s * nch + threadIdx.x) * 2 + 1]; }
    t1 = block_sum_f64<256>(t1, red);
    t2 = block_sum_f64<256>(t2, red);
    if (threadIdx.x != 0) return;
    obj1[s] = nvalid[s] ? (t1 + c0[s]) / (double)nvalid[s] : 0.0;
    if (two) obj2[s] = nvalid[s] ? (t2 + c0[s]) / (double)nvalid[s] : 0.0;
    done[s] = 0;
}

int objective_launch(Ctx *ctx, const Db *db, LadBatch *lb, const LadRows &rows, const uint8_t *d_need2, const double *d_x1, const double *d_x2, double *d_obj1,
                     double *d_obj2) {
    const uint32_t S = db->S;
    const bool by_nodes = ctx->cfg.objective == "nodes";   // measurements / tests: the pass over the nodes
    if (rows.c0_valid && lb->n_wide == 0 && (!by_nodes || rows.masks_in_sort)) {
        KTimer t(ctx, "objective_rows_kernel");
        PTX_HIP(ctx, lb->d_partial.alloc((size_t)S * STAT_CHUNKS * 4));
        if (lb->d_obj_done.n < S) {
            PTX_HIP(ctx, lb->d_obj_done.alloc(S));
            PTX_HIP(ctx, hipMemsetAsync(lb->d_obj_done.p, 0, lb->d_obj_done.bytes(), ctx->stream));   // the kernel leaves it zero
        }
        const uint32_t nch = stat_chunks(S);
        // (the solver's per-pattern scratch is free again: the predictions of both solutions go there)
        hipLaunchKernelGGL(pattern_pred_kernel, dim3(S), dim3(256), 0, ctx->stream, lb->d_p.p, d_need2, lb->d_sp_pat_off.p, lb->d_pat_mask.p, db->d_hap_off.p, d_x1, d_x2,
                           lb->pat_scratch.sc_s.p, lb->pat_scratch.sc_rho.p);
        hipLaunchKernelGGL(objective_rows_kernel, dim3(S * nch), dim3(256), 0, ctx->stream, lb->d_p.p, d_need2, lb->d_sp_pat_off.p, lb->d_pat_start.p, lb->row_a,
                           (const double *)lb->pat_scratch.sc_s.p, (const double *)lb->pat_scratch.sc_rho.p, (const double *)lb->d_c0.p, lb->d_partial.p, lb->d_obj_done.p, lb->d_nvalid.p,
                           d_obj1, d_obj2, nch, d_x2 != nullptr);
        PTX_HIP(ctx, hipGetLastError());
        return 0;
    }
    if (rows.fused) return fail(ctx, PANTAX_HIP_E_STATE, "objective: internal (the pass over the nodes after a fused node pass: no abundance array)");
    KTimer t(ctx, "objective_kernel");
    PTX_HIP(ctx, lb->d_partial.alloc((size_t)S * STAT_CHUNKS * 4));
    if (lb->d_obj_done.n < S) {
        PTX_HIP(ctx, lb->d_obj_done.alloc(S));
        PTX_HIP(ctx, hipMemsetAsync(lb->d_obj_done.p, 0, lb->d_obj_done.bytes(), ctx->stream));   // the kernel leaves it zero
    }
    const uint32_t nch = stat_chunks(S);
    hipLaunchKernelGGL(objective_kernel, dim3(S * nch), dim3(256), 0, ctx->stream, lb->d_p.p, d_need2, db->d_node_base.p, lb->d_ab.p,
                       (unsigned long long *)lb->d_mask.p, db->d_hap_off.p, lb->d_wide_off.p, lb->d_wide_nw.p, (const unsigned long long *)lb->d_maskw.p, d_x1, d_x2, lb->d_partial.p, lb->d_obj_done.p, lb->d_nvalid.p, d_obj1, d_obj2, nch);
    PTX_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace ptx
