// stage_bootstrap.hip -- bootstrap of the strain fit (pantax_hip_strain_bootstrap, the --strain-bootstrap report): how far the x_h of the L1 fit move when the
// rows of the LP are drawn again.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Bootstrap of the strain fit"): the rows of a species are its nodes with a_v = bases / len > 0 and a non-empty
// mask over the selected haplotypes (column k = position in the species' selection); replicate b repeats row v w_v times, w_v a Poisson(1) weight capped at 16
// from a hash of (seed, sp_key, b, v_local) (bootstrap_weight.hpp), replicate 0 every row once; every replicate is solved as a LAD of its own rows.
//
// Once per call -- boot_front_build below, the front half this stage shares with the leave-one-out test of stage_dropout.hip (boot_front.hpp):
//   boot rows      one chained scan over the nodes: head flag "is a row", the store writes {species, mask, a} and the payload v_local at the prefix (no atomics:
//                  the same rows in the same places every run).  Membership: the two routes of member_plan.hpp (option bootstrap_route); on route 1 the
//                  bits of the node's haplotype word are moved to their columns through a 64-entry table per species;
//   sort           the radix sort of primitives.hpp over (species, mask, a), v_local riding as payload;
//   base patterns  one chained scan over the sorted rows: runs of equal (species, mask).
// Per chunk of replicates (bootstrap_plan.hpp: as many as the cap on expanded rows in flight holds) -- the hot path, items = (replicate, sorted row):
//   weights + scan    ONE chained scan: the load functor hashes the item to its weight, the store writes the exclusive prefix = the first expanded row of the
//                     item.  12 bytes read per item (species word and v_local, from L2 after the chunk's first replicate), 4 written;
//   boot_expand       a wave per 64 items: their prefixes give the wave's stretch of output rows (64 on average, 1 024 at the most); the inclusive ends and
//                     the 64 abundances go to LDS and lane t writes output rows t, t + 64, .. of the stretch, each found by a 6-step search over the
//                     64 ends -- consecutive lanes write consecutive doubles whatever the weights are.  12 bytes per item read (its end 4, its abundance 8), 8 per expanded row written;
//   pattern scan      ONE chained scan over (replicate, base pattern): a pattern whose rows all drew 0 does not exist; the store writes pat_mask / pat_start of
//                     the survivors back to back and every item's prefix;
//   boot_finalize     a wave per (replicate, species): its patterns [sp_pat_off), amax = the largest last row of its patterns, the sum of the weights, sp_p = K_s
//                     where there is something to solve and the rows fit the buffer;
//   solver            lad_solve_kernel<16, 1> / <LAD_MAXP, 1> through lad_args_launch (stage_lad.hip): (replicate, species) is one entry with its own col_off;
//   boot_objective    a workgroup per (replicate, species): a wave per pattern sums |s_k - a| over its rows (lane-strided, one DPP reduction), the pattern sums
//                     are added by thread k mod 256 in ascending k and reduced in fixed shape -- the order is a function of the replicate's rows alone.
// Nothing above depends on which replicates share a chunk, so the outputs are the same bits under every chunking.
#include <algorithm>
#include <cmath>
#include <vector>
#include "common.hpp"
#include "boot_front.hpp"
#include "bootstrap_plan.hpp"
#include "bootstrap_weight.hpp"
#include "lad_args.hpp"
#include "lad_device.hpp"
#include "member_device.hpp"
#include "primitives.hpp"
#include "scan_chained.hpp"

namespace ptx {

namespace {

// ---- the rows of the call
struct BootRowSrc {
    const uint32_t *node_off;   // [S + 1] first global node of every species
    uint32_t S;
    const BootSpecies *tab;
    const uint8_t *bit_col;     // [S][64] route 1: haplotype bit -> column
    const uint32_t *node_len;
    const unsigned long long *bases, *node_haps, *wmask;
    __device__ __forceinline__ bool row(uint64_t v, uint32_t &s, unsigned long long &mask, double &a) const {
        a = (double)(long long)bases[v] / (double)node_len[v];   // the arithmetic of node_cov_stats_kernel
        if (!(a > 0.0)) return false;
        uint32_t lo = 0, hi = S;   // species of v: the last s with node_off[s] <= v (an empty species shares its offset with the next one)
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (node_off[mid] <= v) lo = mid + 1; else hi = mid; }
        s = lo - 1;
        const MemberRow m = tab[s].m;
        mask = 0ull;
        if (m.route == 1u) {
            for (unsigned long long x = node_haps[v] & m.bits; x; x &= x - 1ull) mask |= 1ull << bit_col[(size_t)s * 64 + __builtin_ctzll(x)];
        } else if (m.route == 2u) mask = wmask[member_mask_row(m, (uint32_t)v)];   // K <= 64: one word, bit = column
        return mask != 0ull;
    }
};
struct BootRowLoad {
    BootRowSrc src;
    __device__ __forceinline__ uint32_t operator()(uint64_t v) const { uint32_t s; unsigned long long m; double a; return src.row(v, s, m, a) ? 1u : 0u; }
};
struct BootRowStore {
    BootRowSrc src;
    uint64_t *k0, *k1, *k2;
    uint32_t *vloc;
    __device__ __forceinline__ void operator()(uint64_t v, uint32_t j, uint32_t head) const {
        if (!head) return;
        uint32_t s; unsigned long long m; double a;
        (void)src.row(v, s, m, a);
        k0[j] = s; k1[j] = m; k2[j] = (uint64_t)__double_as_longlong(a);   // positive doubles order like their bit patterns
        vloc[j] = (uint32_t)v - src.node_off[s];
    }
};
// ---- base patterns: runs of equal (species, mask) in the sorted rows
struct BootPatLoad {
    const uint64_t *k0, *k1;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return (i == 0 || k0[i] != k0[i - 1] || k1[i] != k1[i - 1]) ? 1u : 0u; }
};
struct BootPatStore {
    const uint64_t *k0, *k1;
    uint64_t *pat_mask;
    uint32_t *pat_start, *pat_species;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t j, uint32_t head) const {
        if (!head) return;
        pat_mask[j] = k1[i]; pat_start[j] = (uint32_t)i; pat_species[j] = (uint32_t)k0[i];
    }
};
// species -> first base pattern ([S + 1]; entry S = P), and the closing pat_start[P] = N
__global__ void __launch_bounds__(256) boot_sp_pat_off_kernel(uint32_t S, uint32_t P, uint32_t N, const uint32_t *__restrict__ pat_species,
                                                              uint32_t *__restrict__ pat_start, uint32_t *__restrict__ sp_pat_off) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s > S) return;
    uint32_t lo = 0, hi = P;   // first pattern with species >= s
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (pat_species[m] < s) lo = m + 1; else hi = m; }
    sp_pat_off[s] = s == S ? P : lo;
    if (s == S) pat_start[P] = N;
}

// ---- per chunk: item i = (replicate b0 + i / N, sorted row i % N)
struct BootWeightLoad {
    const uint64_t *row_sp;     // [N] species of the sorted row
    const uint32_t *vloc;       // [N]
    const BootSpecies *tab;
    uint32_t N, b0;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
        const uint32_t r = (uint32_t)i % N, b = b0 + (uint32_t)i / N;
        return boot_weight_hashed(tab[row_sp[r]].hash, b, vloc[r]);
    }
};
struct BootWeightStore {
    uint32_t *off;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t j, uint32_t) const { off[i] = j; }
};
// off [n_items + 1] -> out: item i's abundance at the rows [off[i], off[i + 1]); rows at or beyond `cap` are not written (boot_finalize reports them)
__global__ void __launch_bounds__(256) boot_expand_kernel(uint32_t n_items, uint32_t N, const uint32_t *__restrict__ off, const double *__restrict__ base_a,
                                                          double *__restrict__ out, uint32_t cap) {
    __shared__ uint32_t s_end[4][64];
    __shared__ double s_a[4][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n_groups = (n_items + 63u) / 64u;
    for (uint32_t g = blockIdx.x * 4 + wave; g < n_groups; g += gridDim.x * 4) {
        const uint32_t i = g * 64u + lane;
        const bool on = i < n_items;
        const uint32_t last = min(g * 64u + 64u, n_items);
        const uint32_t obase = off[g * 64u], total = off[last] - obase;
        s_end[wave][lane] = on ? off[i + 1] - obase : total;   // (a dead lane ends where the stretch ends: no output row is below its end)
        s_a[wave][lane] = on ? base_a[i % N] : 0.0;
        member_wave_sync();
        for (uint32_t t = lane; t < total; t += 64u) {
            uint32_t lo = 0, hi = 63;   // the first item whose end is beyond t (the last item's end is total > t)
#pragma unroll
            for (int step = 0; step < 6; ++step) { const uint32_t mid = (lo + hi) >> 1; if (s_end[wave][mid] > t) hi = mid; else lo = mid + 1; }
            const uint32_t row = obase + t;
            if (row < cap) out[row] = s_a[wave][lo];
        }
        member_wave_sync();
    }
}
// item i = (local replicate i / P, base pattern i % P): alive when some row of it drew a weight
struct BootLiveLoad {
    const uint32_t *off, *bpat_start;
    uint32_t N, P;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
        const uint32_t k = (uint32_t)i % P, base = ((uint32_t)i / P) * N;
        return off[base + bpat_start[k + 1]] > off[base + bpat_start[k]] ? 1u : 0u;
    }
};
struct BootLiveStore {
    const uint32_t *off, *bpat_start;
    const uint64_t *bpat_mask;
    uint32_t N, P;
    uint32_t *prefix, *pat_start;
    uint64_t *pat_mask;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t j, uint32_t live) const {
        prefix[i] = j;
        if (!live) return;
        const uint32_t k = (uint32_t)i % P, base = ((uint32_t)i / P) * N;
        pat_mask[j] = bpat_mask[k];
        pat_start[j] = off[base + bpat_start[k]];
    }
};
struct BootTables {   // what boot_finalize reads and writes
    const uint32_t *off, *bpat_start, *bsp_pat_off, *prefix, *counts /* {expanded rows, patterns} of the chunk */;
    const double *row_a;
    const uint64_t *sel_off;    // [S + 1]
    uint32_t S, N, P, C, cap;
    uint32_t *pat_start, *sp_pat_off, *flags;
    int32_t *sp_p, *pre;
    double *amax;
    uint64_t *col_off, *rows;
};
__global__ void __launch_bounds__(64) boot_finalize_kernel(BootTables T, uint32_t nq) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint32_t total = T.counts[0];
    const bool overflow = total > T.cap;
    if (q == nq) {   // the closing entries
        if (lane == 0) { const uint32_t K = T.counts[1]; T.sp_pat_off[nq] = K; T.pat_start[K] = total; if (overflow) T.flags[0] = 1u; }
        return;
    }
    const uint32_t bl = q / T.S, s = q % T.S, base = bl * T.N;
    const uint32_t kb0 = T.bsp_pat_off[s], kb1 = T.bsp_pat_off[s + 1];
    double amax = 0.0;
    if (!overflow)
        for (uint32_t k = kb0 + lane; k < kb1; k += 64u) {
            const uint32_t e0 = T.off[base + T.bpat_start[k]], e1 = T.off[base + T.bpat_start[k + 1]];
            if (e1 > e0) amax = fmax(amax, T.row_a[e1 - 1]);   // sorted by a inside the pattern
        }
    amax = wave_reduce(amax, [](double x, double y) { return fmax(x, y); });
    if (lane != 0) return;
    const uint32_t k0 = T.prefix[bl * T.P + kb0], k1 = T.prefix[bl * T.P + kb1];
    const uint64_t K = T.sel_off[s + 1] - T.sel_off[s];
    const bool solve = !overflow && K >= 1 && K <= 64 && k1 > k0;
    T.sp_pat_off[q] = k0;
    T.sp_p[q] = solve ? (int32_t)K : 0;
    T.pre[q] = K > 64 ? PANTAX_HIP_E_LIMIT : (solve ? BOOT_PENDING : 1);
    T.amax[q] = amax;
    T.col_off[q] = (uint64_t)bl * T.C + T.sel_off[s];
    T.rows[q] = (uint64_t)(T.off[base + T.bpat_start[kb1]] - T.off[base + T.bpat_start[kb0]]);
}
// obj[q] = sum over the entry's rows of |m . x - a|
__global__ void __launch_bounds__(256) boot_objective_kernel(const int32_t *__restrict__ sp_p, const uint32_t *__restrict__ sp_pat_off, const uint64_t *__restrict__ pat_mask,
                                                             const uint32_t *__restrict__ pat_start, const double *__restrict__ row_a, const uint64_t *__restrict__ col_off,
                                                             const double *__restrict__ x, double *__restrict__ part /*[patterns]*/, double *__restrict__ obj) {
    __shared__ double xs[LAD_MAXP], red[4];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = sp_p[q];
    if (p <= 0) { if (tid == 0) obj[q] = 0.0; return; }
    if ((int)tid < LAD_MAXP) xs[tid] = (int)tid < p ? x[col_off[q] + tid] : 0.0;
    __syncthreads();
    const uint32_t k0 = sp_pat_off[q], k1 = sp_pat_off[q + 1];
    for (uint32_t k = k0 + wave; k < k1; k += 4u) {
        const double sk = mdot(pat_mask[k], xs);
        double acc = 0.0;
        for (uint32_t r = pat_start[k] + lane, en = pat_start[k + 1]; r < en; r += 64u) acc += fabs(sk - row_a[r]);
        acc = wave_reduce(acc, [](double a, double b) { return a + b; });
        if (lane == 0) part[k] = acc;
    }
    __threadfence_block();
    __syncthreads();
    double t = 0.0;
    for (uint32_t k = k0 + tid; k < k1; k += 256u) t += part[k];
    t = block_sum_f64<256>(t, red);
    if (tid == 0) obj[q] = t;
}

}  // namespace

// the front half of the bootstrap and of the leave-one-out test (boot_front.hpp)
int boot_front_build(Ctx *ctx, Db *db, const unsigned long long *d_bases, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *sp_key, uint64_t seed,
                     const std::string &route_opt, const char *what, const std::function<int(uint64_t)> &sized, BootFront &F) {
    const uint32_t S = db->S;
    const uint64_t V = db->V;
    F.N = 0; F.P = 0; F.k_max = 0;
    if (V >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: %llu nodes exceed 32-bit positions", what, (unsigned long long)V);
    const bool by_node = member_by_node(db->nh_built, route_opt);
    // ---- host tables
    std::vector<BootSpecies> tab(S);
    std::vector<uint8_t> bit_col((size_t)S * 64, 0);
    std::vector<uint32_t> node_off(S + 1);
    F.pre_host.assign(S, 0);   // per species: E_LIMIT, 1 (nothing selected) or pending
    WalkMasks &wm = F.wm;
    uint64_t k_max = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = sel_off[s + 1] - sel_off[s];
        const bool served = K <= 64;
        tab[s].m = wm.row(db, s, by_node, sel_hap + sel_off[s], served ? K : 0);   // a species beyond the limit has no rows
        tab[s].hash = sp_key ? boot_species_hash(seed, sp_key[s]) : 0ull;
        if (tab[s].m.route == 1u) for (uint64_t k = 0; k < K; ++k) bit_col[(size_t)s * 64 + sel_hap[sel_off[s] + k]] = (uint8_t)k;
        if (served) k_max = std::max(k_max, K);
        node_off[s] = (uint32_t)db->h_node_off[s];
        F.pre_host[s] = K > 64 ? PANTAX_HIP_E_LIMIT : (K == 0 ? 1 : BOOT_PENDING);
    }
    node_off[S] = (uint32_t)db->h_node_off[S];
    F.k_max = k_max;
    if (V == 0 || k_max == 0) return 0;
    // ---- rows: {species, mask, a} + v_local, compacted by one scan over the nodes
    PTX_TRY(wm.build(ctx, db));
    PTX_TRY(upload(ctx, F.d_tab, tab.data(), tab.size()));
    PTX_TRY(upload(ctx, F.d_bit_col, bit_col.data(), bit_col.size()));
    PTX_TRY(upload(ctx, F.d_node_off, node_off.data(), node_off.size()));
    PTX_TRY(upload(ctx, F.d_sel_off, sel_off, (size_t)S + 1));
    PTX_HIP(ctx, F.d_counts.alloc(4));
    PTX_HIP(ctx, hipMemsetAsync(F.d_counts.p, 0, 4 * sizeof(uint32_t), ctx->stream));
    for (int w = 0; w < 3; ++w) PTX_HIP(ctx, F.ka[w].alloc(V));
    PTX_HIP(ctx, F.d_va.alloc(V));
    const BootRowSrc src{F.d_node_off.p, S, F.d_tab.p, F.d_bit_col.p, db->d_node_len.p, d_bases,
                         by_node ? (const unsigned long long *)db->d_node_haps.p : (const unsigned long long *)nullptr, wm.d_mask.p};
    PTX_TRY(exclusive_scan_fn(ctx, BootRowLoad{src}, BootRowStore{src, F.ka[0].p, F.ka[1].p, F.ka[2].p, F.d_va.p}, V, F.d_counts.p, "scan_chained_kernel<BootRows>"));
    uint32_t n_rows32 = 0;
    PTX_TRY(download(ctx, &n_rows32, F.d_counts.p, 1));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t N = n_rows32;
    if (N == 0) return 0;
    // ---- the caller's plan, before anything is sized by it
    PTX_TRY(sized(N));
    // ---- sort by (species, mask, a), v_local as payload
    for (int w = 0; w < 3; ++w) PTX_HIP(ctx, F.kb[w].alloc(N));
    PTX_HIP(ctx, F.d_vb.alloc(N));
    PTX_HIP(ctx, F.d_table.alloc(sort_table_elems(N)));
    PTX_HIP(ctx, F.d_scan_tmp.alloc(scan_tmp_elems(std::max<uint64_t>(N, 256ull * 2048))));
    SortBufs A, B;
    A.nw = B.nw = 3;
    for (int w = 0; w < 3; ++w) { A.k[w] = F.ka[w].p; B.k[w] = F.kb[w].p; }
    A.v = F.d_va.p; B.v = F.d_vb.p;
    std::vector<SortPass> passes;
    add_passes(passes, 2, 0, 63);                       // a > 0: sign bit clear
    add_passes(passes, 1, 0, (int)k_max);
    if (S > 1) add_passes(passes, 0, 0, bits_for(S - 1));
    bool in_b = false;
    PTX_TRY(radix_sort(ctx, A, B, N, passes.data(), (int)passes.size(), F.d_table.p, F.d_scan_tmp.p, &in_b));
    const SortBufs &Sd = in_b ? B : A;
    F.row_sp = Sd.k[0]; F.row_mask = Sd.k[1];
    F.base_a = reinterpret_cast<const double *>(Sd.k[2]);
    F.vloc = Sd.v;
    // ---- base patterns
    PTX_HIP(ctx, F.d_bpat_mask.alloc(N)); PTX_HIP(ctx, F.d_bpat_start.alloc(N + 1)); PTX_HIP(ctx, F.d_bpat_species.alloc(N)); PTX_HIP(ctx, F.d_bsp_pat_off.alloc((size_t)S + 1));
    PTX_TRY(exclusive_scan_fn(ctx, BootPatLoad{Sd.k[0], Sd.k[1]}, BootPatStore{Sd.k[0], Sd.k[1], F.d_bpat_mask.p, F.d_bpat_start.p, F.d_bpat_species.p}, N, F.d_counts.p + 1,
                              "scan_chained_kernel<BootPat>"));
    uint32_t P = 0;
    PTX_TRY(download(ctx, &P, F.d_counts.p + 1, 1));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (P == 0 || P > N) return fail(ctx, PANTAX_HIP_E_STATE, "%s: internal (%u patterns of %llu rows)", what, P, (unsigned long long)N);
    hipLaunchKernelGGL(boot_sp_pat_off_kernel, dim3((S + 1 + 255) / 256), dim3(256), 0, ctx->stream, S, P, (uint32_t)N, F.d_bpat_species.p, F.d_bpat_start.p, F.d_bsp_pat_off.p);
    PTX_HIP(ctx, hipGetLastError());
    F.N = N; F.P = P;
    return 0;
}

int boot_objective_launch(Ctx *ctx, uint32_t nq, const int32_t *sp_p, const uint32_t *sp_pat_off, const uint64_t *pat_mask, const uint32_t *pat_start, const double *row_a,
                          const uint64_t *col_off, const double *x, double *part, double *obj, const char *timer_name) {
    if (nq == 0) return 0;
    {
        KTimer tm(ctx, timer_name);
        hipLaunchKernelGGL(boot_objective_kernel, dim3(nq), dim3(256), 0, ctx->stream, sp_p, sp_pat_off, pat_mask, pat_start, row_a, col_off, x, part, obj);
    }
    PTX_HIP(ctx, hipGetLastError());
    return 0;
}

// selection and sp_key validated by the caller
int bootstrap_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *sp_key, uint64_t seed, uint32_t n_replicates, double *x_out,
                     double *obj_out, uint64_t *rows_out, int32_t *status_out) {
    return bootstrap_launch_on(ctx, db, (const unsigned long long *)db->d_bases.p, sel_off, sel_hap, sp_key, seed, n_replicates, ctx->cfg.bootstrap_route, "strain_bootstrap",
                               nullptr, x_out, obj_out, rows_out, status_out);
}

// the same on any per-node bases array of the db's V nodes (boot_front.hpp): the rarefaction's refit of a thinned level is this with n_replicates = 0
int bootstrap_launch_on(Ctx *ctx, Db *db, const unsigned long long *d_bases, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *sp_key, uint64_t seed,
                        uint32_t n_replicates, const std::string &route_opt, const char *what, const std::function<int(const BootFront &)> *front_built, double *x_out,
                        double *obj_out, uint64_t *rows_out, int32_t *status_out) {
    const uint32_t S = db->S;
    const uint64_t C = sel_off[S], V = db->V, R = (uint64_t)n_replicates + 1;
    if (S == 0) return 0;
    if (V >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: %llu nodes exceed 32-bit positions", what, (unsigned long long)V);
    if (R * std::max<uint64_t>(C, S) >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: %llu replicates of %llu selection entries and %u species exceed 32-bit positions", what, (unsigned long long)R, (unsigned long long)C, S);
    // ---- the plan of the chunks, once the rows are counted
    BootstrapPlan plan;
    const auto sized = [&](uint64_t n_rows) {
        uint64_t cap = ctx->cfg.bootstrap_rows_max;
        if (cap == 0) {
            size_t free_b = 0, total_b = 0;
            PTX_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
            cap = bootstrap_default_cap(free_b);
        }
        std::string why;
        if (!bootstrap_plan(n_rows, R, cap, plan, why)) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s", why.c_str());
        return 0;
    };
    // ---- host tables, rows, sort, base patterns (boot_front.hpp)
    BootFront F;
    {
        const int rc = boot_front_build(ctx, db, d_bases, sel_off, sel_hap, sp_key, seed, route_opt, what, sized, F);
        if (rc != 0) return rc;
    }
    if (front_built && F.N) PTX_TRY((*front_built)(F));
    const std::vector<int32_t> &pre_host = F.pre_host;
    // results on the host; the caller's arrays are written at the very end
    std::vector<double> hx((size_t)(R * C)), hobj((size_t)(R * S), 0.0);
    std::vector<uint64_t> hrows((size_t)(R * S), 0);
    std::vector<int32_t> hstatus((size_t)(R * S));
    for (uint64_t b = 0; b < R; ++b) for (uint32_t s = 0; s < S; ++s) hstatus[b * S + s] = pre_host[s] == BOOT_PENDING ? 1 : pre_host[s];
    std::fill(hx.begin(), hx.end(), 0.0);
    const auto deliver = [&]() {
        std::copy(hx.begin(), hx.end(), x_out); std::copy(hobj.begin(), hobj.end(), obj_out);
        std::copy(hrows.begin(), hrows.end(), rows_out); std::copy(hstatus.begin(), hstatus.end(), status_out);
        return 0;
    };
    if (F.N == 0) return deliver();
    const uint64_t N = F.N, k_max = F.k_max;
    const uint32_t P = F.P;
    const uint64_t *row_sp = F.row_sp;
    const double *base_a = F.base_a;
    DevBuf<BootSpecies> &d_tab = F.d_tab;
    DevBuf<uint32_t> &d_counts = F.d_counts, &d_bpat_start = F.d_bpat_start, &d_bsp_pat_off = F.d_bsp_pat_off;
    DevBuf<uint64_t> &d_sel_off = F.d_sel_off, &d_bpat_mask = F.d_bpat_mask;
    // ---- the chunk's scratch, once (DevBuf: the ctx's device cache); nothing is allocated inside the loop
    const uint64_t per = plan.per_chunk, nq_max = per * S, np_max = per * P, ni_max = per * N;
    DevBuf<uint32_t> d_off, d_prefix, d_pat_start, d_sp_pat_off, d_flags;
    DevBuf<uint64_t> d_pat_mask, d_col_off, d_rows;
    DevBuf<double> d_exp_a, d_amax, d_x, d_obj;
    DevBuf<int32_t> d_sp_p, d_pre, d_status, d_iters;
    LadPatScratch pat_scratch;
    PTX_HIP(ctx, d_off.alloc(ni_max + 1)); PTX_HIP(ctx, d_exp_a.alloc(plan.chunk_rows));
    PTX_HIP(ctx, d_prefix.alloc(np_max + 1)); PTX_HIP(ctx, d_pat_start.alloc(np_max + 1)); PTX_HIP(ctx, d_pat_mask.alloc(np_max));
    PTX_HIP(ctx, d_sp_pat_off.alloc(nq_max + 1)); PTX_HIP(ctx, d_flags.alloc(1));
    PTX_HIP(ctx, d_col_off.alloc(nq_max)); PTX_HIP(ctx, d_rows.alloc(nq_max)); PTX_HIP(ctx, d_amax.alloc(nq_max)); PTX_HIP(ctx, d_obj.alloc(nq_max));
    PTX_HIP(ctx, d_sp_p.alloc(nq_max)); PTX_HIP(ctx, d_pre.alloc(nq_max)); PTX_HIP(ctx, d_status.alloc(nq_max)); PTX_HIP(ctx, d_iters.alloc(nq_max));
    PTX_HIP(ctx, d_x.alloc(per * std::max<uint64_t>(C, 1)));
    PTX_TRY(pat_scratch.alloc(ctx, np_max));
    PTX_HIP(ctx, hipMemsetAsync(d_flags.p, 0, sizeof(uint32_t), ctx->stream));
    std::vector<int32_t> c_pre(nq_max), c_status(nq_max);
    uint32_t h_flag = 0;
    const uint32_t cap_rows = (uint32_t)plan.chunk_rows;
    for (uint64_t b0 = 0; b0 < R; b0 += per) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(per, R - b0), n_items = nb * (uint32_t)N, n_pat = nb * P, nq = nb * S;
        // weights -> first expanded row of every item; the total closes the offsets
        PTX_TRY(exclusive_scan_fn(ctx, BootWeightLoad{row_sp, F.vloc, d_tab.p, (uint32_t)N, (uint32_t)b0}, BootWeightStore{d_off.p}, n_items, d_counts.p + 2, "scan_chained_kernel<BootWeights>"));
        PTX_HIP(ctx, hipMemcpyAsync(d_off.p + n_items, d_counts.p + 2, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        {
            KTimer tm(ctx, "boot_expand_kernel");
            hipLaunchKernelGGL(boot_expand_kernel, dim3(grid_for(((uint64_t)n_items + 63) / 64, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_items, (uint32_t)N, d_off.p, base_a, d_exp_a.p, cap_rows);
        }
        // the replicates' pattern tables
        PTX_TRY(exclusive_scan_fn(ctx, BootLiveLoad{d_off.p, d_bpat_start.p, (uint32_t)N, P},
                                  BootLiveStore{d_off.p, d_bpat_start.p, d_bpat_mask.p, (uint32_t)N, P, d_prefix.p, d_pat_start.p, d_pat_mask.p}, n_pat, d_counts.p + 3,
                                  "scan_chained_kernel<BootLive>"));
        PTX_HIP(ctx, hipMemcpyAsync(d_prefix.p + n_pat, d_counts.p + 3, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        BootTables T;
        T.off = d_off.p; T.bpat_start = d_bpat_start.p; T.bsp_pat_off = d_bsp_pat_off.p; T.prefix = d_prefix.p; T.counts = d_counts.p + 2;
        T.row_a = d_exp_a.p; T.sel_off = d_sel_off.p; T.S = S; T.N = (uint32_t)N; T.P = P; T.C = (uint32_t)C; T.cap = cap_rows;
        T.pat_start = d_pat_start.p; T.sp_pat_off = d_sp_pat_off.p; T.flags = d_flags.p; T.sp_p = d_sp_p.p; T.pre = d_pre.p; T.amax = d_amax.p;
        T.col_off = d_col_off.p; T.rows = d_rows.p;
        {
            KTimer tm(ctx, "boot_finalize_kernel");
            hipLaunchKernelGGL(boot_finalize_kernel, dim3(nq + 1), dim3(64), 0, ctx->stream, T, nq);
        }
        PTX_HIP(ctx, hipGetLastError());
        if (C) PTX_HIP(ctx, hipMemsetAsync(d_x.p, 0, (size_t)nb * C * sizeof(double), ctx->stream));
        PTX_HIP(ctx, hipMemsetAsync(d_status.p, 0, (size_t)nq * sizeof(int32_t), ctx->stream));
        const LadArgs LA = lad_plain_args(LadRowTables{d_exp_a.p, d_pat_mask.p, d_pat_start.p, d_sp_pat_off.p}, LadLpTables{d_sp_p.p, d_amax.p, d_col_off.p, nullptr, nullptr},
                                          LadOutputs{d_x.p, d_status.p, d_iters.p}, pat_scratch);
        PTX_TRY(lad_args_launch(ctx, LA, nq, (int)k_max, "lad_solve_kernel<bootstrap>"));
        PTX_TRY(boot_objective_launch(ctx, nq, d_sp_p.p, d_sp_pat_off.p, d_pat_mask.p, d_pat_start.p, d_exp_a.p, d_col_off.p, d_x.p, pat_scratch.sc_s.p, d_obj.p, "boot_objective_kernel"));
        if (C) PTX_TRY(download(ctx, hx.data() + b0 * C, d_x.p, (size_t)nb * C));
        PTX_TRY(download(ctx, hobj.data() + b0 * S, d_obj.p, (size_t)nq));
        PTX_TRY(download(ctx, (unsigned long long *)hrows.data() + b0 * S, (const unsigned long long *)d_rows.p, (size_t)nq));
        PTX_TRY(download(ctx, c_pre.data(), d_pre.p, (size_t)nq));
        PTX_TRY(download(ctx, c_status.data(), d_status.p, (size_t)nq));
        PTX_TRY(download(ctx, &h_flag, d_flags.p, 1));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (h_flag)
            return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: the replicates %llu .. %llu drew more than the %u expanded rows their chunk is sized for (bootstrap_plan.hpp)", what,
                        (unsigned long long)b0, (unsigned long long)(b0 + nb - 1), cap_rows);
        for (uint32_t q = 0; q < nq; ++q)
            hstatus[b0 * S + q] = c_pre[q] != BOOT_PENDING ? c_pre[q] : (c_status[q] == 0 ? 0 : PANTAX_HIP_E_SOLVER);
    }
    return deliver();
}

}  // namespace ptx
