// stage_lp_rows.hip -- a10 on device: candidate-path membership masks + path_cov_ratio, the node -> haplotype words built at upload, and the
// LP rows: which route they take (row_route), their emission / sort and the pattern tables (lad_prepare).
#include <algorithm>
#include <cstdio>
#include <vector>
#include "lad.hpp"
#include "lad_device.hpp"
#include "cov_plan.hpp"
#include "primitives.hpp"
#include "wave.hpp"
#include "scan_chained.hpp"

namespace ptx {

// ---------------------------------------------------------------------------------------------
// a10: membership masks (the 0/1 coefficient matrix, one u64 row per node) and path_cov_ratio
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t find_hap_l(const uint64_t *__restrict__ path_off, uint32_t H, uint64_t q) {
    uint32_t lo = 0, hi = H;
    while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (path_off[mid] <= q) lo = mid + 1; else hi = mid; }
    return lo - 1;
}

__global__ void __launch_bounds__(256) mask_kernel(const uint2 *__restrict__ tiles, const uint64_t *__restrict__ path_off,
                                                   const uint32_t *__restrict__ path_nodes, const uint32_t *__restrict__ hap_species,
                                                   const uint32_t *__restrict__ node_base, const int32_t *__restrict__ hap_bit,
                                                   unsigned long long *__restrict__ mask, const int32_t *__restrict__ sp_p,
                                                   const uint32_t *__restrict__ wide_off /* null: no species can be wide */,
                                                   const uint32_t *__restrict__ wide_nw, unsigned long long *__restrict__ maskw,
                                                   const uint64_t *__restrict__ by_node_hap_off /* non-null: species of <= 64 haplotypes were done by mask_nodes_kernel */) {
    const uint2 tile = tiles[blockIdx.x];   // {hap, chunk}: see trio_device.hpp
    if (tile.x == 0xFFFFFFFFu) return;      // filler tile
    const uint32_t h = tile.x;
    const int bit = hap_bit[h];
    if (bit < 0) return;
    const uint32_t sp = hap_species[h];
    const uint32_t nb = node_base[sp];
    const uint64_t q0 = path_off[h] + (uint64_t)tile.y * PATH_TILE, qend = path_off[h + 1];
    if (wide_off && sp_p[sp] > LAD_MAXP) {   // wide species: wide_nw[sp] (LAD_WIDE_NW or more) words per node in the side array
        const unsigned long long m = 1ull << (bit & 63);
        const size_t nw = wide_nw[sp];
        unsigned long long *base = maskw + (size_t)wide_off[sp] * LAD_WIDE_NW + (bit >> 6);
        for (uint64_t q = q0 + threadIdx.x; q < q0 + PATH_TILE && q < qend; q += 256) {
            unsigned long long *w = base + (size_t)path_nodes[q] * nw;
            if ((*w & m) == 0) atomicOr(w, m);
        }
        return;
    }
    if (by_node_hap_off && by_node_hap_off[sp + 1] - by_node_hap_off[sp] <= 64ull) return;
    const unsigned long long m = 1ull << bit;
    for (uint64_t q = q0 + threadIdx.x; q < q0 + PATH_TILE && q < qend; q += 256) {
        unsigned long long *w = &mask[nb + path_nodes[q]];
        if ((*w & m) == 0) atomicOr(w, m);   // coeff_matrix[(v,pos)] = 1.0 even for repeated visits (profile.rs:1336-1340)
    }
}

// ---- the same matrix built BY NODE (round 3).  mask_kernel walks the candidates' paths and ORs a bit into the word of every
// node it meets: 2.2e9 path steps at cfg4, a read-test-atomic on a 2.5-GB array each, 9 ms of a 58-ms step at 0.8 TB/s.  Which
// haplotypes of its species visit a node depends on the database alone: node_haps_build writes that set once at upload as one
// 64-bit word per node (bit j = haplotype j of the species; a layout table like d_tiles and the node-block runs), and the step
// turns it into the candidates' word in registers -- one coalesced 8-byte load, a lookup in the species' haplotype -> column
// table per set bit, one 8-byte store, zero words included: no atomics, no zero fill, every byte touched once.
// Species of more than 64 haplotypes keep the path walk (their nodes get a zero here first).
__global__ void __launch_bounds__(256) node_haps_fill_kernel(const uint2 *__restrict__ tiles, const uint64_t *__restrict__ path_off,
                                                             const uint32_t *__restrict__ path_nodes, const uint32_t *__restrict__ hap_species,
                                                             const uint32_t *__restrict__ node_base, const uint64_t *__restrict__ hap_off,
                                                             unsigned long long *__restrict__ node_haps, uint32_t fast, const uint32_t *__restrict__ fast_slow) {
    const uint2 tile = tiles[blockIdx.x];
    if (tile.x == 0xFFFFFFFFu) return;
    const uint32_t h = tile.x, sp = hap_species[h], nb = node_base[sp];
    if (hap_off[sp + 1] - hap_off[sp] > 64ull) return;
    if (fast && !fast_slow[sp]) return;                     // a species of the visit table: node_haps_visits_kernel
    const unsigned long long m = 1ull << (h - hap_off[sp]);
    const uint64_t q0 = path_off[h] + (uint64_t)tile.y * PATH_TILE, qend = path_off[h + 1];
    for (uint64_t q = q0 + threadIdx.x; q < q0 + PATH_TILE && q < qend; q += 256) {
        unsigned long long *w = &node_haps[nb + path_nodes[q]];
        if ((*w & m) == 0) atomicOr(w, m);
    }
}
__global__ void __launch_bounds__(256) mask_nodes_kernel(uint64_t V, const uint2 *__restrict__ tile_sp, const uint32_t *__restrict__ node_base,
                                                         const uint64_t *__restrict__ hap_off, const int32_t *__restrict__ sp_p,
                                                         const int32_t *__restrict__ hap_bit, const unsigned long long *__restrict__ node_haps,
                                                         unsigned long long *__restrict__ mask, const uint32_t *__restrict__ cov,
                                                         const uint32_t *__restrict__ node_len, unsigned long long *__restrict__ ratio) {
    // one workgroup per 2048-node tile of d_emit_tile_sp (eight nodes per thread: the table below is set up once per 2048 nodes)
    // ratio != null: the path_cov_ratio sums of ratio_kernel (profile.rs:1344-1361) for every species this kernel builds the masks of,
    // taken while the mask is in a register -- ratio_kernel's 8V bytes of masks are not read a second time
    __shared__ int s_bit[64];     // haplotype -> LP column of the species the tile starts in (nearly always its only one)
    // ... and the same map BYTE-WISE: s_tab[b][x] = the columns of the haplotypes 8b .. 8b+7 whose bits are set in x.  A node's mask is the OR
    // of one entry per byte of its haplotype word (two lookups at ten haplotypes) instead of a loop over its set bits (the kernel was
    // bound by VALU issue: 205 instructions per 64 nodes, `r04_pmc_cfg4.json`); building 256 entries per used byte costs a thread one entry
    __shared__ unsigned long long s_tab[8][256];
    __shared__ unsigned long long acc[2 * LAD_MAXP];
    if (ratio && threadIdx.x < 2 * LAD_MAXP) acc[threadIdx.x] = 0;
    unsigned long long c8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, l8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t v0 = (uint64_t)blockIdx.x * 2048;
    const uint2 t = tile_sp[blockIdx.x];
    const uint32_t sp0 = t.x;
    {
        const uint64_t h0 = hap_off[sp0], nh = hap_off[sp0 + 1] - h0;
        if (threadIdx.x < 64) s_bit[threadIdx.x] = threadIdx.x < nh ? hap_bit[h0 + threadIdx.x] : -1;
    }
    const int p0 = sp_p[sp0];
    const uint64_t end0 = sp0 < t.y ? (uint64_t)node_base[sp0 + 1] : V;     // first node that is not of the tile's first species any more
    const int nbyte = (int)((hap_off[sp0 + 1] - hap_off[sp0] + 7) / 8);     // bytes of the haplotype word in use (block-uniform; > 8: a species the path walk fills)
    __syncthreads();
    if (p0 > 0 && p0 <= LAD_MAXP && nbyte <= 8) {
        for (int b = 0; b < nbyte; ++b) {
            unsigned long long e = 0ull;
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int bit = s_bit[8 * b + i]; if (((threadIdx.x >> i) & 1u) && bit >= 0) e |= 1ull << bit; }
            s_tab[b][threadIdx.x] = e;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint64_t v = v0 + (uint64_t)r * 256 + threadIdx.x;
        if (v >= V) break;
        unsigned long long hm = node_haps[v];      // (zero for species of more than 64 haplotypes: the path walk fills those)
        const unsigned long long c = ratio ? cov[v] : 0ull, l = ratio ? node_len[v] : 0ull;
        unsigned long long m = 0ull;
        if (v < end0) {
            if (p0 > 0 && p0 <= LAD_MAXP && nbyte <= 8)
                for (int b = 0; b < nbyte; ++b) m |= s_tab[b][(hm >> (8 * b)) & 255ull];
            if (ratio && m) {                      // the first eight candidates (nearly always all) in registers, like ratio_kernel
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < p0) { const bool on = (m >> k) & 1ull; c8[k] += on ? c : 0ull; l8[k] += on ? l : 0ull; }   // (block-uniform: the columns that exist)
                unsigned long long rest = m >> 8;
                while (rest) {
                    const int k = __ffsll((long long)rest) - 1 + 8;
                    rest &= rest - 1;
                    if (c) atomicAdd(&acc[2 * k], c);
                    atomicAdd(&acc[2 * k + 1], l);
                }
            }
        } else {                                    // a species border inside the tile: the few nodes behind it look their species up
            uint32_t sp = sp0 + 1;
            while (sp < t.y && node_base[sp + 1] <= v) ++sp;
            const int p = sp_p[sp];
            if (p > 0 && p <= LAD_MAXP) {
                const int32_t *hb = hap_bit + hap_off[sp];
                while (hm) { const int j = __ffsll((long long)hm) - 1; hm &= hm - 1; const int bit = hb[j]; if (bit >= 0) m |= 1ull << bit; }
                unsigned long long rest = ratio ? m : 0ull;
                while (rest) {
                    const int k = __ffsll((long long)rest) - 1;
                    rest &= rest - 1;
                    if (c) atomicAdd(&ratio[2 * (hap_off[sp] + k)], c);
                    atomicAdd(&ratio[2 * (hap_off[sp] + k) + 1], l);
                }
            }
        }
        mask[v] = m;      // coeff_matrix[(v,pos)] = 1.0 for every candidate path that visits v (profile.rs:1336-1340)
    }
    if (!ratio || p0 <= 0 || p0 > LAD_MAXP) return;            // (block-uniform)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= p0) break;
        const unsigned long long cs = wave_reduce(c8[k], [](unsigned long long x, unsigned long long y) { return x + y; });
        const unsigned long long ls = wave_reduce(l8[k], [](unsigned long long x, unsigned long long y) { return x + y; });
        if ((threadIdx.x & 63) == 0) {
            if (cs) atomicAdd(&acc[2 * k], cs);
            if (ls) atomicAdd(&acc[2 * k + 1], ls);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * p0 && acc[threadIdx.x]) atomicAdd(&ratio[2 * hap_off[sp0] + threadIdx.x], acc[threadIdx.x]);
}

// Wide species: the one-word "mask" of a node becomes a 64-bit hash of its mask words (0 stays 0), so that the row grouping
// (sort by mask, runs of equal masks = patterns) works on it unchanged.  Equal hashes of different word sets are caught by
// wide_pattern_kernel / the solver (status 7), never silently merged.
constexpr int WIDE_CHUNKS = 64;
__device__ __forceinline__ unsigned long long wide_hash(const unsigned long long *w, int nw) {
    unsigned long long h = 0, any = 0;
    for (int i = 0; i < nw; ++i) { any |= w[i]; h = splitmix64(h ^ (w[i] + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1))); }
    return any ? (h ? h : 1ull) : 0ull;
}
__global__ void __launch_bounds__(256) mask_fold_kernel(const uint32_t *__restrict__ wide_list, const uint32_t *__restrict__ wide_off,
                                                        const uint32_t *__restrict__ wide_nw, const uint32_t *__restrict__ node_base, const int32_t *__restrict__ sp_p,
                                                        const unsigned long long *__restrict__ maskw, unsigned long long *__restrict__ mask) {
    const uint32_t s = wide_list[blockIdx.x / WIDE_CHUNKS], ch = blockIdx.x % WIDE_CHUNKS;
    if (sp_p[s] <= LAD_MAXP) return;
    const uint32_t b = node_base[s], n = node_base[s + 1] - b;
    const unsigned long long *mw = maskw + (size_t)wide_off[s] * LAD_WIDE_NW;
    const int nw = (int)wide_nw[s];
    for (uint32_t v = ch * 256 + threadIdx.x; v < n; v += WIDE_CHUNKS * 256) mask[b + v] = wide_hash(mw + (size_t)v * nw, nw);
}

// Wide species, after the patterns are known: every LP row's node finds its pattern (binary search of its hash among the
// species' patterns, which are sorted by it) and ORs / ANDs its mask words into the pattern's slots.  OR == AND for every
// pattern <=> all of its rows have the same words (the solver checks and reports status 7 otherwise).
__global__ void __launch_bounds__(256) wide_pattern_kernel(const uint32_t *__restrict__ wide_list, const uint32_t *__restrict__ wide_off,
                                                           const uint32_t *__restrict__ wide_nw, const uint32_t *__restrict__ node_base, const int32_t *__restrict__ sp_p,
                                                           const double *__restrict__ ab, const unsigned long long *__restrict__ mask,
                                                           const unsigned long long *__restrict__ maskw, const uint32_t *__restrict__ sp_pat_off,
                                                           const uint64_t *__restrict__ pat_mask, unsigned long long *__restrict__ pat_or,
                                                           unsigned long long *__restrict__ pat_and) {
    const uint32_t s = wide_list[blockIdx.x / WIDE_CHUNKS], ch = blockIdx.x % WIDE_CHUNKS;
    if (sp_p[s] <= LAD_MAXP) return;
    const uint32_t b = node_base[s], n = node_base[s + 1] - b;
    const uint32_t k0 = sp_pat_off[s], k1 = sp_pat_off[s + 1];
    const size_t wo = (size_t)wide_off[s] * LAD_WIDE_NW, nw = wide_nw[s];
    for (uint32_t v = ch * 256 + threadIdx.x; v < n; v += WIDE_CHUNKS * 256) {
        const unsigned long long hm = mask[b + v];
        if (!(ab[b + v] > 0.0) || hm == 0ull) continue;
        uint32_t lo = k0, hi = k1;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (pat_mask[mid] < hm) lo = mid + 1; else hi = mid; }
        if (lo >= k1 || pat_mask[lo] != hm) continue;   // cannot happen: every such node is a row
        for (size_t i = 0; i < nw; ++i) {
            const unsigned long long w = maskw[wo + (size_t)v * nw + i];
            atomicOr(&pat_or[wo + (size_t)(lo - k0) * nw + i], w);
            atomicAnd(&pat_and[wo + (size_t)(lo - k0) * nw + i], w);
        }
    }
}

constexpr int RATIO_CHUNKS = 128;
constexpr int ROW_ITEMS = 8;   // nodes per thread of the row compaction kernels
// path_cov_ratio sums (profile.rs:1344-1361): per candidate k, sum of covered bases and of lengths over its
// nodes.  The first 8 candidates (nearly always all of them) accumulate in registers and are combined by wave
// reductions; 64 lanes hammering 2-4 LDS addresses with 64-bit atomics serialise.
__global__ void __launch_bounds__(256) ratio_kernel(const uint32_t *__restrict__ node_base, const uint32_t *__restrict__ node_len,
                                                    const uint32_t *__restrict__ cov, const unsigned long long *__restrict__ mask,
                                                    const int32_t *__restrict__ sp_p, const uint64_t *__restrict__ hap_off,
                                                    const uint32_t *__restrict__ wide_off, const uint32_t *__restrict__ wide_nw,
                                                    const unsigned long long *__restrict__ maskw, unsigned long long *__restrict__ ratio,
                                                    int by_node_done /* the species of at most 64 haplotypes got their sums from mask_nodes_kernel */) {
    __shared__ unsigned long long acc[LAD_WIDEP * 2];
    const uint32_t s = blockIdx.x / RATIO_CHUNKS, ch = blockIdx.x % RATIO_CHUNKS;
    const int p = sp_p[s];
    if (p <= 0) return;
    if (by_node_done && hap_off[s + 1] - hap_off[s] <= 64) return;
    const uint32_t b = node_base[s], e = node_base[s + 1];
    const uint32_t per = (e - b + RATIO_CHUNKS - 1) / RATIO_CHUNKS;
    uint32_t lo = b + ch * per, hi = lo + per;
    if (hi > e) hi = e;
    if (p > LAD_MAXP) {   // wide species: the candidates through the LDS accumulators, LAD_WIDEP (four mask words) at a time
        const unsigned long long *mw = maskw + (size_t)wide_off[s] * LAD_WIDE_NW;
        const size_t nw = wide_nw[s];
        for (int kb = 0; kb < p; kb += LAD_WIDEP) {
            const int pn = p - kb < LAD_WIDEP ? p - kb : LAD_WIDEP;
            __syncthreads();
            for (int i = threadIdx.x; i < 2 * pn; i += 256) acc[i] = 0;
            __syncthreads();
            for (uint32_t v = lo + threadIdx.x; v < hi; v += 256) {
                const unsigned long long c = cov[v], l = node_len[v];
#pragma unroll
                for (int i = 0; i < LAD_WIDE_NW; ++i) {
                    unsigned long long m = mw[(size_t)(v - b) * nw + (kb >> 6) + i];
                    while (m) {
                        const int k = 64 * i + __ffsll((long long)m) - 1;
                        m &= m - 1;
                        if (c) atomicAdd(&acc[2 * k], c);
                        atomicAdd(&acc[2 * k + 1], l);
                    }
                }
            }
            __syncthreads();
            for (int i = threadIdx.x; i < 2 * pn; i += 256) if (acc[i]) atomicAdd(&ratio[2 * (hap_off[s] + kb) + i], acc[i]);
        }
        return;
    }
    for (int i = threadIdx.x; i < 2 * p; i += 256) acc[i] = 0;
    __syncthreads();
    unsigned long long c8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, l8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t v = lo + threadIdx.x; v < hi; v += 256) {
        unsigned long long m = mask[v];
        if (!m) continue;
        const unsigned long long c = cov[v], l = node_len[v];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool on = (m >> k) & 1ull;
            c8[k] += on ? c : 0ull;
            l8[k] += on ? l : 0ull;
        }
        m >>= 8;
        while (m) {
            int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            if (c) atomicAdd(&acc[2 * (k + 8)], c);
            atomicAdd(&acc[2 * (k + 8) + 1], l);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned long long cs = wave_reduce(c8[k], [](unsigned long long x, unsigned long long y) { return x + y; });
        const unsigned long long ls = wave_reduce(l8[k], [](unsigned long long x, unsigned long long y) { return x + y; });
        if ((threadIdx.x & 63) == 0) {
            if (cs) atomicAdd(&acc[2 * k], cs);
            if (ls) atomicAdd(&acc[2 * k + 1], ls);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * p && acc[threadIdx.x]) atomicAdd(&ratio[2 * hap_off[s] + threadIdx.x], acc[threadIdx.x]);
}


// ---------------------------------------------------------------------------------------------
// LP rows: nodes with a_v > 0 (valid rows, profile.rs:1380-1385) and a non-empty mask; rows with an
// empty mask only add the constant a_v to the objective and are handled by objective_kernel.
// ---------------------------------------------------------------------------------------------
// One launch: every workgroup compacts its tile of nodes and claims its output range with a single atomic
// on the row counter.  Row order across workgroups is arbitrary, which is immaterial: the rows are sorted by
// their full key (species, mask, a) next, and rows with equal keys are indistinguishable.
__global__ void __launch_bounds__(256) row_emit_kernel(uint64_t V, uint32_t S, const uint32_t *__restrict__ node_base, const double *__restrict__ ab,
                                                       const unsigned long long *__restrict__ mask, uint32_t *__restrict__ n_rows,
                                                       uint64_t *__restrict__ k0, uint64_t *__restrict__ k1, uint64_t *__restrict__ k2,
                                                       int pack_shift /* >= 0: two-word rows {species << shift | mask, a} in k0, k1 */) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_base;
    const uint64_t base = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * ROW_ITEMS;
    double a[ROW_ITEMS];
    unsigned long long m[ROW_ITEMS];
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < ROW_ITEMS; ++i) {
        const uint64_t v = base + i;
        a[i] = 0.0; m[i] = 0;
        if (v < V) { a[i] = ab[v]; m[i] = mask[v]; }
        cnt += (a[i] > 0.0 && m[i] != 0ull) ? 1u : 0u;
    }
    // exclusive offsets inside the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { uint32_t t = __shfl_up(incl, d); if (lane >= d) incl += t; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { uint32_t t = s_wave[w]; if (w < wave) woff += t; tot += t; }
    if (threadIdx.x == 0) s_base = tot ? atomicAdd(n_rows, tot) : 0u;
    __syncthreads();
    uint32_t j = s_base + woff + incl - cnt;
    uint32_t sp1 = 0;              // 1 + species of the previous emitted node of this thread (its nodes are consecutive)
#pragma unroll
    for (int i = 0; i < ROW_ITEMS; ++i) {
        if (!(a[i] > 0.0 && m[i] != 0ull)) continue;
        const uint64_t v = base + i;
        uint32_t lo;
        if (sp1 == 0) {            // species of node v: last s with node_base[s] <= v
            uint32_t hi = S;
            lo = 0;
            while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (node_base[mid] <= v) lo = mid + 1; else hi = mid; }
        } else {
            lo = sp1;
            while (lo < S && node_base[lo] <= v) ++lo;   // at most a species border or two between neighbouring nodes
        }
        sp1 = lo;
        const uint64_t abits = (uint64_t)__double_as_longlong(a[i]);   // positive doubles order like their bit patterns
        if (pack_shift >= 0) {
            k0[j] = (pack_shift < 64 ? ((uint64_t)(lo - 1) << pack_shift) : 0ull) | m[i];
            k1[j] = abits;
        } else {
            k0[j] = lo - 1;
            k1[j] = m[i];
            k2[j] = abits;
        }
        ++j;
    }
}
// Patterns = runs of equal (species, mask) in the sorted rows.  One chained-scan launch: the head flag of a row is
// computed from the keys as it is loaded, and a head whose exclusive prefix is j emits pattern j on the spot.
struct PatLoad {
    const uint32_t *d_n;
    const uint64_t *k0, *k1;   // k1 == null: species and mask share k0
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
        const uint64_t n = *d_n;   // rows actually present (the scan covers the host-side bound)
        return (i < n && (i == 0 || k0[i] != k0[i - 1] || (k1 && k1[i] != k1[i - 1]))) ? 1u : 0u;
    }
};
struct PatStore {
    const uint64_t *k0, *k1;
    uint32_t k_cap;
    int pack_shift;
    uint64_t *pat_mask;
    uint32_t *pat_start, *pat_species, *overflow;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t j, uint32_t head) const {
        if (!head) return;
        if (j >= k_cap) { *overflow = 1; return; }   // more patterns than this build sizes for: reported as PANTAX_HIP_E_LIMIT
        if (pack_shift >= 0) {
            const uint64_t w = k0[i];
            pat_mask[j] = pack_shift < 64 ? (w & ((1ull << pack_shift) - 1ull)) : w;
            pat_species[j] = pack_shift < 64 ? (uint32_t)(w >> pack_shift) : 0u;
        } else {
            pat_mask[j] = k1[i];
            pat_species[j] = (uint32_t)k0[i];
        }
        pat_start[j] = (uint32_t)i;
    }
};

// species -> first pattern (patterns are sorted by species); entry S = K; also closes pat_start[K] = n_rows
__global__ void __launch_bounds__(256) sp_pat_off_kernel(uint32_t S, const uint32_t *__restrict__ d_K, uint32_t k_cap,
                                                         const uint32_t *__restrict__ pat_species, const uint32_t *__restrict__ d_n,
                                                         uint32_t *__restrict__ pat_start, uint32_t *__restrict__ sp_pat_off) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s > S) return;
    const uint32_t K = min(*d_K, k_cap), n_rows = *d_n;
    uint32_t lo = 0, hi = K;   // first pattern with species >= s
    while (lo < hi) { uint32_t m = (lo + hi) >> 1; if (pat_species[m] < s) lo = m + 1; else hi = m; }
    sp_pat_off[s] = (s == S) ? K : lo;
    if (s == S) pat_start[K] = n_rows;
}

// option mask=walk: the path-walk kernel although the table exists (measurements, tests)
// ... from the VISIT TABLE where a species has one (round 5): the interior visits of a node sit in one stretch of one 64-lane group, so the word of a node
// is the OR over its stretch of (1 << owner of the visit's position) -- one wave per group, the owners from the species' walk offsets held one per lane
// (as in the filing of the index rows), one ballot per haplotype of the species, one plain 8-byte store per node; the two END positions of every walk
// are no interior visits and come in by atomics afterwards (node_haps_ends_kernel).  The pass over the walks above issued a probe + an atomic per path
// step: 21 ms at 1e4 strains, 50-62 ms per db of 2.8e9 path steps at fifty strains per species.
__global__ void __launch_bounds__(256) node_haps_visits_kernel(uint32_t NG, const uint32_t *__restrict__ vis_pos, const uint64_t *__restrict__ vis_head,
                                                               const uint32_t *__restrict__ vis_nbase, const uint32_t *__restrict__ vis_sp,
                                                               const uint64_t *__restrict__ path_off, const uint64_t *__restrict__ hap_off,
                                                               const uint32_t *__restrict__ path_nodes, const uint32_t *__restrict__ by_walk,
                                                               unsigned long long *__restrict__ node_haps) {
    const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= NG) return;
    if (by_walk[vis_sp[g]]) return;                        // (wave-uniform) a species of many haplotypes: the pass over its walks is cheaper
    const int lane = threadIdx.x & 63;
    const uint32_t q = vis_pos[(uint64_t)g * 64 + lane];
    const bool valid = q != 0xFFFFFFFFu;
    const uint32_t sp = vis_sp[g], nb = vis_nbase[g];
    const uint32_t h0 = (uint32_t)hap_off[sp], hs = (uint32_t)hap_off[sp + 1] - h0;
    const unsigned long long vmask = __builtin_amdgcn_ballot_w64(valid), hd = vis_head[g] & vmask;
    const uint32_t woff = (uint32_t)lane < hs ? (uint32_t)path_off[h0 + (uint32_t)lane] : 0xFFFFFFFFu;     // P < 2^32 where a visit table exists
    uint32_t hl = 0;                                                                     // owner within the species: walk offsets at or below the position, minus one
    for (uint32_t j = 1; j < hs; ++j) hl += (uint32_t)__builtin_amdgcn_readlane((int)woff, (int)j) <= q ? 1u : 0u;
    const bool head = (hd >> lane) & 1ull;
    const uint32_t mid = head ? path_nodes[q] : 0u;                                      // the stretch's node (its first visit names it)
    // my stretch = lanes [lane, next head or first pad)
    const unsigned long long he = hd | (~vmask & (vmask + 1ull));
    const unsigned long long above = he & ~((2ull << lane) - 1ull);
    const int end = above ? __builtin_ctzll(above) : 64;
    const unsigned long long range = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
    unsigned long long word = 0ull;
    for (uint32_t j = 0; j < hs; ++j) {
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(valid && hl == j);
        if (bal & range) word |= 1ull << j;
    }
    if (head) node_haps[nb + mid] = word;
}
// the first and the last position of every walk of a visit-table species (a walk of one or two positions has no interior visit at all)
__global__ void __launch_bounds__(256) node_haps_ends_kernel(uint32_t H, const uint64_t *__restrict__ path_off, const uint32_t *__restrict__ path_nodes,
                                                             const uint32_t *__restrict__ hap_species, const uint32_t *__restrict__ node_base,
                                                             const uint64_t *__restrict__ hap_off, const uint32_t *__restrict__ slow,
                                                             unsigned long long *__restrict__ node_haps) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    const uint32_t sp = hap_species[h];
    if (slow[sp]) return;                                  // (slow = the species' words come from the pass over its walks)
    const uint64_t b = path_off[h], e = path_off[h + 1];
    if (e == b) return;
    const unsigned long long m = 1ull << (h - hap_off[sp]);
    atomicOr(&node_haps[node_base[sp] + path_nodes[b]], m);
    atomicOr(&node_haps[node_base[sp] + path_nodes[e - 1]], m);
}
bool use_node_haps(const Ctx *ctx, const Db *db) { return db->nh_built && ctx->cfg.mask != "walk"; }
// end of db upload: the node -> haplotypes words of mask_nodes_kernel (one launch over the path tiles)
int node_haps_build(Ctx *ctx, Db *db) {
    db->nh_built = false; db->nh_walk_too = false;
    const uint64_t V = db->V;
    if (!V || !db->P || !db->n_tiles) return 0;
    bool any_small = false;
    for (uint32_t s = 0; s < db->S; ++s) {
        if (db->h_hap_off[s + 1] - db->h_hap_off[s] > 64) db->nh_walk_too = true; else any_small = true;
    }
    if (!any_small) return 0;
    PTX_HIP(ctx, db->d_node_haps.alloc(V));
    PTX_TRY(zero_fill(ctx, db->d_node_haps.p, V * sizeof(uint64_t)));
    // the species of the visit table with up to NH_VISIT_HAPS haplotypes from the table, the others by the pass over their walks (the table kernel costs a
    // readlane + a ballot per haplotype of the species and group: at fifty haplotypes 78 ms per db of 2.8e9 path steps against 50 for the walks' atomics;
    // at ten: ms against tens of ms)
    constexpr uint64_t NH_VISIT_HAPS = 16;
    const bool table = db->trio_visit_ok && db->n_vgroups && db->P < 0xFFFFFFFFull;
    std::vector<uint32_t> by_walk(db->S ? db->S : 1, 1u);
    bool any_walk = false, any_visits = false;
    for (uint32_t s = 0; s < db->S; ++s) {
        const uint64_t hs = db->h_hap_off[s + 1] - db->h_hap_off[s];
        by_walk[s] = (table && !db->h_trio_slow[s] && hs <= NH_VISIT_HAPS) ? 0u : 1u;
        if (hs <= 64) { if (by_walk[s]) any_walk = true; else any_visits = true; }
    }
    DevBuf<uint32_t> d_by_walk;
    PTX_TRY(upload(ctx, d_by_walk, by_walk.data(), by_walk.size()));
    if (any_visits) {
        hipLaunchKernelGGL(node_haps_visits_kernel, dim3((db->n_vgroups + 3) / 4), dim3(256), 0, ctx->stream, db->n_vgroups, db->d_vis_pos.p, db->d_vis_head.p, db->d_vis_nbase.p,
                           db->d_vis_sp.p, db->d_path_off.p, db->d_hap_off.p, db->d_path_nodes.p, (const uint32_t *)d_by_walk.p, (unsigned long long *)db->d_node_haps.p);
        hipLaunchKernelGGL(node_haps_ends_kernel, dim3((uint32_t)((db->H + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t)db->H, db->d_path_off.p, db->d_path_nodes.p,
                           db->d_hap_species.p, db->d_node_base.p, db->d_hap_off.p, (const uint32_t *)d_by_walk.p, (unsigned long long *)db->d_node_haps.p);
    }
    if (any_walk)
        hipLaunchKernelGGL(node_haps_fill_kernel, dim3((uint32_t)db->n_tiles), dim3(256), 0, ctx->stream, db->d_tiles.p, db->d_path_off.p, db->d_path_nodes.p,
                           db->d_hap_species.p, db->d_node_base.p, db->d_hap_off.p, (unsigned long long *)db->d_node_haps.p, 1u, (const uint32_t *)d_by_walk.p);
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // d_by_walk goes out of scope
    PTX_HIP(ctx, hipGetLastError());
    db->nh_built = true;
    return 0;
}

// Which route the LP rows of this db take under the ctx's options.  Everything here is known on the host before the step; nothing is launched or allocated.
RowRoute row_route(const Ctx *ctx, const Db *db) {
    const uint32_t S = db->S;
    const uint64_t V = db->V;
    RowRoute r;
    uint64_t max_hs = 0;
    r.max_vs = 0;
    for (uint32_t s_ = 0; s_ < S; ++s_) {
        r.max_vs = std::max<uint64_t>(r.max_vs, db->h_node_off[s_ + 1] - db->h_node_off[s_]);
        max_hs = std::max<uint64_t>(max_hs, db->h_hap_off[s_ + 1] - db->h_hap_off[s_]);
    }
    r.max_haps = (uint32_t)max_hs;
    // Many species: the rows are sorted species by species straight from the node arrays (sample_sort_nodes.hip) -- no compaction pass in front, no limit
    // on a species' size below 2^26 nodes (round 3's compaction + segmented sample sort, unreachable since round 4, was deleted in round 5)
    r.use_nodes = V > SS_MAX_N && r.max_vs <= SSN_MAX_SEG && S <= 65535;
    if (!ctx->cfg.row_sort.empty()) {   // measurements / tests: "radix" = the whole-batch sorts at any size; "nodes" = the batched sort wherever it can run
        const char *ev = ctx->cfg.row_sort.c_str();
        if (ev[0] == 'r') r.use_nodes = false;
        if (ev[0] == 'n') r.use_nodes = r.max_vs <= SSN_MAX_SEG && S <= 65535 && V > 0;
    }
    // above the sample-sort limit the rows that are not sorted from the node arrays go through the radix sort
    r.use_sample = V <= SS_MAX_N;
    r.by_node = use_node_haps(ctx, db);
    // the path_cov_ratio sums ride on the by-node mask pass (PANTAX_RATIO=kernel: ratio_kernel for every species, as in round 3)
    r.ratio_by_node = r.by_node && V && !ctx->cfg.ratio_kernel;
    r.wide = max_hs > (uint64_t)LAD_MAXP;                         // (= lb->n_wide != 0: the species lad_prepare lays the wide tables out for, checked there)
    const bool mask_pass_env = ctx->cfg.mask_pass || ctx->cfg.objective == "nodes";
    // Where the rows are sorted straight from the node arrays and every species has at most 64 haplotypes, the masks are formed INSIDE the sort's histogram
    // pass (ssn_hist_kernel<true>): no mask array, no pass of its own (PANTAX_MASK_PASS=1 keeps mask_nodes_kernel; so do the measurement modes that read the
    // array afterwards).
    r.masks_in_sort = r.use_nodes && r.ratio_by_node && !db->nh_walk_too && !r.wide && !mask_pass_env;
    return r;
}
// species and mask share one key word whenever their bits fit (16-byte records instead of 24): the shift of the species, or -1 for three-word rows
int row_pack_shift(const RowRoute &rt, uint32_t S, int pmax_bound) {
    const int sp_bits = S > 1 ? bits_for(S - 1) : 0;
    return (!rt.use_sample && sp_bits + pmax_bound <= 64 && !(rt.use_nodes && pmax_bound >= 64)) ? pmax_bound : -1;
}

// Which LDS shape the LAD solver launches with (lad.hpp).  Host-known before the launch; nothing is launched or allocated.
LadShape lad_shape(const std::string &option, uint32_t n_workgroups, int n_cu, int pmax_bound) {
    if (pmax_bound > 16 || option == "roomy") return LadShape::roomy;
    if (option == "compact") return LadShape::compact;
    return n_workgroups > (uint32_t)std::max(n_cu, 0) ? LadShape::compact : LadShape::roomy;
}
const char *lad_shape_name(LadShape s) { return s == LadShape::compact ? "compact" : "roomy"; }

// The fused node pass serves the resident step (the coverage pass left its counts: CovState::count_pending) whose masks are formed in the sort, without a11 (it
// needs nvalid on the host and edits the abundances in front of the sort), without the self-cleaning readers, and not the long-node variant of the
// statistics kernel (the reference-DB shape: its per-stretch prefix in LDS does not fit beside the histogram pass's tree and tables -- it stays on the
// two kernels).  Nothing hands `cov` or `ab` out after a resident step, so no output asks for the split path.  Option node_pass=split: never.
bool node_pass_fused_eligible(const Ctx *ctx, const Db *db, const pantax_hip_strain_config *cfg, bool readers_clean) {
    if (ctx->cfg.node_pass == "split" || !db->cov.count_pending() || db->V == 0) return false;
    if (cfg->sample_nodes != 0 || ctx->cfg.cov_readers_clean || readers_clean) return false;
    if (long_node_shape(db->L, db->V, ctx->cfg.ncs_prefix_min, ctx->cfg.ncs_no_prefix)) return false;
    return row_route(ctx, db).masks_in_sort;
}

// ---- the phases of lad_prepare, in the order it calls them
// 1. the candidates of the solver seam: lb->h_p / h_cand -> d_hap_bit / d_p (the strain step's first_filter_kernel wrote them on the device)
static int upload_candidates(Ctx *ctx, const Db *db, LadBatch *lb) {
    const uint32_t S = db->S;
    const uint64_t H = db->H;
    std::vector<int32_t> hap_bit(H ? H : 1, -1);
    for (uint32_t s = 0; s < S; ++s)
        for (int k = 0; k < lb->h_p[s]; ++k) hap_bit[db->h_hap_off[s] + lb->h_cand[db->h_hap_off[s] + k]] = k;
    PTX_TRY(upload(ctx, lb->d_hap_bit, hap_bit.data(), hap_bit.size()));
    PTX_TRY(upload(ctx, lb->d_p, lb->h_p.data(), S));
    return 0;
}
// 2. species that can be wide (more than 64 haplotypes): side arrays laid out once per db, zeroed every step
// More than LAD_WIDEP haplotypes ("huge"): as many mask words as the haplotypes need, rounded up to whole groups of
// LAD_WIDE_NW -- the reference has no cap on the LP columns (dense nvert x npaths matrix, profile.rs:1333-1342), and neither
// has this path; what grows is the scratch (W and G: 3 x (64 nw)^2 doubles per such species) and the time of one workgroup.
static int wide_layout(Ctx *ctx, const Db *db, LadBatch *lb, const RowRoute &rt) {
    const uint32_t S = db->S;
    if (!lb->wide_laid_out) {   // (the batch is its db's own: Db::lad)
        std::vector<uint32_t> off(S ? S : 1, 0xFFFFFFFFu), slot(S ? S : 1, 0xFFFFFFFFu), nwv(S ? S : 1, 0u), list;
        std::vector<uint64_t> woff, coff;
        uint64_t vw = 0, wtot = 0, ctot = 0;
        uint32_t n_huge = 0;
        for (uint32_t s = 0; s < S; ++s) {
            const uint64_t Hs = db->h_hap_off[s + 1] - db->h_hap_off[s];
            if (Hs <= (uint64_t)LAD_MAXP) continue;
            if (Hs > 30000ull) return fail(ctx, PANTAX_HIP_E_LIMIT, "lad_prepare: species %u has %llu haplotypes; the basis inverse is indexed with 32 bits (30000 columns)", s, (unsigned long long)Hs);
            const uint32_t nw = (uint32_t)((Hs + LAD_WIDEP - 1) / LAD_WIDEP) * LAD_WIDE_NW;
            off[s] = (uint32_t)vw; slot[s] = (uint32_t)list.size(); list.push_back(s); nwv[s] = nw;
            vw += (db->h_node_off[s + 1] - db->h_node_off[s]) * (nw / LAD_WIDE_NW);
            woff.push_back(wtot); coff.push_back(ctot);
            wtot += 64ull * nw * 64ull * nw;
            if (nw > (uint32_t)LAD_WIDE_NW) { ++n_huge; ctot += 64ull * nw; }
        }
        if (vw >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "lad_prepare: %llu four-word mask groups in species of more than %d haplotypes", (unsigned long long)vw, LAD_MAXP);
        lb->n_wide = (uint32_t)list.size(); lb->n_huge = n_huge; lb->Vw = vw;
        if (lb->n_wide) {
            PTX_TRY(upload(ctx, lb->d_wide_off, off.data(), S));
            PTX_TRY(upload(ctx, lb->d_wide_slot, slot.data(), S));
            PTX_TRY(upload(ctx, lb->d_wide_nw, nwv.data(), S));
            PTX_TRY(upload(ctx, lb->d_wide_list, list.data(), list.size()));
            woff.insert(woff.end(), coff.begin(), coff.end());     // [n_wide] W offsets, then [n_wide] column-state offsets
            PTX_TRY(upload(ctx, lb->d_wide_woff, woff.data(), woff.size()));
            PTX_HIP(ctx, lb->d_maskw.alloc(vw * LAD_WIDE_NW)); PTX_HIP(ctx, lb->d_pat_or.alloc(vw * LAD_WIDE_NW)); PTX_HIP(ctx, lb->d_pat_and.alloc(vw * LAD_WIDE_NW));
            // W and G are sized by ALL haplotypes of such a species (the candidate count is decided on the device, after the first filter):
            // 3 x (64 nw)^2 doubles each -- 0.6 GB at 5 000 haplotypes, 22 GB at the 30 000 limit.  A db whose scratch does not fit is refused
            // with the figure, not with a bare allocation error (INTEGRATION.md states the cost)
            if (lb->d_wide_W.alloc(wtot) != hipSuccess || lb->d_wide_G.alloc(2 * wtot) != hipSuccess) {
                (void)hipGetLastError();
                lb->d_wide_W.release(); lb->d_wide_G.release();
                return fail(ctx, PANTAX_HIP_E_LIMIT, "lad_prepare: %.1f GB of solver scratch for the %u species of more than %d haplotypes do not fit in device memory "
                            "(3 x (64 x words)^2 doubles per species)", 3.0 * (double)wtot * 8.0 / 1e9, (uint32_t)list.size(), LAD_MAXP);
            }
            if (n_huge) { PTX_HIP(ctx, lb->d_huge_f64.alloc(ctot * 8)); PTX_HIP(ctx, lb->d_huge_i32.alloc(ctot * 5)); }
        }
        lb->wide_laid_out = true;
    }
    if (rt.wide != (lb->n_wide != 0)) return fail(ctx, PANTAX_HIP_E_STATE, "lad_prepare: internal (the row route and the wide tables disagree about species of more than %d haplotypes)", LAD_MAXP);
    if (rt.wide) {
        PTX_TRY(zero_fill(ctx, lb->d_maskw.p, lb->Vw * LAD_WIDE_NW * sizeof(uint64_t)));
        PTX_TRY(zero_fill(ctx, lb->d_pat_or.p, lb->Vw * LAD_WIDE_NW * sizeof(uint64_t)));
        PTX_HIP(ctx, hipMemsetAsync(lb->d_pat_and.p, 0xFF, lb->Vw * LAD_WIDE_NW * sizeof(uint64_t), ctx->stream));
    }
    return 0;
}
// 3. the masks and the path_cov_ratio sums that the row sort does not form itself, and the wide species' hashes
static void mask_ratio_passes(Ctx *ctx, const Db *db, LadBatch *lb, const RowRoute &rt) {
    const uint32_t S = db->S;
    const uint64_t V = db->V;
    if (!rt.masks_in_sort) {
        KTimer t(ctx, rt.by_node ? "mask_nodes_kernel" : "mask_kernel");   // the names rocprofv3 shows
        if (rt.by_node && V)
            hipLaunchKernelGGL(mask_nodes_kernel, dim3((uint32_t)((V + 2047) / 2048)), dim3(256), 0, ctx->stream, V, db->d_emit_tile_sp.p, db->d_node_base.p, db->d_hap_off.p,
                               lb->d_p.p, lb->d_hap_bit.p, (const unsigned long long *)db->d_node_haps.p, (unsigned long long *)lb->d_mask.p,
                               rt.ratio_by_node ? db->d_cov.p : (const uint32_t *)nullptr, db->d_node_len.p, rt.ratio_by_node ? lb->d_ratio.p : (unsigned long long *)nullptr);
        if (db->n_tiles && (!rt.by_node || db->nh_walk_too))
            hipLaunchKernelGGL(mask_kernel, dim3((uint32_t)db->n_tiles), dim3(256), 0, ctx->stream, db->d_tiles.p, db->d_path_off.p,
                               db->d_path_nodes.p, db->d_hap_species.p, db->d_node_base.p, lb->d_hap_bit.p, (unsigned long long *)lb->d_mask.p,
                               lb->d_p.p, rt.wide ? lb->d_wide_off.p : (const uint32_t *)nullptr, lb->d_wide_nw.p, (unsigned long long *)lb->d_maskw.p,
                               rt.by_node ? db->d_hap_off.p : (const uint64_t *)nullptr);
    }
    if (!rt.masks_in_sort && (!rt.ratio_by_node || db->nh_walk_too)) {   // what the mask pass did not sum: species of more than 64 haplotypes (their masks come from the path walk)
        KTimer t(ctx, "ratio_kernel");
        hipLaunchKernelGGL(ratio_kernel, dim3(S * RATIO_CHUNKS), dim3(256), 0, ctx->stream, db->d_node_base.p, db->d_node_len.p, db->d_cov.p,
                           (unsigned long long *)lb->d_mask.p, lb->d_p.p, db->d_hap_off.p, lb->d_wide_off.p, lb->d_wide_nw.p,
                           (const unsigned long long *)lb->d_maskw.p, lb->d_ratio.p, rt.ratio_by_node ? 1 : 0);
    }
    if (rt.wide)
        hipLaunchKernelGGL(mask_fold_kernel, dim3(lb->n_wide * WIDE_CHUNKS), dim3(256), 0, ctx->stream, lb->d_wide_list.p, lb->d_wide_off.p,
                           lb->d_wide_nw.p, db->d_node_base.p, lb->d_p.p, (const unsigned long long *)lb->d_maskw.p, (unsigned long long *)lb->d_mask.p);
}
// 4. rows: compact (the routes that do not read the node arrays) -> sort by (species, mask, a); *sorted: where the sorted rows are.  The staging buffers
// live in the db so that repeated steps do not hipMalloc; the node sort writes the pattern tables itself (from its splitters), so they are allocated here.
static int sort_rows(Ctx *ctx, Db *db, LadBatch *lb, const RowRoute &rt, const FusedNodePass *fused_pass, int pmax_bound, int pack_shift, SortBufs *sorted, bool *c0_valid) {
    const uint32_t S = db->S;
    const uint64_t V = db->V;
    DevBuf<uint32_t> &scan_tmp = db->d_scan_tmp, &table = db->d_sort_table;
    PTX_HIP(ctx, scan_tmp.alloc(scan_tmp_elems(std::max<uint64_t>(V, 256ull * 2048))));
    PTX_HIP(ctx, table.alloc(sort_table_elems(V)));
    PTX_HIP(ctx, lb->d_counts.alloc(4));
    uint32_t *d_n = lb->d_counts.p, *d_K = lb->d_counts.p + 1;
    DevBuf<uint64_t> *ka = db->d_ka, *kb = db->d_kb;
    for (int w = 0; w < 3; ++w) { PTX_HIP(ctx, ka[w].alloc(V)); if (!rt.use_nodes) PTX_HIP(ctx, kb[w].alloc(V)); }
    if (rt.use_nodes) {
        if (pack_shift >= 64) return fail(ctx, PANTAX_HIP_E_LIMIT, "lad_prepare: internal (64 candidate columns and a packed species key)");
    } else {
        KTimer t(ctx, "row_emit_kernel");   // d_n was zeroed with the step's result arena
        const uint32_t grid_rows = (uint32_t)((V + 256ull * ROW_ITEMS - 1) / (256ull * ROW_ITEMS));
        hipLaunchKernelGGL(row_emit_kernel, dim3(grid_rows ? grid_rows : 1), dim3(256), 0, ctx->stream, V, S, db->d_node_base.p, lb->d_ab.p,
                           (unsigned long long *)lb->d_mask.p, d_n, ka[0].p, ka[1].p, ka[2].p, pack_shift);
    }
    if (db->trio.free_event_pending() && db->ev_trio_free) {   // the next step's index rebuild may start from here (api_strain.cpp)
        PTX_HIP(ctx, hipEventRecord(db->ev_trio_free, ctx->stream));
        db->trio.free_event_recorded();
    }
    SortBufs A, B;
    A.nw = B.nw = pack_shift >= 0 ? 2 : 3;
    for (int w = 0; w < 3; ++w) { A.k[w] = ka[w].p; B.k[w] = kb[w].p; }
    bool in_b = false;
    // patterns = runs of equal (species, mask)
    const uint64_t k_cap = V;   // patterns are runs of rows and rows are nodes: never more than V, so the tables cannot overflow
    lb->k_cap = (uint32_t)k_cap;
    PTX_HIP(ctx, lb->d_pat_mask.alloc(k_cap)); PTX_HIP(ctx, lb->d_pat_start.alloc(k_cap + 1)); PTX_HIP(ctx, lb->d_pat_species.alloc(k_cap));
    PTX_HIP(ctx, lb->d_sp_pat_off.alloc(S + 1));
    if (rt.use_nodes) {   // no compaction: the sort's passes read the node arrays and skip the nodes that are no rows; the patterns come from its splitters
        const bool fused = fused_pass != nullptr;
        PTX_HIP(ctx, db->d_ss_ws.alloc(sample_sort_nodes_ws_elems(S, rt.max_vs, V)));
        PTX_HIP(ctx, db->d_row16.alloc(4 * V));
        PTX_HIP(ctx, lb->d_c0.alloc(S));
        const RowPatterns pat{lb->d_pat_mask.p, lb->d_pat_start.p, lb->d_pat_species.p, lb->d_sp_pat_off.p, d_K, lb->d_c0.p};
        *c0_valid = true;
        RowMaskSource hp;
        NodeCovSource fz;
        if (fused) {
            fz.bases = (const unsigned long long *)db->d_bases.p; fz.bit_off = db->d_bit_off.p; fz.full = db->d_full.p; fz.bitmap = db->d_bitmap.p;
            fz.active = fused_pass->active; fz.min_depth = fused_pass->min_depth;
            fz.amax = lb->d_amax.p; fz.nzsum = lb->d_nzsum.p; fz.nvalid = lb->d_nvalid.p; fz.nzcnt = lb->d_nzcnt.p;
        }
        if (rt.masks_in_sort) {
            hp.node_haps = (const unsigned long long *)db->d_node_haps.p; hp.hap_off = db->d_hap_off.p; hp.hap_bit = lb->d_hap_bit.p; hp.sp_p = lb->d_p.p;
            hp.cov = db->d_cov.p; hp.node_len = db->d_node_len.p; hp.ratio = lb->d_ratio.p; hp.max_haps = rt.max_haps;
        }
        PTX_TRY(sample_sort_nodes(ctx, fused ? (const double *)nullptr : lb->d_ab.p, lb->d_mask.p, db->d_node_base.p, S, rt.max_vs, V, db->d_row16.p, A.k, pack_shift, db->d_ss_ws.p, d_n, &pat,
                                  rt.masks_in_sort ? &hp : nullptr, fused ? &fz : nullptr));
        if (fused) db->cov.counted();           // the covered bases were counted (and used) inside the sort
    } else if (rt.use_sample) {   // few rows: sample sort (6 launches) instead of 10+ radix passes of 3 launches each
        PTX_HIP(ctx, db->d_ss_ws.alloc(sample_sort_ws_elems(V)));
        PTX_TRY(sample_sort3(ctx, A, B, V, db->d_ss_ws.p, d_n));
    } else {
        const int sp_bits = S > 1 ? bits_for(S - 1) : 0;
        std::vector<SortPass> passes;
        if (pack_shift >= 0) {
            add_passes(passes, 1, 0, 63);                      // a > 0: sign bit clear
            add_passes(passes, 0, 0, pmax_bound + sp_bits);    // mask bits that can be in use, then the species
        } else {
            add_passes(passes, 2, 0, 63);
            add_passes(passes, 1, 0, pmax_bound);
            if (S > 1) add_passes(passes, 0, 0, sp_bits);
        }
        PTX_TRY(radix_sort(ctx, A, B, V, passes.data(), (int)passes.size(), table.p, scan_tmp.p, &in_b, d_n));
    }
    *sorted = in_b ? B : A;
    lb->row_a = reinterpret_cast<const double *>(sorted->k[pack_shift >= 0 ? 1 : 2]);   // sorted abundances, used in place
    return 0;
}
// 5. the pattern tables of the routes whose sort does not write them, and the wide species' mask words per pattern
static int pattern_tables(Ctx *ctx, const Db *db, LadBatch *lb, const RowRoute &rt, int pack_shift, const SortBufs &Sd) {
    const uint32_t S = db->S;
    uint32_t *d_n = lb->d_counts.p, *d_K = lb->d_counts.p + 1, *d_ovf = lb->d_counts.p + 2;
    if (!rt.use_nodes) {
        const uint64_t *pk1 = pack_shift >= 0 ? (const uint64_t *)nullptr : Sd.k[1];
        PTX_TRY(exclusive_scan_fn(ctx, PatLoad{d_n, Sd.k[0], pk1},
                                  PatStore{Sd.k[0], pk1, lb->k_cap, pack_shift, lb->d_pat_mask.p, lb->d_pat_start.p, lb->d_pat_species.p, d_ovf},
                                  db->V, d_K, "scan_chained_kernel<Pat>"));
        hipLaunchKernelGGL(sp_pat_off_kernel, dim3((S + 1 + 255) / 256), dim3(256), 0, ctx->stream, S, d_K, lb->k_cap, lb->d_pat_species.p, d_n,
                           lb->d_pat_start.p, lb->d_sp_pat_off.p);
    }
    if (rt.wide)
        hipLaunchKernelGGL(wide_pattern_kernel, dim3(lb->n_wide * WIDE_CHUNKS), dim3(256), 0, ctx->stream, lb->d_wide_list.p, lb->d_wide_off.p,
                           lb->d_wide_nw.p, db->d_node_base.p, lb->d_p.p, lb->d_ab.p, (const unsigned long long *)lb->d_mask.p, (const unsigned long long *)lb->d_maskw.p,
                           lb->d_sp_pat_off.p, lb->d_pat_mask.p, (unsigned long long *)lb->d_pat_or.p, (unsigned long long *)lb->d_pat_and.p);
    return 0;
}
// 6. the solver's per-pattern scratch
static int solver_scratch(Ctx *ctx, LadBatch *lb) {
    const uint64_t k_cap = lb->k_cap;
    PTX_TRY(lb->pat_scratch.alloc(ctx, k_cap));
    if (lb->n_huge) PTX_HIP(ctx, lb->d_pat_act.alloc(k_cap));
    return 0;
}

// All of it is enqueued without a host round trip: the row count n and the pattern count K stay on the
// device (lb->d_counts = {n_rows, K, overflow}); buffers are sized by their host-known bounds (n <= V,
// K <= k_cap).  The request and what comes back in *rows: lad.hpp.
int lad_prepare(Ctx *ctx, Db *db, LadBatch *lb, const LadRequest &rq, LadRows *rows) {
    const uint64_t V = db->V, H = db->H;
    const RowRoute rt = row_route(ctx, db);
    const int pack_shift = row_pack_shift(rt, db->S, rq.pmax_bound);
    *rows = LadRows{false, rt.masks_in_sort, rq.fused != nullptr};
    if (!rq.cand_on_device) PTX_TRY(upload_candidates(ctx, db, lb));
    PTX_HIP(ctx, lb->d_mask.alloc(V));
    PTX_HIP(ctx, lb->d_ratio.alloc((size_t)(H ? H : 1) * 2));
    if (!rq.zeroed && !rt.by_node) PTX_TRY(zero_fill(ctx, lb->d_mask.p, V * sizeof(uint64_t)));   // (mask_nodes_kernel writes every word)
    PTX_TRY(wide_layout(ctx, db, lb, rt));
    // d_ratio and d_counts live in the step's result arena, which the caller has just zeroed
    // the fused node pass was decided before the step's first kernel (strain_enqueue): no abundance array and no covered-base counts exist, so every reader
    // of them below (mask_nodes_kernel, ratio_kernel, row_emit_kernel, wide_pattern_kernel; objective_kernel in objective_launch) is excluded by it
    if (rq.fused && (!rt.masks_in_sort || rt.wide || !rq.cand_on_device))
        return fail(ctx, PANTAX_HIP_E_STATE, "lad_prepare: internal (the fused node pass without masks formed in the row sort)");
    mask_ratio_passes(ctx, db, lb, rt);
    SortBufs sorted;
    PTX_TRY(sort_rows(ctx, db, lb, rt, rq.fused, rq.pmax_bound, pack_shift, &sorted, &rows->c0_valid));
    PTX_TRY(pattern_tables(ctx, db, lb, rt, pack_shift, sorted));
    PTX_TRY(solver_scratch(ctx, lb));
    PTX_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace ptx
