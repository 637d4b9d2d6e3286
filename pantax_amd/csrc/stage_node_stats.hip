// stage_node_stats.hip -- node abundance + per-species statistics of the strain step (with the covered-base counts folded in for the
// resident step), and a11: row sub-sampling (sample_sorted, profile.rs:1287-1295).
#include <algorithm>
#include <cstdio>
#include <vector>
#include "lad.hpp"
#include "lad_device.hpp"
#include "cov_plan.hpp"
#include "row_sample.hpp"
#include "primitives.hpp"
#include "wave.hpp"
#include "scan_chained.hpp"

namespace ptx {

// ---------------------------------------------------------------------------------------------
// node abundance + per-species statistics
// ---------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) node_stats_kernel(const uint32_t *__restrict__ node_base, const uint32_t *__restrict__ node_len,
                                                         const unsigned long long *__restrict__ bases, double min_depth,
                                                         double *__restrict__ ab_out, NodePartial *__restrict__ part,
                                                         const uint32_t *__restrict__ chunk_sp, const uint32_t *__restrict__ sp_chunk_off) {
    __shared__ double red[4];
    __shared__ unsigned long long redu[4];
    // chunks by SIZE (round 6): a species takes chunks in proportion to its nodes -- with one workgroup per species (what an even split gave a db of
    // thousands of species) the 3e5-node graphs of the multi-strain species ran beside 5e3-node chunk graphs: 12.4 ms at the reference-DB shape
    const uint32_t s = chunk_sp[blockIdx.x], nch = sp_chunk_off[s + 1] - sp_chunk_off[s], ch = blockIdx.x - sp_chunk_off[s];
    const uint32_t b = node_base[s], e = node_base[s + 1];
    const uint32_t per = (e - b + nch - 1) / nch;
    uint32_t lo = b + ch * per, hi = lo + per;
    if (hi > e) hi = e;
    double mx = -INFINITY, zs = 0.0;
    unsigned long long nv = 0, zc = 0;
    for (uint32_t v = lo + threadIdx.x; v < hi; v += 256) {
        double len = (double)node_len[v];                        // (the 4-byte copy of the lengths: 4V instead of 8V of offsets)
        double ab = (double)(long long)bases[v] / len;           // profile.rs:987-988
        ab_out[v] = ab;
        mx = fmax(mx, ab);
        if (ab > 0.0) ++nv;
        double o = ab > min_depth ? ab : 0.0;                    // :2941-2944
        if (o > 0.0) { zs += o; ++zc; }
    }
    mx = block_max_f64<256>(mx, red);
    zs = block_sum_f64<256>(zs, red);
    nv = block_sum_u64<256>(nv, redu);
    zc = block_sum_u64<256>(zc, redu);
    if (threadIdx.x == 0) part[blockIdx.x] = {mx, zs, nv, zc};
}
// The same pass with the covered-base count of every node folded in (node_base_cov, profile.rs:844/874, :1018-1023 -- popcount_kernel's
// work, stage_cov.hip): in the resident step nothing reads the counts between the coverage pass and this one, and the two passes share
// the node lengths.  The bit offset of a node comes from a running prefix of the lengths inside the workgroup's range (one 8-byte load
// per workgroup instead of 8V bytes of offsets); 24V + L/8 bytes instead of 32V + L/8 for the two kernels.
// CLEAN (round 6): this pass is the LAST reader of `bases`, the bit vector and the full-node flags in the resident step -- it leaves them zeroed for
// the next step's coverage pass (only what is not zero is written: the lines are in the caches, a node some step covered whole has no marked bits),
// instead of a 4-GB zero fill per step in front of it.  A word of flags / bits that a wave shares with its neighbours (the ends of its range of nodes)
// loses this wave's bits only, atomically; a word that is all its own is stored.  (No __restrict__ on the three arrays: they are read and written here.)
// LONGN (round 6): graphs of LONG nodes -- a single-genome species is a chain of 1024-bp chunks (build_eq1.rs:26-36), 32 bitmap words per node.  The
// per-lane loop over a node's interior words walks 64 different cache lines per iteration (12.4 ms at the reference-DB shape).  Instead the wave reads
// the words of its whole 64-node stretch coalesced, keeps the running count of set bits in front of every word in LDS (a DPP prefix sum per 64 words),
// and a node's covered bases are the difference of that prefix at its two ends -- two LDS reads per node, whatever its length.
constexpr uint32_t NCS_PWORDS = 2304;   // words of one stretch the prefix holds (64 nodes x 1152 bases); a longer stretch takes the per-lane loop
extern __shared__ __attribute__((aligned(16))) uint32_t s_ncs_prefix[];
template <bool CLEAN, bool LONGN = false>
__global__ void __launch_bounds__(256) node_cov_stats_kernel(const uint32_t *__restrict__ node_base, const uint32_t *__restrict__ node_len,
                                                             unsigned long long *bases, const uint64_t *__restrict__ bit_off,
                                                             uint32_t *full, uint32_t *bitmap, double min_depth,
                                                             uint32_t *__restrict__ cov_out, double *__restrict__ ab_out, NodePartial *__restrict__ part,
                                                             const uint32_t *__restrict__ chunk_sp, const uint32_t *__restrict__ sp_chunk_off,
                                                             const uint8_t *__restrict__ active) {
    __shared__ double red[4];
    __shared__ unsigned long long redu[4];
    const uint32_t s = chunk_sp[blockIdx.x], nch = sp_chunk_off[s + 1] - sp_chunk_off[s], ch = blockIdx.x - sp_chunk_off[s];   // (chunks by size: node_stats_kernel)
    const uint32_t b = node_base[s], e = node_base[s + 1];
    const uint32_t per = (e - b + nch - 1) / nch;
    uint32_t lo = b + ch * per, hi = lo + per;
    if (hi > e) hi = e;
    // A species the species level dropped (round 6): the coverage pass skipped its reads (the same flags), so its part of the arena is all zero and what this
    // pass would compute from it is known -- zeros, written without reading anything.  The work follows the species that are PRESENT in the sample, not the
    // size of the resident DB (the reference-DB shape, four fifths of the single-genome species absent: this pass 4.97 -> 3.92 ms, the step 25.4 -> 23.2).
    if (active != nullptr && active[s] == 0) {                   // (workgroup-uniform)
        for (uint32_t v = lo + threadIdx.x; v < hi; v += 256) { cov_out[v] = 0u; ab_out[v] = 0.0; }
        if (threadIdx.x == 0) part[blockIdx.x] = {hi > lo ? 0.0 : -INFINITY, 0.0, 0ull, 0ull};
        return;
    }
    double mx = -INFINITY, zs = 0.0;
    unsigned long long nv = 0, zc = 0;
    // every WAVE walks its own quarter of the workgroup's range with its own running bit offset: no LDS, no barrier in the loop --
    // the waves of a CU hide each other's two dependent loads (lengths -> bitmap words)
#ifndef NCS_NR
#define NCS_NR 4
#endif
    constexpr int NR = NCS_NR;                                   // 64-node stretches per round: their loads are in flight together (-DNCS_NR: measurement builds)
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t quarter = ((hi > lo ? hi - lo : 0u) + 3u) / 4u;
    const uint32_t wlo = min(hi, lo + wave * quarter), whi = min(hi, wlo + quarter);
    uint64_t run = wlo < whi ? bit_off[wlo] : 0ull;              // bit offset of the first node of the coming round
    // (requesting the three streams of round r + 1 at the top of round r -- what took a dependent level off the coverage kernel's chain -- LOST here:
    // 2.55 -> 3.17 ms at 1e4 strains, 16 more registers for a kernel whose rounds are already four stretches deep)
    for (uint32_t v0 = wlo; v0 < whi; v0 += 64 * NR) {
        uint32_t l[NR], fw[NR];
        unsigned long long bs[NR];
        uint64_t g0[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint32_t v = v0 + (uint32_t)r * 64u + lane;
            const bool in = v < whi;
            l[r] = in ? node_len[v] : 0u;
            bs[r] = in ? bases[v] : 0ull;
            fw[r] = in ? full[v >> 5] : 0u;
        }
        const uint64_t round_b0 = run;                           // the bits of this round's nodes: [round_b0, run) once the lengths are summed
        uint64_t sb[NR + 1];                                     // first bit of every stretch (wave-uniform)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint32_t incl = wave_incl_scan_dpp(l[r]);      // (a species' bases fit 32 bits: checked at upload)
            sb[r] = run;
            g0[r] = run + incl - l[r];
            run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        sb[NR] = run;
        uint32_t bw0[NR], bw1[NR];                               // first and last bitmap word of every node: independent loads, issued together
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const bool any = l[r] != 0u;                         // (l = 0 outside the range)
            bw0[r] = any ? bitmap[g0[r] >> 5] : 0u;
            bw1[r] = any ? bitmap[(g0[r] + l[r] - 1) >> 5] : 0u;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint32_t v = v0 + (uint32_t)r * 64u + lane;
            bool coop = false;                                   // (wave-uniform) this stretch's counts come from the prefix in LDS
            uint64_t wa = 0;
            if constexpr (LONGN) {
                const uint64_t b0 = sb[r], b1 = sb[r + 1];
                const bool has_long = __builtin_amdgcn_ballot_w64(l[r] > 64u) != 0ull;
                wa = (b0 >> 5) & ~3ull;                                  // (from a 16-byte boundary: four words per lane and load; the tail read beyond the stretch is inside the arena)
                const uint64_t nw = b1 > b0 ? ((b1 - 1) >> 5) - wa + 1 : 0;
                coop = has_long && nw <= (uint64_t)NCS_PWORDS;
                if (coop) {
                    uint32_t *pw = s_ncs_prefix + wave * NCS_PWORDS;
                    uint32_t carry = 0;
                    for (uint32_t k = 0; k < (uint32_t)nw; k += 256) {
                        const uint32_t i = k + 4u * lane;
                        const uint4 x = i < (uint32_t)nw ? *reinterpret_cast<const uint4 *>(bitmap + wa + i) : make_uint4(0u, 0u, 0u, 0u);
                        const uint32_t p0 = (uint32_t)__popc(x.x), p1 = p0 + (uint32_t)__popc(x.y), p2 = p1 + (uint32_t)__popc(x.z), p3 = p2 + (uint32_t)__popc(x.w);
                        const uint32_t incl = wave_incl_scan_dpp(p3);
                        const uint32_t base = carry + incl - p3;              // set bits in front of this lane's four words
                        if (i < (uint32_t)nw) *reinterpret_cast<uint4 *>(pw + i) = make_uint4(base, base + p0, base + p1, base + p2);
                        carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
                }
            }
            if (v >= whi) continue;
            uint32_t c = 0;
            if (LONGN && coop) {
                if (l[r]) {
                    const uint64_t g1 = g0[r] + l[r], w0 = g0[r] >> 5, w1 = (g1 - 1) >> 5;
                    const uint32_t below0 = (1u << (g0[r] & 31)) - 1u, m1 = 0xFFFFFFFFu >> (31 - (uint32_t)((g1 - 1) & 31));
                    const uint32_t *pw = s_ncs_prefix + wave * NCS_PWORDS;
                    c = (pw[w1 - wa] + (uint32_t)__popc(bw1[r] & m1)) - (pw[w0 - wa] + (uint32_t)__popc(bw0[r] & below0));
                }
            } else
            if (l[r]) {
                const uint64_t g1 = g0[r] + l[r], w0 = g0[r] >> 5, w1 = (g1 - 1) >> 5;
                const uint32_t m0 = 0xFFFFFFFFu << (g0[r] & 31), m1 = 0xFFFFFFFFu >> (31 - (uint32_t)((g1 - 1) & 31));
                c = w0 == w1 ? __popc(bw0[r] & m0 & m1) : __popc(bw0[r] & m0) + __popc(bw1[r] & m1);
                for (uint64_t w = w0 + 1; w < w1; ++w) {                           // nodes of more than 33 bases
                    const uint32_t x = bitmap[w];
                    c += __popc(x);
                    if (CLEAN && x) bitmap[w] = 0u;                                // (a word inside one node is that node's alone)
                }
                if constexpr (CLEAN) {
                    // A word is zeroed by the node that holds its LAST bit, with a plain store of what that lane has loaded anyway -- when all of the word's
                    // bits belong to THIS round of this wave [round_b0, run): every other node that touches the word has then been read, in this very round.
                    // The (at most two) words that reach over the round's ends lose this round's bits atomically, below.
                    const bool in0 = (w0 << 5) >= round_b0 && (w0 << 5) + 32 <= run, in1 = (w1 << 5) >= round_b0 && (w1 << 5) + 32 <= run;
                    if (bw0[r] && in0 && (w0 << 5) + 32 <= g1) bitmap[w0] = 0u;
                    if (w1 != w0 && bw1[r] && in1 && (g1 & 31) == 0) bitmap[w1] = 0u;
                }
            }
            if ((fw[r] >> (v & 31u)) & 1u) c = l[r];             // a step covered the whole node: a flag instead of marked bits
            cov_out[v] = c;
            const double len = (double)l[r];
            const double ab = (double)(long long)bs[r] / len;    // profile.rs:987-988
            ab_out[v] = ab;
            mx = fmax(mx, ab);
            if (ab > 0.0) ++nv;
            const double o = ab > min_depth ? ab : 0.0;          // :2941-2944
            if (o > 0.0) { zs += o; ++zc; }
        }
        if constexpr (CLEAN) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const uint32_t v = v0 + (uint32_t)r * 64u + lane;
                const bool in = v < whi;
                if (in && bs[r] != 0ull) bases[v] = 0ull;
                // the flags of this stretch's nodes, word by word: the first lane of every word's run of lanes clears the run's bits
                if (in && (lane == 0u || (v & 31u) == 0u)) {
                    const uint32_t n = min(min(32u - (v & 31u), 64u - lane), whi - v);
                    const uint32_t m = (n >= 32u ? 0xFFFFFFFFu : ((1u << n) - 1u)) << (v & 31u);
                    if (fw[r] & m) { if (m == 0xFFFFFFFFu) full[v >> 5] = 0u; else atomicAnd(&full[v >> 5], ~m); }
                }
            }
            if (run > round_b0 && lane < 2u) {                   // the words over the round's two ends: this round's bits of them, atomically (lane 0: the first, lane 1: the last)
                const uint64_t ws = round_b0 >> 5, we = (run - 1) >> 5;
                const uint32_t ms = 0xFFFFFFFFu << (round_b0 & 31), me = 0xFFFFFFFFu >> (31 - (uint32_t)((run - 1) & 31));
                const bool s_part = (round_b0 & 31) != 0, e_part = (run & 31) != 0;
                if (lane == 0u && (s_part || (ws == we && e_part))) atomicAnd(&bitmap[ws], ~(ws == we ? ms & me : ms));
                if (lane == 1u && e_part && we != ws) atomicAnd(&bitmap[we], ~me);
            }
        }
    }
    __syncthreads();
    mx = block_max_f64<256>(mx, red);
    zs = block_sum_f64<256>(zs, red);
    nv = block_sum_u64<256>(nv, redu);
    zc = block_sum_u64<256>(zc, redu);
    if (threadIdx.x == 0) part[blockIdx.x] = {mx, zs, nv, zc};
}
// one wave per species: lane l combines chunks l, l+64, ... in order, then a fixed-shape wave reduction
__global__ void __launch_bounds__(64) node_stats_final_kernel(uint32_t S, const NodePartial *__restrict__ part, double *__restrict__ amax_out,
                                                              uint32_t *__restrict__ nvalid_out, double *__restrict__ nzsum_out,
                                                              uint32_t *__restrict__ nzcnt_out, const uint32_t *__restrict__ sp_chunk_off) {
    const uint32_t s = blockIdx.x, c0 = sp_chunk_off[s], nch = sp_chunk_off[s + 1] - c0;
    double mx = -INFINITY, zs = 0.0; unsigned long long nv = 0, zc = 0;
    for (uint32_t c = threadIdx.x; c < nch; c += 64) { NodePartial p = part[(size_t)c0 + c]; mx = fmax(mx, p.mx); zs += p.zs; nv += p.nv; zc += p.zc; }
    mx = wave_reduce(mx, [](double x, double y) { return fmax(x, y); });
    zs = wave_reduce(zs, [](double x, double y) { return x + y; });
    nv = wave_reduce(nv, [](unsigned long long x, unsigned long long y) { return x + y; });
    zc = wave_reduce(zc, [](unsigned long long x, unsigned long long y) { return x + y; });
    if (threadIdx.x == 0) { amax_out[s] = mx; nvalid_out[s] = (uint32_t)nv; nzsum_out[s] = zs; nzcnt_out[s] = (uint32_t)zc; }
}

int node_stats_launch(Ctx *ctx, Db *db, LadBatch *lb, int64_t min_depth, const uint8_t *d_active, bool readers_clean) {
    if (ctx->cfg.no_absent_skip) d_active = nullptr;     // (tests compare, measurements)
    uint32_t S = db->S;
    lb->S = S;
    PTX_HIP(ctx, lb->d_ab.alloc(db->V));
    PTX_HIP(ctx, lb->d_amax.alloc(S)); PTX_HIP(ctx, lb->d_nvalid.alloc(S));
    PTX_HIP(ctx, lb->d_nzsum.alloc(S)); PTX_HIP(ctx, lb->d_nzcnt.alloc(S));
    PTX_HIP(ctx, lb->d_partial.alloc((size_t)S * STAT_CHUNKS * 4));
    const bool with_cov = db->cov.count_pending();               // the resident step left the covered-base counts to this pass
    if (with_cov) PTX_HIP(ctx, db->d_cov.alloc(db->V));
    // the chunk table of this db (made once per variant): ~8192 workgroups in all for the fused kernel (it holds fewer workgroups per CU: shorter ones, so
    // that the last round is short), ~2048 for the plain one; every species at least one chunk and at most STAT_CHUNKS, in proportion to its nodes
    Db::NodeChunks &nc = db->node_chunks[with_cov ? 1 : 0];
    if (nc.n == 0 && S) {
        const double target = std::max(1.0, (double)db->V / (with_cov ? 8192.0 : 2048.0));
        std::vector<uint32_t> off(S + 1, 0), sp;
        for (uint32_t s2 = 0; s2 < S; ++s2) {
            const double vs = (double)(db->h_node_off[s2 + 1] - db->h_node_off[s2]);
            const uint32_t k = (uint32_t)std::min<double>((double)STAT_CHUNKS, std::max(1.0, std::floor(vs / target + 0.5)));
            off[s2 + 1] = off[s2] + k;
            sp.insert(sp.end(), k, s2);
        }
        PTX_TRY(upload(ctx, nc.d_sp_off, off.data(), off.size()));
        PTX_TRY(upload(ctx, nc.d_chunk_sp, sp.data(), sp.size()));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (once per db: the staging vectors go out of scope)
        nc.n = off[S];
    }
    KTimer t(ctx, with_cov ? "node_cov_stats_kernel" : "node_stats_kernel");
    if (with_cov) {
        if (readers_clean)
        hipLaunchKernelGGL(node_cov_stats_kernel<true>, dim3(nc.n), dim3(256), 0, ctx->stream, db->d_node_base.p, db->d_node_len.p, db->d_bases.p, db->d_bit_off.p,
                           db->d_full.p, db->d_bitmap.p, (double)min_depth, db->d_cov.p, lb->d_ab.p, (NodePartial *)lb->d_partial.p, (const uint32_t *)nc.d_chunk_sp.p, (const uint32_t *)nc.d_sp_off.p, d_active);
        else if (long_node_shape(db->L, db->V, ctx->cfg.ncs_prefix_min, ctx->cfg.ncs_no_prefix))   // long nodes on average (chunk graphs of single-genome species among them): counts from a per-stretch prefix in LDS
        hipLaunchKernelGGL((node_cov_stats_kernel<false, true>), dim3(nc.n), dim3(256), (size_t)4 * NCS_PWORDS * sizeof(uint32_t), ctx->stream, db->d_node_base.p, db->d_node_len.p, db->d_bases.p, db->d_bit_off.p,
                           db->d_full.p, db->d_bitmap.p, (double)min_depth, db->d_cov.p, lb->d_ab.p, (NodePartial *)lb->d_partial.p, (const uint32_t *)nc.d_chunk_sp.p, (const uint32_t *)nc.d_sp_off.p, d_active);
        else
        hipLaunchKernelGGL(node_cov_stats_kernel<false>, dim3(nc.n), dim3(256), 0, ctx->stream, db->d_node_base.p, db->d_node_len.p, db->d_bases.p, db->d_bit_off.p,
                           db->d_full.p, db->d_bitmap.p, (double)min_depth, db->d_cov.p, lb->d_ab.p, (NodePartial *)lb->d_partial.p, (const uint32_t *)nc.d_chunk_sp.p, (const uint32_t *)nc.d_sp_off.p, d_active);
        db->cov.counted();
    } else
    hipLaunchKernelGGL(node_stats_kernel, dim3(nc.n), dim3(256), 0, ctx->stream, db->d_node_base.p, db->d_node_len.p, db->d_bases.p,
                       (double)min_depth, lb->d_ab.p, (NodePartial *)lb->d_partial.p, (const uint32_t *)nc.d_chunk_sp.p, (const uint32_t *)nc.d_sp_off.p);
    hipLaunchKernelGGL(node_stats_final_kernel, dim3(S), dim3(64), 0, ctx->stream, S, (const NodePartial *)lb->d_partial.p,
                       lb->d_amax.p, lb->d_nvalid.p, lb->d_nzsum.p, lb->d_nzcnt.p, (const uint32_t *)nc.d_sp_off.p);
    PTX_HIP(ctx, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// a11: row sub-sampling (sample_sorted, profile.rs:1287-1295 and its call sites :1394-1400 / :2738-2752).
// Only species with more valid rows than `sample_nodes` are touched, and only those cost a host round trip (their
// row count n decides the chosen ranks).  The chosen set is a bitmap over the RANKS of the valid rows in node
// order (row_sample.cpp); one chained scan ranks the valid nodes and clears the abundance of the unchosen ones in
// the LP's copy, so row_emit_kernel and objective_kernel see exactly the sampled rows.  max a (the x bound),
// path_cov_ratio and the single-path statistics were taken before and are not sampled (profile.rs:2700-2729).
// ---------------------------------------------------------------------------------------------
struct SampleLoad {
    const double *ab;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return ab[i] > 0.0 ? 1u : 0u; }
};
struct SampleStore {
    double *ab;
    const uint32_t *bits;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t rank, uint32_t valid) const {
        if (valid && !((bits[rank >> 5] >> (rank & 31)) & 1u)) ab[i] = 0.0;
    }
};

int row_sample_apply(Ctx *ctx, const Db *db, LadBatch *lb, int64_t sample_nodes) {
    const uint32_t S = db->S;
    bool possible = false;
    for (uint32_t s = 0; s < S && !possible; ++s) possible = (int64_t)(db->h_node_off[s + 1] - db->h_node_off[s]) > sample_nodes;
    if (sample_nodes <= 0 || !possible) return 0;   // no species can have more valid rows than the limit
    std::vector<uint32_t> nvalid(S);
    PTX_TRY(download(ctx, nvalid.data(), lb->d_nvalid.p, S));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> bits;
    DevBuf<uint32_t> d_bits;
    for (uint32_t s = 0; s < S; ++s) {
        if ((int64_t)nvalid[s] <= sample_nodes) continue;
        sample_ranks(nvalid[s], (uint64_t)sample_nodes, 42, bits);
        PTX_TRY(upload(ctx, d_bits, bits.data(), bits.size()));
        double *ab = lb->d_ab.p + db->h_node_off[s];
        PTX_TRY(exclusive_scan_fn(ctx, SampleLoad{ab}, SampleStore{ab, d_bits.p}, db->h_node_off[s + 1] - db->h_node_off[s], nullptr, "row_sample_kernel"));
        nvalid[s] = (uint32_t)sample_nodes;                // n of the objective's 1/n (profile.rs:2755)
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // d_bits is reused by the next species
    }
    PTX_HIP(ctx, hipMemcpyAsync(lb->d_nvalid.p, nvalid.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // namespace ptx
