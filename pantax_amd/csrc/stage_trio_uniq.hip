// stage_trio_uniq.hip -- which windows of the unique-trio index (a7) occur once (count_per_trio == 1, profile.rs:688-709), by three paths that write the
// same outputs -- one flag bit per unique window start and the count of unique windows per middle node (the visit kernel on the fast route: the
// groups' ballots and records instead): the visit table (trio_visit_kernel, the default), node blocks in LDS for the species that hold a node of
// more than 64 visits (trio_block_kernel), and global buckets for a whole db (trio_count / fill / uniq kernels: round 1's plan, now the fallback).
// One host function per bracket of trio_index_build at the end.
#include <algorithm>
#include "trio_device.hpp"

namespace ptx {

// 1. bucket sizes: windows per middle node
__global__ void __launch_bounds__(256) trio_count_kernel(TRIO_GRAPH_ARGS, uint32_t *__restrict__ cnt) {
    TILE_LOOP(q, h, qend) {
        const uint32_t nb = node_base[hap_species[h]];
        uint32_t g, a, b, c;
        if (window_of(q, qend, nb, path_nodes, g, a, b, c)) atomicAdd(&cnt[g], 1u);
    }
}
// uniq flags of the path positions: ONE BIT per position (a byte per position cost 8x the zero-fill before every build and
// 8x the reads of the two passes that rank the unique windows)
__device__ __forceinline__ void uniq_mark(uint32_t *__restrict__ bits, uint32_t q) { atomicOr(&bits[q >> 5], 1u << (q & 31u)); }
// 2. scatter windows into their bucket (slot order inside a bucket is arbitrary and irrelevant)
__global__ void __launch_bounds__(256) trio_fill_kernel(TRIO_GRAPH_ARGS, const uint32_t *__restrict__ bucket_off,
                                                        uint32_t *__restrict__ cursor, uint4 *__restrict__ bucket) {
    TILE_LOOP(q, h, qend) {
        const uint32_t nb = node_base[hap_species[h]];
        uint32_t g, a, b, c;
        if (!window_of(q, qend, nb, path_nodes, g, a, b, c)) continue;
        uint32_t slot = bucket_off[g] + atomicAdd(&cursor[g], 1u);
        bucket[slot] = make_uint4((uint32_t)q, a, c, g);   // one 16-byte record per window: {start position, smaller end, larger end, middle}
    }
}
// 3. a window is unique iff no other window of its bucket has the same (b,c): count == 1 (profile.rs:688-709).
//    Entries of a bucket are contiguous, so a wave compares its 64 consecutive entries through shuffles (one
//    16-byte load per window instead of one per pair); only the part of a bucket that lies outside the wave's
//    64 entries is read from memory.
__global__ void __launch_bounds__(256) trio_uniq_kernel(uint64_t n_win, const uint4 *__restrict__ bucket,
                                                        const uint32_t *__restrict__ bucket_off, uint32_t *__restrict__ uniq_q,
                                                        uint32_t *__restrict__ first_cnt) {
    const int lane = threadIdx.x & 63;
    for (uint64_t base = ((uint64_t)blockIdx.x * 256 + threadIdx.x) - lane; base < n_win; base += (uint64_t)gridDim.x * 256) {
        const uint64_t i = base + lane;
        const bool valid = i < n_win;
        uint4 me = make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);
        if (valid) me = bucket[i];
        const uint32_t g = me.w;
        bool dup = false;
        // my place inside my bucket tells which lower lanes share it (entries of a bucket are contiguous): no id shuffle
        uint32_t b0 = 0, b1 = 0;
        if (valid) { b0 = bucket_off[g]; b1 = bucket_off[g + 1]; }
        const uint32_t below = valid ? (uint32_t)(i - b0) : 0u;         // entries of my bucket before me
        for (int d = 1; d < 64; ++d) {
            const bool same = valid && lane >= d && (uint32_t)d <= below;
            if (!__any(same)) break;   // no pair at distance d means none further apart
            const uint32_t oy = __shfl(me.y, lane - d), oz = __shfl(me.z, lane - d);
            const unsigned long long eq = __ballot(same && oy == me.y && oz == me.z);
            if ((eq >> lane) & 1ull) dup = true;                            // my partner is d below
            if (lane + d < 64 && ((eq >> (lane + d)) & 1ull)) dup = true;   // my partner is d above
        }
        if (valid && !dup) {
            const uint64_t wend = base + 64;
            for (uint64_t j = b0; j < b1 && j < base && !dup; ++j) { const uint4 o = bucket[j]; if (o.y == me.y && o.z == me.z) dup = true; }
            for (uint64_t j = (wend > b0 ? wend : b0); j < b1 && !dup; ++j) { const uint4 o = bucket[j]; if (o.y == me.y && o.z == me.z) dup = true; }
        }
        if (valid && !dup) { uniq_mark(uniq_q, me.x); atomicAdd(&first_cnt[g], 1u); }
    }
}
// 3'. the same test through an LDS hash table, for graphs where many haplotypes share their nodes (buckets of tens of
//     entries, nearly all of them equal): a workgroup owns the buckets that START inside its slice of UNIQ_CH
//     entries (bucket_off is searched for the two slice ends), so every bucket is seen whole by one workgroup.  Each
//     entry claims or joins the table slot of its (g, b, c) and counts itself there; unique <=> the count is 1.  O(1)
//     per window instead of O(bucket).  A slice that does not fit the LDS copy (one bucket of thousands of entries)
//     falls back to scanning the bucket in memory.
constexpr uint32_t UNIQ_CH = 1024, UNIQ_CAP = 1536, UNIQ_SLOTS = 4096;
__device__ __forceinline__ uint32_t uniq_hash(uint32_t g, uint32_t b, uint32_t c) {
    uint32_t h = g * 0x9E3779B1u;
    h = (h ^ b) * 0x85EBCA77u;
    h = (h ^ c) * 0xC2B2AE3Du;
    return (h ^ (h >> 15)) & (UNIQ_SLOTS - 1);
}
__global__ void __launch_bounds__(256) trio_uniq_lds_kernel(uint64_t n_win, uint32_t V, const uint4 *__restrict__ bucket,
                                                            const uint32_t *__restrict__ bucket_off, uint32_t *__restrict__ uniq_q,
                                                            uint32_t *__restrict__ first_cnt) {
    __shared__ uint32_t s_g[UNIQ_CAP], s_b[UNIQ_CAP], s_c[UNIQ_CAP];
    __shared__ uint32_t s_tab[UNIQ_SLOTS], s_cnt[UNIQ_SLOTS];
    constexpr uint32_t EMPTY = 0xFFFFFFFFu;
    // first bucket start >= x (bucket_off[0..V] ascending, bucket_off[V] = n_win)
    auto first_start = [&](uint64_t x) -> uint64_t {
        if (x >= n_win) return n_win;
        uint32_t lo = 0, hi = V;                       // smallest v with bucket_off[v] >= x
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)bucket_off[mid] < x) lo = mid + 1; else hi = mid; }
        return bucket_off[lo];
    };
    const uint64_t lo = first_start((uint64_t)blockIdx.x * UNIQ_CH), hi = first_start((uint64_t)(blockIdx.x + 1) * UNIQ_CH);
    if (hi <= lo) return;
    const uint32_t n = (uint32_t)(hi - lo);
    if (n > UNIQ_CAP) {                                // oversized bucket(s): plain scan of each entry's bucket
        for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) {
            const uint4 me = bucket[i];
            bool dup = false;
            for (uint32_t j = bucket_off[me.w], e = bucket_off[me.w + 1]; j < e && !dup; ++j)
                if (j != i) { const uint4 o = bucket[j]; dup = o.y == me.y && o.z == me.z; }
            if (!dup) { uniq_mark(uniq_q, me.x); atomicAdd(&first_cnt[me.w], 1u); }
        }
        return;
    }
    for (uint32_t k = threadIdx.x; k < UNIQ_SLOTS; k += 256) { s_tab[k] = EMPTY; s_cnt[k] = 0; }
    uint32_t my_q[UNIQ_CAP / 256], my_slot[UNIQ_CAP / 256];
#pragma unroll
    for (int k = 0; k < (int)(UNIQ_CAP / 256); ++k) {
        const uint32_t t = threadIdx.x + k * 256;
        if (t < n) { const uint4 me = bucket[lo + t]; my_q[k] = me.x; s_b[t] = me.y; s_c[t] = me.z; s_g[t] = me.w; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (int)(UNIQ_CAP / 256); ++k) {
        const uint32_t t = threadIdx.x + k * 256;
        if (t >= n) continue;
        const uint32_t g = s_g[t], b = s_b[t], c = s_c[t];
        uint32_t h = uniq_hash(g, b, c);
        for (;;) {
            uint32_t cur = s_tab[h];
            if (cur == EMPTY) cur = atomicCAS(&s_tab[h], EMPTY, t);
            if (cur == EMPTY || (s_g[cur] == g && s_b[cur] == b && s_c[cur] == c)) break;
            h = (h + 1) & (UNIQ_SLOTS - 1);
        }
        atomicAdd(&s_cnt[h], 1u);
        my_slot[k] = h;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (int)(UNIQ_CAP / 256); ++k) {
        const uint32_t t = threadIdx.x + k * 256;
        if (t < n && s_cnt[my_slot[k]] == 1u) { uniq_mark(uniq_q, my_q[k]); atomicAdd(&first_cnt[s_g[t]], 1u); }
    }
}
// 3''. Uniqueness by node block, no global scatter (round 2's default; since round 4 the path of species that hold a node with
//      more than 64 visits -- everything else goes through the visit table below).  Every species' nodes are cut into blocks of
//      TRIO_BLK consecutive local ids; the walks were cut at upload into runs of consecutive positions inside one block
//      (trio_runs_build, stage_trio_tables.hip).  A window is OWNED by the position of its MIDDLE node: position p owns (p-1, p, p+1), whose
//      canonical key is (min(n[p-1], n[p+1]), n[p], max(..)) (profile.rs:672-678) in either orientation.  So the wave of a block
//      meets EVERY occurrence of every window whose middle lies in the block -- all haplotypes -- and count_per_trio == 1
//      (profile.rs:688-709) is decided in an LDS hash table keyed by (middle - block start, smaller end, larger end) packed into
//      64 bits.  Collinear haplotypes collapse in LDS; HBM sees the walks once (4P) and one bit per UNIQUE window.  A block whose
//      distinct windows overflow the table is redone in 2, 4, ... sub-passes over disjoint key classes (exact: all occurrences
//      of a key fall into the same class).
constexpr unsigned long long TB_EMPTY = ~0ull;
constexpr uint32_t TB_MULTI = 0xFFFFFFFFu;
constexpr int TB_UNR = 4;
// slot = {64-bit key, u32 q}: q is the position of the window's only occurrence, or TB_MULTI once a second one arrived
// (both sides use atomicMax, so the outcome does not depend on who comes first; positions are < 2^32 - 1)
template <int TB_SLOTS>
__device__ __forceinline__ void tb_insert(unsigned long long *s_key, uint32_t *s_q, uint32_t *s_over, uint32_t a_l, uint32_t b, uint32_t c,
                                          uint32_t q, uint32_t sub_mask, uint32_t sub_j) {
    const unsigned long long key = ((unsigned long long)a_l << 54) | ((unsigned long long)b << 27) | c;
    // hash of the key from full-rate 24-bit multiplies (a 64-bit multiply is four quarter-rate ones, and this kernel is bound
    // by VALU issue): b and c are the block's neighbours, their low bits carry the entropy; the full key decides equality
    uint32_t mix = __umul24(b, 0x9E3779u) + __umul24(c, 0x85EBCBu) + __umul24(a_l, 0x27D4EBu);
    mix ^= mix >> 13;
    if (((mix >> 16) & sub_mask) != sub_j) return;
    uint32_t h = mix & (TB_SLOTS - 1);
    for (int probes = 0; probes < TB_SLOTS; ++probes) {
        unsigned long long cur = s_key[h];
        if (cur == TB_EMPTY) cur = atomicCAS(&s_key[h], TB_EMPTY, key);
        if (cur == TB_EMPTY) { atomicMax(&s_q[h], q); return; }
        if (cur == key) { s_q[h] = TB_MULTI; return; }    // plain store of the maximum: nothing can undo it
        h = (h + 1) & (TB_SLOTS - 1);
    }
    *s_over = 1u;
}
// ONE WAVE per block of TRIO_BLK nodes (a workgroup is one wave: no workgroup barrier anywhere, two dozen independent
// waves per CU hide each other's trips to memory; a 256-thread workgroup per 256-node block spent most of its life in
// barriers and fixed overhead).  blk_rec[gb] = {first run, end run, global index of the block's first node, its
// species-local id / 64 | the block's node count << 24} (the blocks of one launch need not be neighbours: only the species the
// visit table leaves to this kernel have any).
template <int TB_SLOTS>
__global__ void __launch_bounds__(64) trio_block_kernel(const uint4 *__restrict__ blk_rec, const uint4 *__restrict__ runs,
                                                        const uint32_t *__restrict__ path_nodes, uint32_t *__restrict__ uniq_q,
                                                        uint32_t *__restrict__ first_cnt, uint32_t *__restrict__ err) {
    __shared__ unsigned long long s_key[TB_SLOTS];
    __shared__ uint32_t s_q[TB_SLOTS], s_ncnt[TRIO_BLK], s_over, s_pref[64];
    __shared__ uint4 s_run[64];
    const uint4 rec = blk_rec[blockIdx.x];
    const uint32_t nn = rec.w >> 24;                                    // nodes of the block (the last block of a species holds fewer than 64)
    const uint32_t r0 = rec.x, r1 = rec.y, n0 = (rec.w & 0xFFFFFFu) << TRIO_BLK_SHIFT;
    const uint32_t lane = threadIdx.x;
    for (uint32_t nsub = 1;; nsub <<= 1) {
        s_ncnt[lane] = 0;
        bool over = false;
        for (uint32_t j = 0; j < nsub && !over; ++j) {
            for (int i = lane; i < TB_SLOTS; i += 64) { s_key[i] = TB_EMPTY; s_q[i] = 0; }
            if (lane == 0) s_over = 0;
            __syncthreads();
            // the block's runs go to LDS 64 at a time; their positions are then handed out flat over the wave, TB_UNR per
            // lane and round, all loads of a round issued before the first table operation
            for (uint32_t rb = r0; rb < r1; rb += 64) {
                const uint32_t n_r = r1 - rb < 64u ? r1 - rb : 64u;
                uint4 run = make_uint4(0u, 0u, 0u, 0u);
                if (lane < n_r) run = runs[rb + lane];
                const uint32_t incl = wave_incl_scan_dpp(run.y);
                const uint32_t total = __shfl(incl, 63);
                s_run[lane] = run; s_pref[lane] = incl - run.y;
                __syncthreads();
                uint32_t lo_carry = 0;   // run of the last flat index handed out so far: the indices only grow, so does the run
                for (uint32_t idx0 = lane; idx0 < total; idx0 += 64 * TB_UNR) {
                    uint32_t x[TB_UNR], pp[TB_UNR], b1[TB_UNR], c1[TB_UNR];
                    bool md[TB_UNR];
#pragma unroll
                    for (int u = 0; u < TB_UNR; ++u) {
                        const uint32_t idx = idx0 + u * 64;
                        md[u] = false;
                        x[u] = pp[u] = b1[u] = c1[u] = 0u;
                        uint32_t lo = lo_carry;
                        if (idx < total) {
                            // last run whose first flat index is <= idx: a short walk forward from the previous group's last run
                            // (runs are mostly longer than a wave, so a group of 64 indices crosses one or two run borders;
                            // entries past the block's runs hold `total` and stop the walk)
                            while (lo < 63u && s_pref[lo + 1] <= idx) ++lo;
                            const uint4 rn = s_run[lo];
                            const uint32_t pos = rn.x + (idx - s_pref[lo]);
                            pp[u] = pos;
                            x[u] = path_nodes[pos];
                            md[u] = pos > rn.z && pos + 1 < rn.w;     // the middle of a window: a neighbour on either side inside the walk
                            if (md[u]) { b1[u] = path_nodes[pos - 1]; c1[u] = path_nodes[pos + 1]; }
                        }
                        lo_carry = __shfl(lo, 63);   // lane 63 holds the group's largest index (or, past the end, the carry itself)
                    }
#pragma unroll
                    for (int u = 0; u < TB_UNR; ++u) {
                        if (md[u]) tb_insert<TB_SLOTS>(s_key, s_q, &s_over, x[u] - n0, min(b1[u], c1[u]), max(b1[u], c1[u]), pp[u] - 1, nsub - 1, j);   // flagged at the window's START
                    }
                }
                __syncthreads();   // s_run / s_pref are reused by the next 64 runs
            }
            over = s_over != 0;
            if (!over)
                for (int i = lane; i < TB_SLOTS; i += 64) {
                    const unsigned long long k = s_key[i];
                    const uint32_t q = s_q[i];
                    if (k != TB_EMPTY && q != TB_MULTI) { uniq_mark(uniq_q, q); atomicAdd(&s_ncnt[(uint32_t)(k >> 54)], 1u); }
                }
            __syncthreads();
        }
        if (!over) break;
        if (nsub >= (1u << 20)) { if (lane == 0) atomicAdd(err, 1u); break; }   // cannot happen short of 2^31 equal hashes; never silent
    }
    __syncthreads();
    if (lane < nn) first_cnt[rec.z + lane] = s_ncnt[lane];
}

// 3v. THE DEFAULT (round 4): uniqueness through the VISIT TABLE -- the walks transposed.  All occurrences of a window share
//     its middle node b (window_of), so count_per_trio == 1 (profile.rs:688-709) is a question about the visits of b:
//     among all interior positions p with n[p] = b -- every haplotype of the species -- does the unordered pair
//     {n[p-1], n[p+1]} occur exactly once?  The visit table (trio_visits_build, once at upload: a layout of the walks like
//     the tile and run tables, the CSC to the walks' CSR) lists the interior positions node by node in groups of 64: a
//     node's visits never straddle a group (pads fill the tail), so ONE WAVE holds every visit of the handful of nodes of its
//     group; the visits of a node are kept sorted by their pair (an order of the table, like the order of an adjacency list), so
//     equal pairs are neighbours and lane l decides its window by comparing its pair with the lanes l - 1 and l + 1 of its node's
//     stretch -- no hash table, no LDS, no atomics, no loop on the way to the decision.  A step reads the table (4 B per visit) and
//     gathers the three consecutive walk entries of every visit (collinear haplotypes: the lanes of one haplotype read
//     neighbouring addresses, the lines are reused by the next groups of the wave).  A species that holds a node with more
//     than 64 interior visits (more than 64 haplotypes, or walks that keep returning to a node) is left to the node-block
//     kernel above; both write the same two outputs: one flag bit per window start and the count of unique windows per node.

// -DTV_ABLATE builds (never the product library) read PANTAX_TV_ABLATE: bit 0 no flag atomics, bit 1 no count stores, bit 2 no
// comparisons -- wrong results, for timing only
#ifdef TV_ABLATE
#define TV_ABL(bit) (ablate & (bit))
#else
#define TV_ABL(bit) false
#endif
// ROWS (the default): the wave hands its unique windows to trio_rows_kernel -- the group's ballot of unique visits and, for the first VIS_REC
// of them, a 16-byte record {window start, smaller end, larger end, middle (global node indices)}.  The rows of the index are then numbered IN
// THIS ORDER (round 5): a row = the rank of its visit among the unique visits of the table, i.e. a scan over the groups' counts (a tenth of the
// nodes) and one pass over the records -- no flag bit per path position, no ranks of flags, no scatter in (hap, position) order.  A group with more
// unique visits than records (one in seven at ten strains per species) is read again by trio_rows_kernel.
// !ROWS (option trio_rows=path; tests): one flag bit per unique window start + the count of unique windows per node, the inputs of the pass over
// the walks (trio_lookup_kernel) that also serves the species the visit table leaves to the node-block kernel.
template <int U, bool ROWS>
__global__ void __launch_bounds__(256) trio_visit_kernel(uint32_t NG, uint32_t rounds, const uint32_t *__restrict__ vis_pos, const uint64_t *__restrict__ vis_head,
                                                         const uint32_t *__restrict__ vis_nbase, const uint32_t *__restrict__ path_nodes,
                                                         uint32_t *__restrict__ uniq_q, uint32_t *__restrict__ first_cnt, uint32_t *__restrict__ err, uint32_t ablate,
                                                         unsigned long long *__restrict__ vis_uq, uint4 *__restrict__ vis_rec, uint32_t xcd_chunks) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // xcd_chunks != 0 (= the number of workgroups' worth of groups): workgroups go to the XCDs round-robin, so XCD x is given the x-th
    // contiguous eighth of the table -- neighbouring chunks read neighbouring lines of the same walks, and meet in ONE L2
    uint32_t blk = blockIdx.x;
    if (xcd_chunks) { blk = (blockIdx.x & 7u) * ((xcd_chunks + 7u) / 8u) + (blockIdx.x >> 3); if (blk >= xcd_chunks) blk = 0xFFFFFFu; }
    uint32_t g0 = blk == 0xFFFFFFu ? NG : (blk * 4u + wave) * ((uint32_t)U * rounds);      // this wave's U x rounds consecutive groups
    for (uint32_t r = 0; r < rounds && g0 < NG; ++r, g0 += U) {
        uint32_t q[U], nb[U];
        uint64_t heads[U];
        bool valid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g = g0 + (uint32_t)u < NG ? g0 + (uint32_t)u : g0;   // wave-uniform
            q[u] = vis_pos[(uint64_t)g * 64 + lane];
            heads[u] = vis_head[g]; nb[u] = vis_nbase[g];
        }
        __builtin_amdgcn_sched_barrier(0);       // all U table loads leave before the first of them is waited for
        U32x3 w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            valid[u] = g0 + (uint32_t)u < NG && q[u] != VIS_PAD;
            w[u] = *reinterpret_cast<const U32x3 *>(path_nodes + (valid[u] ? q[u] - 1u : 0u));   // an interior position: p - 1 and p + 1 exist
        }
        __builtin_amdgcn_sched_barrier(0);       // ... and all U gathers before the first decision
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t lo = min(w[u].x, w[u].z), hi = max(w[u].x, w[u].z);
            const unsigned long long vmask = __builtin_amdgcn_ballot_w64(valid[u]);
            const unsigned long long hd = heads[u] & vmask;
            // The visits of a node are SORTED by (smaller end, larger end) -- the table's order, fixed at upload -- so equal pairs sit in
            // neighbouring lanes: a window occurs once iff its pair differs from the pair of the lane below AND of the lane above
            // inside its node's stretch.  The order itself is checked on the way (a table that is not sorted is reported, never
            // silently trusted): one DPP shift and three compares per visit, no loop over the stretch.
            const unsigned long long inb = vmask & ~hd;                      // lanes with a lane of their own stretch below them
            const uint32_t slo = wave_shr1z(lo), shi = wave_shr1z(hi);       // the pair of the lane below (DPP moves)
            unsigned long long eq = __builtin_amdgcn_ballot_w64(slo == lo && shi == hi) & inb;
            if (TV_ABL(4u)) eq = 0ull;
            const unsigned long long bad = __builtin_amdgcn_ballot_w64(slo > lo || (slo == lo && shi > hi)) & inb;
            if (bad && lane == 0) atomicAdd(err, 1u);
            const unsigned long long dup = eq | (eq >> 1);                   // both partners are not unique
            const unsigned long long uq = vmask & ~dup;
            if (ROWS) {
                const uint32_t g = g0 + (uint32_t)u;
                if (g < NG) {
                    if (lane == 0) vis_uq[g] = uq;
                    const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(uq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)uq, 0u));   // unique visits in the lanes below
                    if (((uq >> lane) & 1ull) && rk < (uint32_t)VIS_REC && !TV_ABL(2u))
                        vis_rec[(uint64_t)g * VIS_REC + rk] = make_uint4(q[u] - 1u, nb[u] + lo, nb[u] + hi, nb[u] + w[u].y);
                }
            } else {
                if (((uq >> lane) & 1ull) && !TV_ABL(1u)) uniq_mark(uniq_q, q[u] - 1u);          // flagged at the window's start
                if (((hd >> lane) & 1ull) && !TV_ABL(2u)) {                                      // the head lane stores its node's count of unique windows
                    const unsigned long long he = hd | (~vmask & (vmask + 1ull));   // the first pad lane closes the last stretch (pads sit at the tail)
                    const unsigned long long above = he & ~((2ull << lane) - 1ull);
                    const int end = above ? __builtin_ctzll(above) : 64;
                    const unsigned long long m = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
                    first_cnt[nb[u] + w[u].y] = (uint32_t)__popcll(uq & m);
                }
            }
        }
    }
}

// ---- the brackets of trio_index_build ----
// every wave walks U x rounds consecutive groups of 64 visits (tv_u / tv_rounds pick another shape, for
// measurements): consecutive groups visit consecutive nodes, whose walk entries share cache lines
template <int U, bool ROWS>
static void visit_launch(Ctx *ctx, Db *db, const TrioGroupGrid &g) {
    TrioScratch &ts = db->trio_scratch;
    hipLaunchKernelGGL((trio_visit_kernel<U, ROWS>), dim3(g.grid), dim3(256), 0, ctx->stream, db->n_vgroups, g.rounds, db->d_vis_pos.p, db->d_vis_head.p, db->d_vis_nbase.p,
                       db->d_path_nodes.p, ts.uniq_q.p, ts.first_cnt.p, ts.d_tot.p + 2, ctx->cfg.tv_ablate /* -DTV_ABLATE builds only */,
                       reinterpret_cast<unsigned long long *>(ts.vis_uq.p), ts.vis_rec.p, g.xcd_chunks);
}
int trio_visit_launch(Ctx *ctx, Db *db, const TrioPlan &pl) {
    KTimer t(ctx, "trio_visit_kernel");
    const TrioGroupGrid &g = pl.visit;
    if (pl.rows_by_visit) {
        if (g.u == 2) visit_launch<2, true>(ctx, db, g);
        else if (g.u == 4) visit_launch<4, true>(ctx, db, g);
        else if (g.u == 8) visit_launch<8, true>(ctx, db, g);
        else return fail(ctx, PANTAX_HIP_E_STATE, "trio_index: no trio_visit_kernel of %u groups in flight", g.u);
    } else {
        if (g.u == 2) visit_launch<2, false>(ctx, db, g);
        else if (g.u == 4) visit_launch<4, false>(ctx, db, g);
        else if (g.u == 8) visit_launch<8, false>(ctx, db, g);
        else return fail(ctx, PANTAX_HIP_E_STATE, "trio_index: no trio_visit_kernel of %u groups in flight", g.u);
    }
    return 0;
}

// LDS table slots per 64-node block (tb_slots = 512 | 256 | 128 picks another instantiation, for measurements): fewer
// slots = more blocks resident per CU (the kernel is bound by the latency of each wave's dependent loads), more blocks
// that need sub-passes
template <int SLOTS>
static void block_launch(Ctx *ctx, Db *db) {
    TrioScratch &ts = db->trio_scratch;
    hipLaunchKernelGGL(trio_block_kernel<SLOTS>, dim3(db->n_blocks), dim3(64), 0, ctx->stream, db->d_blk_rec.p, db->d_runs.p, db->d_path_nodes.p, ts.uniq_q.p, ts.first_cnt.p,
                       ts.d_tot.p + 2);
}
int trio_block_launch(Ctx *ctx, Db *db, const TrioPlan &pl) {
    KTimer t(ctx, "trio_block_kernel");
    if (pl.tb_slots == 512) block_launch<512>(ctx, db);
    else if (pl.tb_slots == 256) block_launch<256>(ctx, db);
    else if (pl.tb_slots == 128) block_launch<128>(ctx, db);
    else return fail(ctx, PANTAX_HIP_E_STATE, "trio_index: no trio_block_kernel of %d slots", pl.tb_slots);
    return 0;
}

// the bucket path: count -> scan -> fill -> the uniqueness test of every window against its bucket (pl.n_win windows: every hap with len >= 3
// contributes len - 2)
int trio_bucket_launch(Ctx *ctx, Db *db, const TrioPlan &pl) {
    TrioScratch &ts = db->trio_scratch;
    const uint64_t V = db->V, n_win = pl.n_win;
    const dim3 tgrid((uint32_t)db->n_tiles);
    PTX_HIP(ctx, ts.bucket.alloc(db->P));
    {
        KTimer t(ctx, "trio_count_kernel");
        hipLaunchKernelGGL(trio_count_kernel, tgrid, dim3(256), 0, ctx->stream, TRIO_GRAPH(db), ts.cnt.p);
    }
    PTX_TRY(exclusive_scan_u32(ctx, ts.cnt.p, ts.bucket_off.p, V + 1, ts.scan_tmp.p, ts.d_tot.p));
    {
        KTimer t(ctx, "trio_fill_kernel");
        hipLaunchKernelGGL(trio_fill_kernel, tgrid, dim3(256), 0, ctx->stream, TRIO_GRAPH(db), ts.bucket_off.p, ts.cursor.p, ts.bucket.p);
    }
    if (pl.run_uniq) {
        KTimer t(ctx, "trio_uniq_kernel");
        if (pl.uniq_hashed)
            hipLaunchKernelGGL(trio_uniq_lds_kernel, dim3((uint32_t)((n_win + UNIQ_CH - 1) / UNIQ_CH)), dim3(256), 0, ctx->stream, n_win, (uint32_t)V,
                               ts.bucket.p, ts.bucket_off.p, ts.uniq_q.p, ts.first_cnt.p);
        else
            hipLaunchKernelGGL(trio_uniq_kernel, dim3(grid_for(n_win, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, n_win, ts.bucket.p,
                               ts.bucket_off.p, ts.uniq_q.p, ts.first_cnt.p);
    }
    return 0;
}

}  // namespace ptx
