// stage_trio_rows.hip -- filing the rows of the unique-trio index (a7): a row is a unique window, numbered by the place it is filed at (trio_device.hpp).
//   FAST route (species of the visit table): the groups' counts of unique visits -> prefix (group_tile_* kernels) -> trio_rows_kernel files the
//   visit kernel's records; a REBUILD of a db whose group offsets are known decides and files in one pass (trio_file_kernel).
//   PATH route (the other species; the whole db under trio_path=bucket / trio_rows=path): flags + per-node counts -> scan of the counts (heads)
//   -> trio_lookup_kernel -> trio_canon_kernel.  In a mixed db the path route's rows follow the fast route's.
// The host launch functions at the end are the phases trio_index_build (stage_trio.hip) calls.
#include <algorithm>
#include "trio_device.hpp"
#include "scan_chained.hpp"

namespace ptx {

// ---- PATH ROUTE: rows filed by a pass over the walks (species the visit table leaves to the node-block kernel; whole databases on the
// bucket path or under the options trio_path / trio_rows).  Its inputs are one flag bit per unique window start and the count of unique
// windows per node; a scan of the counts gives every node its block of rows (and its lookup head), the pass over the walks drops every unique
// window into its node's block in ARRIVAL order, and trio_canon_kernel then puts every block into the canonical order -- sorted by the pair
// of ends, which is distinct inside a node by the very definition of a unique window -- and files the rows.
// `only_slow` (mixed databases): only the tiles of the species left to the node-block kernel.
__global__ void __launch_bounds__(256) trio_lookup_kernel(TRIO_GRAPH_ARGS, const uint32_t *__restrict__ uniq_q, const uint32_t *__restrict__ trio_first,
                                                          uint32_t *__restrict__ cursor /* = the per-node counts; zero afterwards */, uint2 *__restrict__ trio_ent,
                                                          uint32_t *__restrict__ row_q, const uint32_t *__restrict__ only_slow) {
    constexpr int NR = PATH_TILE / 256;   // rounds of 256 consecutive positions
    __shared__ uint32_t s_wave[NR][4];
    const uint2 tile = tiles[blockIdx.x];
    if (tile.x == 0xFFFFFFFFu) return;   // filler tile
    const uint32_t h = tile.x;
    const uint64_t qend = path_off[h + 1], qt0 = path_off[h] + (uint64_t)tile.y * PATH_TILE;
    const uint32_t sidx = hap_species[h], nbase = node_base[sidx];
    if (only_slow && !only_slow[sidx]) return;                   // a species of the visit table
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // all rounds at once: the flags of the four rounds are loaded together, ONE barrier orders the wave counts, and the
    // gathers / writes of the unique windows of all rounds are in flight together
    uint32_t u[NR];
    unsigned long long bal[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const uint64_t q = qt0 + (uint64_t)r * 256 + threadIdx.x;
        u[r] = (q < qend) ? (uniq_q[q >> 5] >> (uint32_t)(q & 31ull)) & 1u : 0u;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        bal[r] = __ballot(u[r] != 0);
        if (lane == 0) s_wave[r][wave] = (uint32_t)__popcll(bal[r]);
    }
    __syncthreads();
    // The unique windows are a few per cent of the positions: they are compacted into an LDS list first, and the gathers / scatters of a
    // window then run on DENSE lanes
    __shared__ uint16_t s_list[PATH_TILE];
    uint32_t n_u = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        uint32_t woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const uint32_t t = s_wave[r][w]; if (w < wave) woff += t; tot += t; }
        if (u[r]) s_list[n_u + woff + (uint32_t)__popcll(bal[r] & ((1ull << lane) - 1ull))] = (uint16_t)(r * 256 + (int)threadIdx.x);
        n_u += tot;
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < n_u; t += 256) {
        const uint64_t q = qt0 + s_list[t];
        uint32_t g, a, b, c;
        window_of(q, qend, nbase, path_nodes, g, a, b, c);
        const uint32_t j = trio_first[g] + atomicSub(&cursor[g], 1u) - 1u;   // the node's own count, counted down: no cursor array to zero
        trio_ent[j] = make_uint2(nbase + a, nbase + c);                      // global node indices: the coverage pass works in them throughout
        row_q[j] = (uint32_t)q;
    }
}
// one thread per node that heads rows (path route): its block of rows sorted by (smaller end, larger end) -- insertion sort, a handful of rows;
// a hub of a thousand distinct neighbour pairs is a millisecond of one thread at load time -- and filed
template <bool KEYS, bool FIRST>
__global__ void __launch_bounds__(256) trio_canon_kernel(uint64_t V, uint32_t S, const uint32_t *__restrict__ node_base, const uint4 *__restrict__ node_rec,
                                                         const uint32_t *__restrict__ trio_first, const uint32_t *__restrict__ visited,
                                                         const uint32_t *__restrict__ only_slow, uint32_t *__restrict__ row_q, RowOut o) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    if (visited && !((visited[v >> 5] >> (uint32_t)(v & 31ull)) & 1u)) return;
    const uint32_t n = nr_rows(node_rec[v].y);
    if (n == 0) return;
    uint32_t lo = 0, hi = S;                                             // last s with node_base[s] <= v
    while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)node_base[mid] <= v) lo = mid; else hi = mid; }
    const uint32_t sp = lo;
    if (only_slow && !only_slow[sp]) return;                             // a species of the visit table: trio_rows_kernel files its rows
    const uint32_t f = trio_first[v];
    for (uint32_t i = 1; i < n; ++i) {
        const uint2 e = o.ent[f + i];
        const uint32_t q = row_q[f + i];
        uint32_t j = i;
        for (; j > 0; --j) {
            const uint2 p = o.ent[f + j - 1];
            if (p.x < e.x || (p.x == e.x && p.y <= e.y)) break;
            o.ent[f + j] = p; row_q[f + j] = row_q[f + j - 1];
        }
        if (j != i) { o.ent[f + j] = e; row_q[f + j] = q; }
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint2 e = o.ent[f + i];
        row_file<KEYS, FIRST>(o, f + i, row_q[f + i], e.x, e.y, (uint32_t)v, sp, HapCount{nullptr, 0u, o.hap_cnt});
    }
}

// scan of the per-node unique-window counts that also writes the lookup heads {first row, #rows} (CSR over the
// middle node) -- the prefix and its consumer in one launch
// `visited` (visit-table / node-block builds): a node without an interior visit is the middle of no window and no kernel of the
// build stores its count -- it reads as zero here instead of being zero-filled before every build (4V bytes)
struct TrioFirstLoad {
    const uint32_t *cnt, *visited;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
        if (visited && !((visited[i >> 5] >> (uint32_t)(i & 31ull)) & 1u)) return 0u;
        return cnt[i];
    }
};
// mixed databases: the lookup heads of the species left to the node-block kernel, filed BEHIND the rows of the visit table's species (row base
// = *u_fast, the total of the groups' counts); a node of a visit-table species reads as zero here
struct SlowFirstLoad {
    const uint32_t *cnt, *visited, *slow;
    const uint2 *tile_sp;
    const uint32_t *node_base;
    uint64_t V;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
        if (i >= V) return 0u;
        const uint2 t = tile_sp[i >> 11];
        uint32_t sp = t.x;
        while (sp < t.y && node_base[sp + 1] <= i) ++sp;
        if (!slow[sp] || !((visited[i >> 5] >> (uint32_t)(i & 31ull)) & 1u)) return 0u;
        return cnt[i];
    }
};
struct SlowFirstStore {
    uint32_t *first;
    uint4 *node_rec;
    uint64_t V;
    const uint32_t *u_fast;
    uint32_t *err;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t excl, uint32_t c) const {
        if (i < V && c) {                                  // (trio_first is written for the nodes that have rows: what the lookup pass reads)
            const uint32_t f = *u_fast + excl;
            first[i] = f;
            if (c >= NODE_REC_MAX_ROWS) atomicAdd(err, 1u);
            uint4 r = node_rec[i];
            const uint32_t y_new = nr_head(r.y, c, 0xFFu);
            if (r.y != y_new || r.w != f) { r.y = y_new; r.w = f; node_rec[i] = r; }
        }
    }
};
struct TrioFirstStore {
    uint32_t *first;
    uint4 *node_rec;   // the head {first row, #rows} rides in the node record the coverage kernel gathers anyway
    uint64_t V;
    uint32_t *err;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t excl, uint32_t c) const {
        first[i] = excl;
        // Only nodes that head unique windows carry a lookup head (8 % of them): which nodes those are and how many rows they head
        // is a function of the graphs alone, so every rebuild writes the same values -- a node without rows keeps the "0 rows" of its
        // upload-time record and is not touched (round 2 read and rewrote all V records per build: 32 bytes of traffic per node).
        if (i < V && c) {
            if (c >= NODE_REC_MAX_ROWS) atomicAdd(err, 1u);
            uint4 r = node_rec[i];
            const uint32_t y_new = nr_head(r.y, c, 0xFFu);   // this route does not compute the pair filter
            if (r.y != y_new || r.w != excl) { r.y = y_new; r.w = excl; node_rec[i] = r; }
        }
    }
};

// ---- FAST ROUTE: the rows of the species the visit table covers, filed from trio_visit_kernel<.., ROWS = true>'s records ----
// the first row of every group = the prefix of the groups' counts of unique visits, in three plain launches (tile sums, a scan of the sums
// by one workgroup, tile prefixes): a chained scan's workgroups spin on their predecessors, and beside the main stream's kernels of the step in
// flight that spinning stretched a 0.34-ms scan to 2.5 ms (and held the slots it spun in) -- the rebuild of the NEXT step runs beside the
// current step's row sort and LPs
struct GroupCountLoad { const unsigned long long *uq; __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return (uint32_t)__popcll(uq[i]); } };
struct PrefixStore { uint32_t *out; __device__ __forceinline__ void operator()(uint64_t i, uint32_t excl, uint32_t) const { out[i] = excl; } };
constexpr int FR_WORDS = 16, FR_TILE = 256 * FR_WORDS;           // counts per thread and per workgroup
__global__ void __launch_bounds__(1024) tile_scan_kernel(uint32_t *__restrict__ sums, uint32_t n_tiles, uint32_t *__restrict__ total) {
    __shared__ uint32_t s_wave[16];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += 1024) {
        const uint32_t i = base + threadIdx.x, v = i < n_tiles ? sums[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan<1024>(v, s_wave, &tot);
        if (i < n_tiles) sums[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0 && total) *total = carry;
}
// (element i of a tile = stretch k, thread t: i = k * 256 + t -- coalesced loads and stores; a stretch's prefix = one DPP scan per wave
// + the four wave sums through LDS)
template <class Count, class Emit>
__device__ __forceinline__ void tile_prefix(uint64_t n, uint32_t start, Count count, Emit emit) {
    __shared__ uint32_t s_w[2][4];
    const uint64_t base = (uint64_t)blockIdx.x * FR_TILE;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t run = start;
#pragma unroll 4
    for (int k = 0; k < FR_WORDS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256 + threadIdx.x;
        const uint32_t c = i < n ? count(i) : 0u;
        const uint32_t incl = wave_incl_scan_dpp(c);
        if (lane == 63) s_w[k & 1][wave] = incl;
        __syncthreads();
        uint32_t woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const uint32_t t = s_w[k & 1][w]; woff += w < (int)wave ? t : 0u; tot += t; }
        if (i < n) emit(i, run + woff + incl - c);
        run += tot;
    }
}
__global__ void __launch_bounds__(256) group_tile_sum_kernel(const unsigned long long *__restrict__ uq, uint64_t n, uint32_t *__restrict__ sums) {
    __shared__ uint32_t s_w[4];
    const uint64_t base = (uint64_t)blockIdx.x * FR_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < FR_WORDS; ++k) { const uint64_t i = base + (uint64_t)k * 256 + threadIdx.x; if (i < n) c += (uint32_t)__popcll(uq[i]); }
    c = wave_reduce(c, [](uint32_t x, uint32_t y) { return x + y; });
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
__global__ void __launch_bounds__(256) group_tile_prefix_kernel(const unsigned long long *__restrict__ uq, uint64_t n, const uint32_t *__restrict__ sums, uint32_t *__restrict__ out) {
    tile_prefix(n, sums[blockIdx.x], [&](uint64_t i) { return (uint32_t)__popcll(uq[i]); }, [&](uint64_t i, uint32_t excl) { out[i] = excl; });
}

// the lookup head of a node = {its first row, the number of its rows}, written into the node record by the lane that holds the
// node's first unique window (records arrive in visit order: a node's windows are neighbours); `cnt` = rows of this node
__device__ __forceinline__ void trio_head_store(uint4 *__restrict__ node_rec, uint32_t v, uint32_t row, uint32_t cnt, uint32_t filter, uint32_t *__restrict__ err) {
    if (cnt >= NODE_REC_MAX_ROWS) atomicAdd(err, 1u);
    uint4 r = node_rec[v];
    const uint32_t y_new = nr_head(r.y, cnt, filter);
    if (r.y != y_new || r.w != row) { r.y = y_new; r.w = row; node_rec[v] = r; }   // (stored only where it is not there yet: see trio_rows_kernel)
}
// a group with more than VIS_REC unique visits (a stretch of private sequence; every group of a single-strain species): the whole wave
// reads the group's visits again, ranks the unique ones, and files them like the records
template <bool KEYS, bool FIRST>
__device__ __forceinline__ void trio_rows_group(uint32_t g, int lane, const unsigned long long *__restrict__ vis_uq, const uint32_t *__restrict__ gprefix,
                                                const uint32_t *__restrict__ vis_pos, const uint32_t *__restrict__ vis_nbase, const uint32_t *__restrict__ vis_sp,
                                                const uint32_t *__restrict__ path_nodes, uint4 *__restrict__ node_rec, const RowOut &o, uint32_t *__restrict__ err,
                                                const HapCount &hc) {
    const unsigned long long uq = vis_uq[g];
    const uint32_t nb = vis_nbase[g], sp = vis_sp[g], base = gprefix[g];
    const bool mine = (uq >> lane) & 1ull;
    uint4 rec = make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);
    if (mine) {
        const uint32_t q = vis_pos[(uint64_t)g * 64 + lane];
        const U32x3 w = *reinterpret_cast<const U32x3 *>(path_nodes + (q - 1u));
        rec = make_uint4(q - 1u, nb + min(w.x, w.z), nb + max(w.x, w.z), nb + w.y);
    }
    const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(uq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)uq, 0u));
    // first unique visit of its node: the unique lane below holds another node (the visits of a node are neighbours)
    const unsigned long long lower = uq & ((1ull << lane) - 1ull);
    const uint32_t prev_w = __shfl(rec.w, lower ? 63 - __builtin_clzll(lower) : lane);
    const bool first = mine && (!lower || prev_w != rec.w);
    const unsigned long long fm = __ballot(first);
    if (mine) row_file<KEYS, FIRST>(o, base + r, rec.x, rec.y, rec.z, rec.w, sp, hc);
    // the node's rows end at the next first lane; its pair filter = OR of the bits of its unique lanes (every first lane walks its span: a node's
    // unique visits, a handful; all lanes reach the shuffles)
    const uint32_t pbit = mine ? nr_pair_bit(rec.y, rec.z) : 0u;
    const unsigned long long nxt = fm & ~((2ull << lane) - 1ull);
    const unsigned long long span = uq & ~((1ull << lane) - 1ull) & (nxt ? (1ull << __builtin_ctzll(nxt)) - 1ull : ~0ull);
    uint32_t filt = 0u;
    unsigned long long sp_ = first ? span : 0ull;
    while (__any(sp_ != 0ull)) {
        const int l = sp_ ? __builtin_ctzll(sp_) : 0;
        const uint32_t ob = __shfl(pbit, l);
        if (sp_) { filt |= ob; sp_ &= sp_ - 1ull; }
    }
    if (first) trio_head_store(node_rec, rec.w, base + r, (uint32_t)__popcll(span), filt, err);
}
// EIGHT groups per batch, lane = (group, record): the records of a group that did not overflow (<= VIS_REC unique visits) are read as
// one coalesced kilobyte per batch; the row of record r of group g is the scan of the groups' counts + r.  A wave takes U batches at
// once, level by level -- counts, records, then the gathers every record depends on (three node lengths, its species' walk offsets, the node
// record its head goes into) -- so that U x the loads are in flight per wave.  Every store is dense in row order except the heads.
template <bool KEYS, bool FIRST, int U>
__global__ void __launch_bounds__(256) trio_rows_kernel(uint32_t NG, const unsigned long long *__restrict__ vis_uq, const uint32_t *__restrict__ gprefix,
                                                        const uint4 *__restrict__ vis_rec, const uint32_t *__restrict__ vis_nbase, const uint32_t *__restrict__ vis_sp,
                                                        const uint32_t *__restrict__ vis_pos, const uint32_t *__restrict__ path_nodes,
                                                        uint4 *__restrict__ node_rec, RowOut o, uint32_t *__restrict__ err, uint32_t xcd_chunks, uint32_t iters) {
    static_assert(VIS_REC == 8, "eight lanes per group");
    const int lane = threadIdx.x & 63;
    // FIRST builds: a workgroup takes `iters` consecutive chunks and counts the rows per haplotype in LDS (HapCount)
    __shared__ uint32_t s_hapcnt[FIRST ? HAPCNT_WIN : 1];
    HapCount hc{nullptr, 0u, o.hap_cnt};
    if (FIRST) {
        for (uint32_t i = threadIdx.x; i < HAPCNT_WIN; i += blockDim.x) s_hapcnt[i] = 0u;
        const uint32_t gfirst = blockIdx.x * iters * 32u * (uint32_t)U;
        hc.lds = s_hapcnt; hc.base = (uint32_t)o.hap_off[vis_sp[gfirst < NG ? gfirst : NG - 1u]];
        __syncthreads();
    }
    for (uint32_t it = 0; it < iters; ++it) {
    uint32_t blk = blockIdx.x * iters + it;          // xcd_chunks != 0 (rebuilds, iters == 1): every XCD files one contiguous eighth of the groups (see trio_visit_kernel)
    if (xcd_chunks) { blk = (blockIdx.x & 7u) * ((xcd_chunks + 7u) / 8u) + (blockIdx.x >> 3); if (blk >= xcd_chunks) break; }
    const uint32_t r = (uint32_t)lane & 7u;
    uint32_t g[U], cnt[U], row[U], sp[U];
    // ---- level 1: the groups' counts, first rows and species
#pragma unroll
    for (int u = 0; u < U; ++u) {
        g[u] = ((blk * 4u + (threadIdx.x >> 6)) * (uint32_t)U + (uint32_t)u) * 8u + ((uint32_t)lane >> 3);
        cnt[u] = 0; row[u] = 0; sp[u] = 0;
        if (g[u] < NG) { cnt[u] = (uint32_t)__popcll(vis_uq[g[u]]); row[u] = gprefix[g[u]] + r; sp[u] = vis_sp[g[u]]; }
    }
    // ---- level 2: the records
    uint4 rec[U];
    bool on[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        on[u] = cnt[u] <= (uint32_t)VIS_REC && r < cnt[u];                     // an overflowing group is taken whole, below
        rec[u] = make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);
        if (on[u]) rec[u] = vis_rec[(uint64_t)g[u] * VIS_REC + r];
    }
    // the owner of a window = the haplotype whose walk holds its start.  The eight groups of a batch nearly always belong to ONE species: the
    // walk offsets of that species' haplotypes (up to 64) are loaded once, lane j holds offset j, and every lane counts the offsets at or
    // below its position by reading them lane after lane -- ALU work beside the record loads instead of a binary search of four dependent
    // loads behind them (the kernel waits for memory: every level of the chain shows).  Lanes of another species take the search.
    uint32_t sp0[U], h00[U], hs0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long live = __ballot(g[u] < NG);
        sp0[u] = (uint32_t)__builtin_amdgcn_readlane((int)sp[u], live ? __builtin_ctzll(live) : 0);
        h00[u] = (uint32_t)o.hap_off[sp0[u]]; hs0[u] = (uint32_t)o.hap_off[sp0[u] + 1] - h00[u];
    }
    // ---- level 3: what every record points at
    uint32_t len3[U], woff[U];
    uint4 nrv[U];
    bool first[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // first record of its node: the record below belongs to another node (or to another group)
        const uint32_t below = wave_shr1(rec[u].w, 0xFFFFFFFFu);
        first[u] = on[u] && (r == 0u || below != rec[u].w);
        len3[u] = 0; nrv[u] = make_uint4(0u, 0u, 0u, 0u);
        woff[u] = ((uint32_t)lane < hs0[u] && hs0[u] <= 64u) ? (uint32_t)o.path_off[h00[u] + (uint32_t)lane] : 0xFFFFFFFFu;   // P < 2^32
        if (on[u]) len3[u] = o.node_len[rec[u].y] + o.node_len[rec[u].w] + o.node_len[rec[u].z];
        if (first[u]) nrv[u] = node_rec[rec[u].w];
    }
    // ---- the rows, the heads
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long fm = __ballot(first[u]), om = __ballot(on[u]);
        uint32_t hl = 0;                                                     // owner within the species: offsets at or below the position, minus one
        if (hs0[u] <= 64u) {
            for (uint32_t j = 1; j < hs0[u]; ++j) hl += (uint32_t)__builtin_amdgcn_readlane((int)woff[u], (int)j) <= rec[u].x ? 1u : 0u;
        }
        if (on[u]) {
            uint32_t hb = h00[u];
            if (hs0[u] > 64u || sp[u] != sp0[u]) {                           // a species of more than 64 haplotypes, or not the batch's first species
                hb = (uint32_t)o.hap_off[sp[u]];
                hl = hap_of_position(o.path_off, hb, (uint32_t)o.hap_off[sp[u] + 1], rec[u].x) - hb;
            }
            o.ent[row[u]] = make_uint2(rec[u].y, rec[u].z);
            o.put_len_hap(row[u], len3[u], hl);
            if (KEYS) o.q[row[u]] = rec[u].x;
            if (FIRST) hc.add(hb + hl);
        }
        // the pair filter of a node = OR of its rows' bits: the rows of a node are neighbouring lanes (at most eight)
        const uint32_t pbit = on[u] ? nr_pair_bit(rec[u].y, rec[u].z) : 0u;
        uint32_t filt = pbit;
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            const uint32_t ob = __shfl(pbit, (lane + d) & 63), ow = __shfl(rec[u].w, (lane + d) & 63);
            if (((lane & 7) + d) < 8 && ow == rec[u].w) filt |= ob;
        }
        if (first[u]) {
            // rows of the node: up to the next first record, or to the end of the group's records
            const unsigned long long grp = 0xFFull << (lane & ~7), stop = (fm | ~om) & grp & ~((2ull << lane) - 1ull);
            const int end = stop ? __builtin_ctzll(stop) : (lane & ~7) + 8;
            const uint32_t rows = (uint32_t)(end - lane);
            if (rows >= NODE_REC_MAX_ROWS) atomicAdd(err, 1u);
            // the head of a node is a function of the graphs alone: every rebuild computes it again, and STORES it only where the record does
            // not hold it yet (the first build of a db) -- a 16-byte store into a line of eight records dirties a 64-byte sector, and the heads
            // of 1e4 strains were 4.5 of the 7.4 GB this kernel wrote per build (`r05_pmc_trio_probe`)
            uint4 nr = nrv[u];
            const uint32_t y_new = nr_head(nr.y, rows, filt);
            if (nr.y != y_new || nr.w != row[u]) { nr.y = y_new; nr.w = row[u]; node_rec[rec[u].w] = nr; }
        }
    }
    // the groups of this wave with more unique visits than records, one after the other
#pragma unroll
    for (int u = 0; u < U; ++u) {
        unsigned long long ov = __ballot(r == 0u && cnt[u] > (uint32_t)VIS_REC);
        while (ov) {
            const int l = __builtin_ctzll(ov);
            ov &= ov - 1ull;
            trio_rows_group<KEYS, FIRST>(g[u] - ((uint32_t)lane >> 3) + ((uint32_t)l >> 3), lane, vis_uq, gprefix, vis_pos, vis_nbase, vis_sp, path_nodes, node_rec, o, err, hc);
        }
    }
    }   // iters
    if (FIRST) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < HAPCNT_WIN; i += blockDim.x) { const uint32_t c = s_hapcnt[i]; if (c) atomicAdd(&o.hap_cnt[hc.base + i], c); }
    }
}

// ---- REBUILDS of a db whose group offsets are known: uniqueness and filing in ONE pass over the visit table -------------------------------
// The first row of every group of 64 visits (gprefix) is a function of the graphs alone, like the group boundaries of the visit table themselves:
// the db's first build learns it (trio_visit_kernel<ROWS> -> prefix of the groups' counts -> trio_rows_kernel) and keeps it with the table.  Every
// later build -- the per-run rebuild of a resident step, profile.rs:2936 -- decides the uniqueness of every window again and files every row again,
// in the kernel that took the decision: no records through memory, no scan, no second kernel.  The offsets are VERIFIED on the way: a group whose
// count of unique visits is not what its neighbours' offsets say raises the error word (it comes back with the step's results).
// A group holds about five unique visits, so filing from the deciding lanes would run everything behind the decision at a twelfth of the lanes (first
// version: 14.6 ms at 1e4 strains against 5.6 + 7.0 for the two kernels -- the kernel is bound by VALU issue, 64-lane instructions per group).  Instead
// every wave QUEUES its unique windows in LDS -- consecutive groups of one species have consecutive rows -- and files the queue on dense lanes, lane =
// row, whenever the next group would not fit: coalesced stores of 64 consecutive rows, one pass over the species' walk offsets per ~12 groups.
struct FileQueue {
    uint4 rec[64];       // {window start, smaller end, larger end, middle} (global node indices), in visit order = row order
};
template <bool KEYS>
__device__ __forceinline__ void trio_file_flush(const FileQueue &qu, uint32_t cnt, uint32_t row0, uint32_t sp, int lane, uint4 *__restrict__ node_rec, const RowOut &o,
                                                uint32_t *__restrict__ err) {
    const bool on = (uint32_t)lane < cnt;
    const uint4 rec = on ? qu.rec[lane] : make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);
    const uint32_t h0 = (uint32_t)o.hap_off[sp], hs = (uint32_t)o.hap_off[sp + 1] - h0;      // wave-uniform
    // the owner of a window = the haplotype whose walk holds its start: the species' walk offsets (up to 64) sit one per lane and every lane counts those
    // at or below its start (trio_rows_kernel)
    const uint32_t woff = ((uint32_t)lane < hs && hs <= 64u) ? (uint32_t)o.path_off[h0 + (uint32_t)lane] : 0xFFFFFFFFu;   // P < 2^32
    // first row of its node: the row below belongs to another node (a node's unique visits are neighbours, and groups -- hence queues -- hold whole nodes)
    const uint32_t below = wave_shr1(rec.w, 0xFFFFFFFFu);
    const bool first = on && (lane == 0 || below != rec.w);
    uint32_t len3 = 0;
    uint4 nrv = make_uint4(0u, 0u, 0u, 0u);
    if (on) len3 = o.node_len[rec.y] + o.node_len[rec.w] + o.node_len[rec.z];
    if (first) nrv = node_rec[rec.w];
    const unsigned long long fm = __ballot(first), om = __ballot(on);
    uint32_t hl = 0;
    if (hs <= 64u) { for (uint32_t j = 1; j < hs; ++j) hl += (uint32_t)__builtin_amdgcn_readlane((int)woff, (int)j) <= rec.x ? 1u : 0u; }
    const uint32_t row = row0 + (uint32_t)lane;
    if (on) {
        if (hs > 64u) hl = hap_of_position(o.path_off, h0, h0 + hs, rec.x) - h0;
        o.ent[row] = make_uint2(rec.y, rec.z);
        o.put_len_hap(row, len3, hl);
        if (KEYS) o.q[row] = rec.x;
    }
    // the node's rows end at the next first lane; its pair filter = OR of its rows' bits (every first lane walks its span: a handful of lanes)
    const uint32_t pbit = on ? nr_pair_bit(rec.y, rec.z) : 0u;
    const unsigned long long nxt = (fm | ~om) & ~((2ull << lane) - 1ull);
    const int end = nxt ? __builtin_ctzll(nxt) : 64;
    const unsigned long long span = first ? ((end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull)) : 0ull;
    uint32_t filt = 0u;
    unsigned long long sp_ = span;
    while (__any(sp_ != 0ull)) {
        const int l = sp_ ? __builtin_ctzll(sp_) : 0;
        const uint32_t ob = __shfl(pbit, l);
        if (sp_) { filt |= ob; sp_ &= sp_ - 1ull; }
    }
    if (first) {
        const uint32_t rows = (uint32_t)(end - lane);
        if (rows >= NODE_REC_MAX_ROWS) atomicAdd(err, 1u);
        uint4 nr = nrv;
        const uint32_t y_new = nr_head(nr.y, rows, filt);
        if (nr.y != y_new || nr.w != row) { nr.y = y_new; nr.w = row; node_rec[rec.w] = nr; }   // (stored only where it is not there yet: trio_rows_kernel)
    }
}
template <int U, bool KEYS>
__global__ void __launch_bounds__(256) trio_file_kernel(uint32_t NG, uint32_t rounds, const uint32_t *__restrict__ vis_pos, const uint64_t *__restrict__ vis_head,
                                                        const uint32_t *__restrict__ vis_nbase, const uint32_t *__restrict__ vis_sp, const uint32_t *__restrict__ gprefix,
                                                        const uint32_t *__restrict__ path_nodes, uint4 *__restrict__ node_rec, RowOut o, uint32_t *__restrict__ err,
                                                        uint32_t xcd_chunks) {
    __shared__ FileQueue queues[4];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    FileQueue &qu = queues[wave];
    uint32_t blk = blockIdx.x;
    if (xcd_chunks) { blk = (blockIdx.x & 7u) * ((xcd_chunks + 7u) / 8u) + (blockIdx.x >> 3); if (blk >= xcd_chunks) blk = 0xFFFFFFu; }
    uint32_t g0 = blk == 0xFFFFFFu ? NG : (blk * 4u + wave) * ((uint32_t)U * rounds);      // this wave's U x rounds consecutive groups
    uint32_t q_cnt = 0, q_row0 = 0, q_sp = 0;                                              // the queue: entries, row of the first, their species (wave-uniform)
    for (uint32_t r = 0; r < rounds && g0 < NG; ++r, g0 += U) {
        uint32_t q[U], nb[U], sp[U], base[U], want[U];
        uint64_t heads[U];
        bool valid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g = g0 + (uint32_t)u < NG ? g0 + (uint32_t)u : g0;   // wave-uniform
            q[u] = vis_pos[(uint64_t)g * 64 + lane];
            heads[u] = vis_head[g]; nb[u] = vis_nbase[g]; sp[u] = vis_sp[g];
            base[u] = gprefix[g]; want[u] = gprefix[g + 1] - base[u];
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
            // the decision: trio_visit_kernel's
            const uint32_t lo = min(w[u].x, w[u].z), hi = max(w[u].x, w[u].z);
            const unsigned long long vmask = __builtin_amdgcn_ballot_w64(valid[u]);
            const unsigned long long hd = heads[u] & vmask;
            const unsigned long long inb = vmask & ~hd;                      // lanes with a lane of their own stretch below them
            const uint32_t slo = wave_shr1z(lo), shi = wave_shr1z(hi);       // the pair of the lane below (DPP moves)
            const unsigned long long eq = __builtin_amdgcn_ballot_w64(slo == lo && shi == hi) & inb;
            const unsigned long long bad = __builtin_amdgcn_ballot_w64(slo > lo || (slo == lo && shi > hi)) & inb;
            const unsigned long long dup = eq | (eq >> 1);                   // both partners are not unique
            const unsigned long long uq = vmask & ~dup;
            const uint32_t n_g = (uint32_t)__popcll(uq);                     // wave-uniform
            if (g0 + (uint32_t)u < NG && (bad || n_g != want[u]) && lane == 0) atomicAdd(err, 1u);   // table out of order / offsets that are not this table's
            if (n_g == 0u) continue;
            // the queue holds consecutive rows of one species: file it first where this group does not fit behind them
            if (q_cnt && (q_cnt + n_g > 64u || sp[u] != q_sp || base[u] != q_row0 + q_cnt)) {
                trio_file_flush<KEYS>(qu, q_cnt, q_row0, q_sp, lane, node_rec, o, err);
                q_cnt = 0;
            }
            if (q_cnt == 0u) { q_row0 = base[u]; q_sp = sp[u]; }
            if ((uq >> lane) & 1ull) {
                const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(uq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)uq, 0u));   // unique visits in the lanes below
                qu.rec[q_cnt + rk] = make_uint4(q[u] - 1u, nb[u] + lo, nb[u] + hi, nb[u] + w[u].y);
            }
            q_cnt += n_g;
        }
    }
    if (q_cnt) trio_file_flush<KEYS>(qu, q_cnt, q_row0, q_sp, lane, node_rec, o, err);
}

// ---- the phases of trio_index_build ----
// the one-pass rebuild.  U groups in flight x `rounds` rounds per wave (tf_u / tf_rounds pick another shape, for measurements).  EIGHT groups per wave, all in
// flight at once, where the visit kernel of the first build takes 4 x 4: ms at 1e4 strains / at the fifty-strain share -- 8 x 1: 6.75 / 5.08, 4 x 2: 7.03 /
// 5.33, 2 x 4: 7.23, 2 x 3: 7.35, 4 x 4: 8.65 / 5.90, 4 x 3: 8.64, 4 x 1: 8.72 / 7.14, 2 x 1: 11.2 / 9.1 (a wave that is filing its queue has no
// loads in flight: short waves, many of them in turn -- but not so short that the queue is filed half empty)
template <int U, bool KEYS>
static void file_launch(Ctx *ctx, Db *db, const TrioGroupGrid &g, const RowOut &ro) {
    TrioScratch &ts = db->trio_scratch;
    hipLaunchKernelGGL((trio_file_kernel<U, KEYS>), dim3(g.grid), dim3(256), 0, ctx->stream, db->n_vgroups, g.rounds, db->d_vis_pos.p, db->d_vis_head.p, db->d_vis_nbase.p,
                       db->d_vis_sp.p, (const uint32_t *)ts.gprefix.p, db->d_path_nodes.p, db->d_node_rec.p, ro, ts.d_tot.p + 2, g.xcd_chunks);
}
int trio_file_launch(Ctx *ctx, Db *db, const TrioPlan &pl, const RowOut &ro) {
    TrioScratch &ts = db->trio_scratch;
    KTimer t(ctx, "trio_file_kernel");
    const TrioGroupGrid &g = pl.file;
    if (pl.with_keys) {
        if (g.u == 2) file_launch<2, true>(ctx, db, g, ro);
        else if (g.u == 4) file_launch<4, true>(ctx, db, g, ro);
        else if (g.u == 8) file_launch<8, true>(ctx, db, g, ro);
        else return fail(ctx, PANTAX_HIP_E_STATE, "trio_index: no trio_file_kernel of %u groups in flight", g.u);
    } else {
        if (g.u == 2) file_launch<2, false>(ctx, db, g, ro);
        else if (g.u == 4) file_launch<4, false>(ctx, db, g, ro);
        else if (g.u == 8) file_launch<8, false>(ctx, db, g, ro);
        else return fail(ctx, PANTAX_HIP_E_STATE, "trio_index: no trio_file_kernel of %u groups in flight", g.u);
    }
    // the rows of the fast route (the base of the path route's rows in a mixed db) = the closing entry of the offsets
    PTX_HIP(ctx, hipMemcpyAsync(ts.d_tot.p + 1, ts.gprefix.p + db->n_vgroups, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

// sizes of the fast route: the first row of every group; the total goes to d_tot[1]
int trio_group_prefix(Ctx *ctx, Db *db, const TrioPlan &pl) {
    TrioScratch &ts = db->trio_scratch;
    if (pl.prefix == TrioPrefix::chained)
        return exclusive_scan_fn(ctx, GroupCountLoad{reinterpret_cast<const unsigned long long *>(ts.vis_uq.p)}, PrefixStore{ts.gprefix.p},
                                 (uint64_t)db->n_vgroups + 1, ts.d_tot.p + 1, "scan_chained_kernel<GroupCount>");
    if (pl.prefix != TrioPrefix::tiles) return fail(ctx, PANTAX_HIP_E_STATE, "trio_index: no group prefix of this form");
    KTimer t(ctx, "group_tile_prefix_kernel");
    const uint64_t ng1 = (uint64_t)db->n_vgroups + 1;
    const uint32_t n_tiles = (uint32_t)((ng1 + FR_TILE - 1) / FR_TILE);
    PTX_HIP(ctx, ts.group_sums.alloc(n_tiles + 1));
    const unsigned long long *uq = reinterpret_cast<const unsigned long long *>(ts.vis_uq.p);
    hipLaunchKernelGGL(group_tile_sum_kernel, dim3(n_tiles), dim3(256), 0, ctx->stream, uq, ng1, ts.group_sums.p);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, ts.group_sums.p, n_tiles, ts.d_tot.p + 1);
    hipLaunchKernelGGL(group_tile_prefix_kernel, dim3(n_tiles), dim3(256), 0, ctx->stream, uq, ng1, (const uint32_t *)ts.group_sums.p, ts.gprefix.p);
    return 0;
}

// sizes of the path route: the first row of every node (and its lookup head); the total goes to d_tot[3]
int trio_head_scan(Ctx *ctx, Db *db, const TrioPlan &pl) {
    TrioScratch &ts = db->trio_scratch;
    const uint64_t V = db->V;
    if (pl.head_scan == TrioHeadScan::slow_first)   // the species of the node-block kernel: heads behind the visit table's rows
        return exclusive_scan_fn(ctx, SlowFirstLoad{ts.first_cnt.p, db->d_node_visited.p, db->d_trio_slow.p, db->d_emit_tile_sp.p, db->d_node_base.p, V},
                                 SlowFirstStore{db->d_trio_first.p, db->d_node_rec.p, V, ts.d_tot.p + 1, ts.d_tot.p + 2}, V, ts.d_tot.p + 3,
                                 "scan_chained_kernel<SlowFirst>");
    if (pl.head_scan != TrioHeadScan::trio_first) return fail(ctx, PANTAX_HIP_E_STATE, "trio_index: no head scan of this form");
    return exclusive_scan_fn(ctx, TrioFirstLoad{ts.first_cnt.p, pl.by_block ? db->d_node_visited.p : nullptr},
                             TrioFirstStore{db->d_trio_first.p, db->d_node_rec.p, V, ts.d_tot.p + 2}, V + 1, ts.d_tot.p + 3, "scan_chained_kernel<TrioFirst>");
}

// the rows of the fast route.  A wave takes rows_u = 1, 2 or 4 batches of eight groups at once.  Two halve what the kernel waits for memory -- and the
// step got SLOWER in round 4 (the current step's local sorts, which run beside it on the main stream, stretched from 1.1 to 3.8 ms).  Hence one.
template <bool KEYS, bool FIRST, int U>
static void rows_launch(Ctx *ctx, Db *db, const TrioRowsGrid &g, const RowOut &ro) {
    TrioScratch &ts = db->trio_scratch;
    hipLaunchKernelGGL((trio_rows_kernel<KEYS, FIRST, U>), dim3(g.grid), dim3(256), 0, ctx->stream, db->n_vgroups, reinterpret_cast<const unsigned long long *>(ts.vis_uq.p),
                       ts.gprefix.p, ts.vis_rec.p, db->d_vis_nbase.p, db->d_vis_sp.p, db->d_vis_pos.p, db->d_path_nodes.p, db->d_node_rec.p, ro, ts.d_tot.p + 2, g.xcd_chunks,
                       g.iters);
}
template <bool KEYS, bool FIRST>
static int rows_pick(Ctx *ctx, Db *db, const TrioRowsGrid &g, const RowOut &ro) {
    if (g.u == 1) rows_launch<KEYS, FIRST, 1>(ctx, db, g, ro);
    else if (g.u == 2) rows_launch<KEYS, FIRST, 2>(ctx, db, g, ro);
    else if (g.u == 4) rows_launch<KEYS, FIRST, 4>(ctx, db, g, ro);
    else return fail(ctx, PANTAX_HIP_E_STATE, "trio_index: no trio_rows_kernel of %u batches in flight", g.u);
    return 0;
}
int trio_rows_launch(Ctx *ctx, Db *db, const TrioPlan &pl, const RowOut &ro) {
    db->trio_scratch.gprefix_for = db->n_vgroups;       // the offsets this launch files by stay with the table: later builds file in one pass (trio_file_kernel)
    KTimer t(ctx, "trio_rows_kernel");
    if (pl.with_keys) return pl.first_build ? rows_pick<true, true>(ctx, db, pl.rows, ro) : rows_pick<true, false>(ctx, db, pl.rows, ro);
    return pl.first_build ? rows_pick<false, true>(ctx, db, pl.rows, ro) : rows_pick<false, false>(ctx, db, pl.rows, ro);
}

// the rows of the path route: every unique window dropped into its node's block, the blocks then put into the canonical order and filed
template <bool KEYS, bool FIRST>
static void canon_launch(Ctx *ctx, Db *db, const TrioPlan &pl, const RowOut &ro) {
    hipLaunchKernelGGL((trio_canon_kernel<KEYS, FIRST>), dim3((uint32_t)((db->V + 255) / 256)), dim3(256), 0, ctx->stream, db->V, db->S, (const uint32_t *)db->d_node_base.p,
                       (const uint4 *)db->d_node_rec.p, (const uint32_t *)db->d_trio_first.p, pl.by_block ? (const uint32_t *)db->d_node_visited.p : (const uint32_t *)nullptr,
                       pl.mixed ? (const uint32_t *)db->d_trio_slow.p : (const uint32_t *)nullptr, db->trio_scratch.row_q.p, ro);
}
int trio_path_rows_launch(Ctx *ctx, Db *db, const TrioPlan &pl, const RowOut &ro) {
    TrioScratch &ts = db->trio_scratch;
    {
        KTimer t(ctx, "trio_lookup_kernel");
        hipLaunchKernelGGL(trio_lookup_kernel, dim3((uint32_t)db->n_tiles), dim3(256), 0, ctx->stream, TRIO_GRAPH(db), (const uint32_t *)ts.uniq_q.p,
                           (const uint32_t *)db->d_trio_first.p, ts.first_cnt.p, db->d_trio_ent.p, ts.row_q.p,
                           pl.mixed ? (const uint32_t *)db->d_trio_slow.p : (const uint32_t *)nullptr);
    }
    KTimer t(ctx, "trio_canon_kernel");
    if (pl.with_keys) { if (pl.first_build) canon_launch<true, true>(ctx, db, pl, ro); else canon_launch<true, false>(ctx, db, pl, ro); }
    else { if (pl.first_build) canon_launch<false, true>(ctx, db, pl, ro); else canon_launch<false, false>(ctx, db, pl, ro); }
    return 0;
}

}  // namespace ptx
