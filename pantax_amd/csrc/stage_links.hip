// stage_links.hip -- link support (pantax_hip_strain_links, the --strain-links report): which adjacencies of a selected strain the reads cross.  Not a
// stage of the reference.
//
// Contract: include/pantax_hip.h, DESIGN.md "Link support".  Integers only: no result depends on any order.
//
// Link table.  links_key_kernel walks the tiles of the selected walks (cov_track_tile.hpp) and emits one 64-bit key per link position,
// (global smaller node) << 32 | global larger node, with the payload species << 6 | list position.  radix_sort orders the keys (two runs of
// bits_for(V - 1) bits).  ONE chained scan (links_table_kernel: scan_chained.hpp with a load and a store functor) finds the run heads, numbers the
// distinct links, files {larger node, smaller node, species} of a link at its head and ORs every key's payload bit into L[link].  links_off_kernel
// files the links at their smaller node: link_off[u] = the first link whose smaller node is >= u, a binary search per node over the distinct smaller
// nodes, so that a lookup is one offset pair and a scan over the node's few larger neighbours.
// Read pass.  links_read_kernel walks the locus-grouped step stream (read_pass_device.hpp: a wave per 64-step group, a lane per step).  A step's
// successor in its walk is the next lane; lane 63 reads the first node of the next group, which is the walk's next step also for walks of more than 64
// steps.  A crossing that is a link adds one to support[link]; any other crossing takes the membership words of its two nodes (either route of
// member_plan.hpp) and adds to its class per lane -- these are rare.  counted_reads, crossings and known are reduced per species of the wave: three
// ballots and at most three 64-bit atomics from lane 0.
// Walk pass.  links_walk_kernel<false> (count) and <true> (emit) run a wave per tile, 16 positions per lane: the successor of a lane's last position is
// the next lane's first, that of the tile's last position the first of the next tile, read directly.  The count pass writes one LkTileSum per tile
// (summed node length, the seven position counters packed in 16-bit fields, the summed support); the host sums them per entry, scans the broken
// counts into brk_off and gives every tile its first slot and its path offset; the emit pass writes every break record from the one lane that owns
// it: count, wave prefix, emit -- no atomics.  links_count_kernel sums the four link counters per species over the distinct links.
//
// Algorithmic bytes (P_sel selected path positions, D distinct links, T' padded steps, R' slots): keys 12 P_sel out, the sort 24 P_sel per pass in and
// out, the table 12 P_sel in + 16 D out; the read pass 4 T' + 1 T' + 16 R' + 8 R' in plus 8 bytes of offsets and 4 per scanned neighbour per crossing
// and one 8-byte atomic; the walk pass (4 + 4) P_sel + per link position the lookup, 8 (support) + 8 (L) + 16 (bases of both ends), twice when any
// position is broken; 40 bytes per break record out.
#include <algorithm>
#include "common.hpp"
#include "cov_track_tile.hpp"
#include "links_plan.hpp"
#include "read_pass_device.hpp"
#include "scan_chained.hpp"

namespace ptx {

namespace {

struct LkSpecies {
    unsigned long long all;   // the K_s low bits: L of a core link
    uint32_t open;            // 1: K_s <= 64
    uint32_t pad;
};
// what a tile of a selected walk carries besides its CtTile
struct LkTile {
    uint64_t end;      // global path position behind the walk's last step
    uint64_t key0;     // first key of the tile (one key per position but the walk's last)
    uint32_t payload;  // species << 6 | list position
    uint32_t pad;
};
struct LkTileSum { unsigned long long sum_len, c0, c1, support; };   // c0 = links | crossed << 16 | open << 32 | broken << 48; c1 = private | private_crossed << 16 | private_broken << 32
struct LkPlace { uint64_t base, out0, step0; };                       // path offset of the tile's first step, its first record slot, the walk-local step of its first position
struct LkTable {
    const uint32_t *off;                 // [V + 1] the links of global node u as the smaller end: [off[u], off[u + 1])
    const uint32_t *hi;                  // [D] the larger end, ascending within a node
    const unsigned long long *L;         // [D]
    unsigned long long *support;         // [D]
};
struct LkOut { unsigned long long *step, *start, *flank, *mask; uint32_t *node_a, *node_b; uint64_t n; };

__device__ __forceinline__ uint32_t lk_find(const LkTable &tb, uint32_t u, uint32_t v) {
    const uint32_t a = min(u, v), b = max(u, v);
    const uint32_t d1 = tb.off[a + 1];
    for (uint32_t d = tb.off[a]; d < d1; ++d)
        if (tb.hi[d] == b) return d;
    return MEMBER_NO_ENTRY;
}

// ---- the link table ----
__global__ void __launch_bounds__(256) links_key_kernel(uint32_t n_tiles, const CtTile *__restrict__ tiles, const LkTile *__restrict__ xt,
                                                        const uint32_t *__restrict__ path_nodes, uint64_t n_keys, unsigned long long *__restrict__ key,
                                                        uint32_t *__restrict__ val) {
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * 4) {
        const CtTile tl = tiles[t];
        const LkTile x = xt[t];
        for (uint32_t j = (uint32_t)lane; j < tl.n; j += 64u) {
            const uint64_t q = tl.p0 + j, k = x.key0 + j;
            if (q + 1 >= x.end || k >= n_keys) continue;   // the walk's last step carries no link
            const uint32_t u = path_nodes[q] + tl.node_base, v = path_nodes[q + 1] + tl.node_base;
            key[k] = ((unsigned long long)min(u, v) << 32) | (unsigned long long)max(u, v);
            val[k] = x.payload;
        }
    }
}
// the chained scan over the sorted keys: load = "this key opens a run", store files the key under the number of its run
struct LkHeadLoad {
    const unsigned long long *key;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return (i == 0 || key[i] != key[i - 1]) ? 1u : 0u; }
};
struct LkFileStore {
    const unsigned long long *key;
    const uint32_t *val;
    uint32_t *hi, *lo, *sp;
    unsigned long long *L;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t excl, uint32_t head) const {
        const uint32_t d = excl + head - 1u;   // (item 0 is a head: never below zero)
        const uint32_t pv = val[i];
        atomicOr(&L[d], 1ull << (pv & 63u));
        if (head) {
            const unsigned long long k = key[i];
            hi[d] = (uint32_t)k; lo[d] = (uint32_t)(k >> 32); sp[d] = pv >> 6;
        }
    }
};
__global__ void __launch_bounds__(256) links_off_kernel(uint64_t V, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ d_D, uint32_t *__restrict__ off) {
    const uint32_t D = *d_D;
    for (uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x; u <= V; u += (uint64_t)gridDim.x * 256u) {
        uint32_t a = 0u, b = D;                // the first link whose smaller node is >= u
        while (a < b) {
            const uint32_t m = a + ((b - a) >> 1);
            if ((uint64_t)lo[m] < u) a = m + 1u; else b = m;
        }
        off[u] = a;
    }
}
__global__ void __launch_bounds__(256) links_count_kernel(uint64_t n_bound, const uint32_t *__restrict__ d_D, const uint32_t *__restrict__ sp,
                                                          const unsigned long long *__restrict__ L, const unsigned long long *__restrict__ support,
                                                          const LkSpecies *__restrict__ lks, unsigned long long *__restrict__ link_out) {
    const int lane = threadIdx.x & 63;
    const uint64_t D = min((uint64_t)*d_D, n_bound);
    for (uint64_t base = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64u; base < D; base += (uint64_t)gridDim.x * 256u) {   // (wave-uniform)
        const uint64_t d = base + (uint64_t)lane;
        const bool in = d < D;
        uint32_t s = 0u;
        bool crossed = false, core = false;
        if (in) { s = sp[d]; crossed = support[d] != 0ull; core = L[d] == lks[s].all; }
        rs_species_rounds(in, s, [&](uint32_t s0, bool mine, unsigned long long mb) {
            const unsigned long long xb = __builtin_amdgcn_ballot_w64(mine && crossed);
            const unsigned long long cb = __builtin_amdgcn_ballot_w64(mine && core), cxb = __builtin_amdgcn_ballot_w64(mine && core && crossed);
            if (lane == 0) {
                unsigned long long *const o = link_out + (uint64_t)s0 * LNK_N_TABLE;
                atomicAdd(o + LNK_DISTINCT, (unsigned long long)__popcll(mb));
                if (xb) atomicAdd(o + LNK_DISTINCT_CROSSED, (unsigned long long)__popcll(xb));
                if (cb) atomicAdd(o + LNK_CORE, (unsigned long long)__popcll(cb));
                if (cxb) atomicAdd(o + LNK_CORE_CROSSED, (unsigned long long)__popcll(cxb));
            }
        });
    }
}

// ---- the read pass ----
__global__ void __launch_bounds__(256) links_read_kernel(uint32_t n_groups, uint32_t n_slots, const uint32_t *__restrict__ group_slot,
                                                         const uint8_t *__restrict__ step_code, const uint32_t *__restrict__ g_node_id,
                                                         const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec, uint64_t T_pad,
                                                         const RsSpecies *__restrict__ tab, const LkSpecies *__restrict__ lks,
                                                         const unsigned long long *__restrict__ node_haps, const unsigned long long *__restrict__ mask, LkTable tb,
                                                         unsigned long long *__restrict__ sp_out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * 4) {
        const uint32_t gs = group_slot[g];                                   // (wave-uniform) NO_SLOT: a group of pads only
        if (gs == RS_NO_SLOT) continue;
        const RsLane L = rs_lane(g, gs, lane, n_slots, step_code, g_node_id, read_rec, slot_rec, tab);
        const uint64_t t = (uint64_t)g * 64u + (uint64_t)lane;
        const bool cross = L.counted && !L.last && t + 1 < T_pad;            // the crossing {my step, the next step of my walk}
        uint32_t nxt = wave_shl1(L.v);
        if (lane == 63 && cross) nxt = g_node_id[t + 1] + L.sr.y;            // the walk goes on in the next group
        LkSpecies ls{0ull, 0u, 0u};
        if (cross) ls = lks[L.sr.x];
        const bool open = cross && ls.open != 0u;
        uint32_t d = MEMBER_NO_ENTRY;
        if (open) d = lk_find(tb, L.v, nxt);
        const bool known = open && d != MEMBER_NO_ENTRY;
        if (known) atomicAdd(&tb.support[d], 1ull);
        if (open && !known) {                                                // rare: per lane
            const int cls = link_unknown_class(rs_word1(L.st, L.v, node_haps, mask), rs_word1(L.st, nxt, node_haps, mask));
            atomicAdd(sp_out + (uint64_t)L.sr.x * LNK_N_SPECIES + (uint32_t)cls, 1ull);
        }
        // counted_reads, crossings and known take nearly every step: per species of the wave
        rs_species_rounds(L.counted, L.sr.x, [&](uint32_t s0, bool mine, unsigned long long) {
            const unsigned long long rb = __builtin_amdgcn_ballot_w64(mine && L.last);
            const unsigned long long xb = __builtin_amdgcn_ballot_w64(mine && cross), kb = __builtin_amdgcn_ballot_w64(mine && known);
            if (lane == 0) {
                unsigned long long *const o = sp_out + (uint64_t)s0 * LNK_N_SPECIES;
                if (rb) atomicAdd(o + LNK_COUNTED, (unsigned long long)__popcll(rb));
                if (xb) atomicAdd(o + LNK_CROSSINGS, (unsigned long long)__popcll(xb));
                if (kb) atomicAdd(o + LNK_KNOWN, (unsigned long long)__popcll(kb));
            }
        });
    }
}

// ---- the walk pass ----
template <bool EMIT>
__global__ void __launch_bounds__(256) links_walk_kernel(uint32_t n_tiles, const CtTile *__restrict__ tiles, const LkTile *__restrict__ xt,
                                                         const LkPlace *__restrict__ place, const uint32_t *__restrict__ path_nodes,
                                                         const uint32_t *__restrict__ node_len, const unsigned long long *__restrict__ bases, LkTable tb,
                                                         LkTileSum *__restrict__ sums, LkOut out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * 4) {
        const CtTile tl = tiles[t];
        const LkTile x = xt[t];
        const uint64_t blk = tl.p0 & ~(CT_TILE - 1), q0 = blk + 16u * (uint32_t)lane;
        uint32_t v[16];
        const uint32_t live = ct_load_ids(path_nodes, q0, tl.p0, tl.p0 + tl.n, tl.node_base, v);
        // the successor of my last position: the next lane's first, or the first position of the next tile
        uint32_t after = wave_shl1(v[0]);
        if (lane == 63 && blk + CT_TILE < x.end) after = path_nodes[blk + CT_TILE] + tl.node_base;
        const unsigned long long me = 1ull << (x.payload & 63u);
        uint32_t len[16];
        unsigned long long lane_sum = 0ull, c0 = 0ull, c1 = 0ull, sup_sum = 0ull;
        uint32_t brk = 0u;   // bit j: position j is broken
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool on = (live >> j) & 1u;
            len[j] = on ? node_len[v[j]] : 0u;
            lane_sum += len[j];
            if (!on || q0 + (uint32_t)j + 1 >= x.end) continue;   // outside the walk, or its last step
            const uint32_t w = j < 15 ? v[j < 15 ? j + 1 : 15] : after;
            const uint32_t d = lk_find(tb, v[j], w);
            unsigned long long sup = 0ull, lm = 0ull;
            if (d != MEMBER_NO_ENTRY) { sup = tb.support[d]; lm = tb.L[d]; }   // (always: the table was built from these positions)
            const bool crossed = sup != 0ull;
            const bool broken = !crossed && bases[v[j]] != 0ull && bases[w] != 0ull;
            const bool priv = lm == me;
            brk |= (broken ? 1u : 0u) << j;
            sup_sum += sup;
            c0 += 1ull + (crossed ? 1ull << 16 : 0ull) + ((!crossed && !broken) ? 1ull << 32 : 0ull) + (broken ? 1ull << 48 : 0ull);
            c1 += (priv ? 1ull : 0ull) + ((priv && crossed) ? 1ull << 16 : 0ull) + ((priv && broken) ? 1ull << 32 : 0ull);
        }
        if constexpr (!EMIT) {
            const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
            lane_sum = wave_reduce(lane_sum, add); c0 = wave_reduce(c0, add); c1 = wave_reduce(c1, add); sup_sum = wave_reduce(sup_sum, add);
            if (lane == 0) sums[t] = LkTileSum{lane_sum, c0, c1, sup_sum};
        } else {
            const LkPlace pl = place[t];
            const uint32_t mine = (uint32_t)__popc(brk);
            if (__builtin_amdgcn_ballot_w64(mine != 0u) == 0ull) continue;   // (wave-uniform) no break in this tile
            uint64_t slot = pl.out0 + (wave_incl_scan_dpp(mine) - mine);
            unsigned long long o = ct_incl_scan64(lane_sum) - lane_sum;       // summed length of the tile's positions before the lane
            const uint32_t first_pos = (uint32_t)(tl.p0 & (CT_TILE - 1));
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                o += len[j];                                                  // ... up to and including position j: o_{i+1}
                if (!((brk >> j) & 1u)) continue;
                const uint32_t w = j < 15 ? v[j < 15 ? j + 1 : 15] : after;
                const uint32_t d = lk_find(tb, v[j], w);
                if (slot < out.n) {   // (always: the plan counted the same positions)
                    const uint32_t la = len[j], lb = node_len[w];
                    const unsigned long long fa = la ? bases[v[j]] / la : 0ull, fb = lb ? bases[w] / lb : 0ull;
                    out.step[slot] = pl.step0 + (16u * (uint32_t)lane + (uint32_t)j - first_pos);
                    out.start[slot] = pl.base + o;
                    out.node_a[slot] = v[j] - tl.node_base;
                    out.node_b[slot] = w - tl.node_base;
                    out.flank[slot] = fa < fb ? fa : fb;
                    out.mask[slot] = d != MEMBER_NO_ENTRY ? tb.L[d] : 0ull;
                }
                ++slot;
            }
        }
    }
}

}  // namespace

// The selection validated by the caller, in the caller's order.  brk_off_out [C+1], species_out [S][6], link_out [S][4] and hap_out [C][8] are written
// on success and on the PANTAX_HIP_E_LIMIT of the record cap; the six record arrays only when the cap holds the records.
int links_launch(Ctx *ctx, Db *db, Reads *rd, const uint64_t *sel_off, const uint32_t *sel_hap, uint64_t *species_out, uint64_t *link_out, uint64_t *hap_out,
                 uint64_t *brk_off_out, uint64_t cap, uint64_t *brk_step_out, uint64_t *brk_start_out, uint32_t *brk_node_a_out, uint32_t *brk_node_b_out,
                 uint64_t *brk_flank_out, uint64_t *brk_mask_out) {
    const uint32_t S = db->S;
    const uint64_t C = sel_off[S], V = db->V;
    if (S >= (1u << 26)) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_links: %u species (a key's payload holds 26 bits of species)", S);
    if (V >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_links: %llu nodes exceed 32-bit positions", (unsigned long long)V);
    // the membership list of every open species; a skipped species gets an empty one: no masks are built for it
    std::vector<uint64_t> list_off(S + 1, 0);
    std::vector<uint32_t> list;
    std::vector<LkSpecies> lks(S ? S : 1, LkSpecies{0ull, 0u, 0u});
    std::vector<CtTile> tiles;
    std::vector<LkTile> xt;
    std::vector<uint64_t> tile_first(C + 1, 0), walk_p0(C ? C : 1, 0);
    uint64_t n_keys = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = sel_off[s + 1] - sel_off[s];
        if (K <= LINKS_MAX_LIST) {
            lks[s].open = 1u;
            lks[s].all = K == 64 ? ~0ull : (1ull << K) - 1ull;
            list.insert(list.end(), sel_hap + sel_off[s], sel_hap + sel_off[s + 1]);
        }
        list_off[s + 1] = list.size();
        for (uint64_t c = sel_off[s]; c < sel_off[s + 1]; ++c) {
            if (lks[s].open) {
                const uint64_t h = db->h_hap_off[s] + sel_hap[c], p1 = db->h_path_off[h + 1];
                walk_p0[c] = db->h_path_off[h];
                for (uint64_t p = db->h_path_off[h]; p < p1;) {
                    const uint64_t e = std::min(p1, (p & ~(CT_TILE - 1)) + CT_TILE);
                    tiles.push_back(CtTile{p, (uint32_t)(e - p), (uint32_t)db->h_node_off[s]});
                    xt.push_back(LkTile{p1, n_keys, (s << 6) | (uint32_t)(c - sel_off[s]), 0u});
                    n_keys += (e - p) - (e == p1 ? 1 : 0);
                    p = e;
                }
            }
            tile_first[c + 1] = tiles.size();
        }
    }
    if (tiles.size() >= 0xFFFFFFFFull || n_keys >= 0xFFFFFFFFull)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_links: %llu positions of selected walks exceed 32-bit positions", (unsigned long long)n_keys);
    const uint32_t n_tiles = (uint32_t)tiles.size();
    if (list.empty()) list.push_back(0u);   // (a pointer to hand on)
    RsTable rt;
    rs_table_build(ctx, db, list_off.data(), list.data(), rt, [](uint64_t, uint64_t) {});
    DevBuf<RsSpecies> d_tab;
    DevBuf<LkSpecies> d_lks;
    DevBuf<CtTile> d_tiles;
    DevBuf<LkTile> d_xt;
    DevBuf<unsigned long long> d_ka, d_kb, d_L, d_cnt;   // d_L: [L n_keys][support n_keys]; d_cnt: [species S x 6][link S x 4]
    DevBuf<uint32_t> d_va, d_vb, d_meta, d_off, d_sort_table, d_scan_tmp, d_D;   // d_meta: [hi n_keys][lo n_keys][sp n_keys]
    const size_t nk = n_keys ? (size_t)n_keys : 1, n_cnt = (size_t)S * (LNK_N_SPECIES + LNK_N_TABLE);
    PTX_TRY(upload(ctx, d_tab, rt.tab.data(), rt.tab.size()));
    PTX_TRY(upload(ctx, d_lks, lks.data(), lks.size()));
    PTX_TRY(rt.wm.build(ctx, db));
    PTX_HIP(ctx, d_L.alloc(2 * nk));
    PTX_HIP(ctx, d_meta.alloc(3 * nk));
    PTX_HIP(ctx, d_off.alloc((size_t)V + 1));
    PTX_HIP(ctx, d_D.alloc(1));
    PTX_HIP(ctx, d_cnt.alloc(n_cnt ? n_cnt : 1));
    PTX_TRY(zero_fill(ctx, d_L.p, 2 * nk * sizeof(unsigned long long)));
    PTX_TRY(zero_fill(ctx, d_off.p, ((size_t)V + 1) * sizeof(uint32_t)));
    PTX_HIP(ctx, hipMemsetAsync(d_D.p, 0, sizeof(uint32_t), ctx->stream));
    PTX_HIP(ctx, hipMemsetAsync(d_cnt.p, 0, (n_cnt ? n_cnt : 1) * sizeof(unsigned long long), ctx->stream));
    uint32_t *const d_hi = d_meta.p, *const d_lo = d_meta.p + nk, *const d_sp = d_meta.p + 2 * nk;
    unsigned long long *const d_sp_out = d_cnt.p, *const d_link_out = d_cnt.p + (size_t)S * LNK_N_SPECIES;
    const LkTable tb{d_off.p, d_hi, d_L.p, d_L.p + nk};
    if (n_tiles) {
        PTX_TRY(upload(ctx, d_tiles, tiles.data(), tiles.size()));
        PTX_TRY(upload(ctx, d_xt, xt.data(), xt.size()));
    }
    if (n_keys) {
        PTX_HIP(ctx, d_ka.alloc(nk)); PTX_HIP(ctx, d_kb.alloc(nk)); PTX_HIP(ctx, d_va.alloc(nk)); PTX_HIP(ctx, d_vb.alloc(nk));
        PTX_HIP(ctx, d_sort_table.alloc(sort_table_elems(n_keys))); PTX_HIP(ctx, d_scan_tmp.alloc(scan_tmp_elems(n_keys)));
        {
            KTimer tm(ctx, "links_key_kernel");
            hipLaunchKernelGGL(links_key_kernel, dim3(grid_for(n_tiles, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_tiles, d_tiles.p, d_xt.p,
                               db->d_path_nodes.p, n_keys, d_ka.p, d_va.p);
        }
        SortBufs A, B;
        A.nw = B.nw = 1; A.k[0] = reinterpret_cast<uint64_t *>(d_ka.p); B.k[0] = reinterpret_cast<uint64_t *>(d_kb.p); A.v = d_va.p; B.v = d_vb.p;
        std::vector<SortPass> passes;
        const int nb = bits_for(V ? V - 1 : 0);
        add_passes(passes, 0, 0, nb);
        add_passes(passes, 0, 32, 32 + nb);
        bool in_b = false;
        PTX_TRY(radix_sort(ctx, A, B, n_keys, passes.data(), (int)passes.size(), d_sort_table.p, d_scan_tmp.p, &in_b));
        const unsigned long long *const key = in_b ? d_kb.p : d_ka.p;
        const uint32_t *const val = in_b ? d_vb.p : d_va.p;
        PTX_TRY(exclusive_scan_fn(ctx, LkHeadLoad{key}, LkFileStore{key, val, d_hi, d_lo, d_sp, d_L.p}, n_keys, d_D.p, "links_table_kernel"));
        {
            KTimer tm(ctx, "links_off_kernel");
            hipLaunchKernelGGL(links_off_kernel, dim3(grid_for(V + 1, 256, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, V, d_lo, d_D.p, d_off.p);
        }
    }
    rs_launch_groups(ctx, rd, "links_read_kernel", links_read_kernel, rd->T_pad, d_tab.p, d_lks.p, rs_node_haps(rt, db), rt.wm.d_mask.p, tb, d_sp_out);
    DevBuf<LkTileSum> d_sums;
    std::vector<LkTileSum> sums(n_tiles);
    if (n_keys) {
        KTimer tm(ctx, "links_count_kernel");
        hipLaunchKernelGGL(links_count_kernel, dim3(grid_for((n_keys + 63) / 64, 4, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, n_keys, d_D.p, d_sp, tb.L,
                           tb.support, d_lks.p, d_link_out);
    }
    if (n_tiles) {
        PTX_HIP(ctx, d_sums.alloc(n_tiles));
        KTimer tm(ctx, "links_walk_kernel");
        hipLaunchKernelGGL(links_walk_kernel<false>, dim3(grid_for(n_tiles, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_tiles, d_tiles.p, d_xt.p,
                           (const LkPlace *)nullptr, db->d_path_nodes.p, db->d_node_len.p, db->d_bases.p, tb, d_sums.p, LkOut{});
    }
    PTX_HIP(ctx, hipGetLastError());
    std::vector<uint64_t> h_cnt(n_cnt ? n_cnt : 1, 0), h_hap(C ? C * LNK_N_HAP : 1, 0), h_off(C + 1, 0);
    if (n_cnt) PTX_TRY(download(ctx, (unsigned long long *)h_cnt.data(), d_cnt.p, n_cnt));
    if (n_tiles) PTX_TRY(download(ctx, sums.data(), d_sums.p, n_tiles));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // per entry the sums of its tiles; per tile its path offset, its walk-local first step and its first record slot
    std::vector<LkPlace> place(n_tiles);
    uint64_t N = 0;
    for (uint64_t c = 0; c < C; ++c) {
        uint64_t *o = h_hap.data() + c * LNK_N_HAP, base = 0;
        for (uint64_t t = tile_first[c]; t < tile_first[c + 1]; ++t) {
            const LkTileSum &ts = sums[t];
            const uint64_t broken = (ts.c0 >> 48) & 0xFFFFu;
            place[t] = LkPlace{base, N, tiles[t].p0 - walk_p0[c]};
            base += ts.sum_len;
            N += broken;
            o[LNK_LINKS] += ts.c0 & 0xFFFFu; o[LNK_CROSSED] += (ts.c0 >> 16) & 0xFFFFu; o[LNK_OPEN] += (ts.c0 >> 32) & 0xFFFFu; o[LNK_BROKEN] += broken;
            o[LNK_PRIVATE] += ts.c1 & 0xFFFFu; o[LNK_PRIVATE_CROSSED] += (ts.c1 >> 16) & 0xFFFFu; o[LNK_PRIVATE_BROKEN] += (ts.c1 >> 32) & 0xFFFFu;
            o[LNK_SUPPORT] += ts.support;
        }
        h_off[c + 1] = N;
    }
    const auto summaries = [&]() {
        std::copy(h_off.begin(), h_off.end(), brk_off_out);
        if (S) std::copy(h_cnt.begin(), h_cnt.begin() + (size_t)S * LNK_N_SPECIES, species_out);
        if (S) std::copy(h_cnt.begin() + (size_t)S * LNK_N_SPECIES, h_cnt.begin() + n_cnt, link_out);
        if (C) std::copy(h_hap.begin(), h_hap.begin() + C * LNK_N_HAP, hap_out);
    };
    if (N > cap) {
        summaries();
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_links: the selection has %llu break records, the output arrays hold %llu (brk_off_out is filled: size the arrays by it)",
                    (unsigned long long)N, (unsigned long long)cap);
    }
    if (N == 0) { summaries(); return 0; }
    if (!brk_step_out || !brk_start_out || !brk_node_a_out || !brk_node_b_out || !brk_flank_out || !brk_mask_out)
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_links: null output array");
    if (N > (~(size_t)0) / 64) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_links: %llu break records", (unsigned long long)N);
    // one device block: [step N u64][start N u64][flank N u64][mask N u64][node_a N u32][node_b N u32]
    DevBuf<unsigned long long> d_out;
    DevBuf<LkPlace> d_place;
    PTX_HIP(ctx, d_out.alloc((size_t)N * 5));
    PTX_TRY(upload(ctx, d_place, place.data(), place.size()));
    unsigned long long *const o64 = d_out.p;
    uint32_t *const o32 = reinterpret_cast<uint32_t *>(o64 + 4 * N);
    const LkOut out{o64, o64 + N, o64 + 2 * N, o64 + 3 * N, o32, o32 + N, N};
    {
        KTimer tm(ctx, "links_emit_kernel");
        hipLaunchKernelGGL(links_walk_kernel<true>, dim3(grid_for(n_tiles, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_tiles, d_tiles.p, d_xt.p, d_place.p,
                           db->d_path_nodes.p, db->d_node_len.p, db->d_bases.p, tb, (LkTileSum *)nullptr, out);
    }
    PTX_HIP(ctx, hipGetLastError());
    std::vector<uint64_t> h64((size_t)N * 4);
    std::vector<uint32_t> h32((size_t)N * 2);
    PTX_TRY(download(ctx, (unsigned long long *)h64.data(), o64, (size_t)N * 4));
    PTX_TRY(download(ctx, h32.data(), o32, (size_t)N * 2));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    summaries();
    std::copy(h64.begin(), h64.begin() + N, brk_step_out);
    std::copy(h64.begin() + N, h64.begin() + 2 * N, brk_start_out);
    std::copy(h64.begin() + 2 * N, h64.begin() + 3 * N, brk_flank_out);
    std::copy(h64.begin() + 3 * N, h64.end(), brk_mask_out);
    std::copy(h32.begin(), h32.begin() + N, brk_node_a_out);
    std::copy(h32.begin() + N, h32.end(), brk_node_b_out);
    return 0;
}

}  // namespace ptx
