// stage_depth.hip -- per-strain depth distribution (pantax_hip_strain_depth, the --strain-depth report): the histogram of node depth over the nodes a
// reported strain walks, over the nodes only it walks among the reported strains of its species, over every node of the species and over the nodes no
// reported strain walks.  What the means of the node evidence report cannot tell: a mobile element at 400x beside private nodes at 3x, a private genome
// that is mostly empty under a healthy mean.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Per-strain depth distribution"): selection, M(v) and m(v) of pantax_hip_strain_evidence; the depth of a node
// d(v) = bases_per_node[v] / node_len[v] in u64 integer division (0 for node_len 0), its bin depth_bin(d) of DEPTH_BINS = 96 (depth_device.hpp, shared
// with the host helpers).  Every output is, per bin, the sum of (1, node_len[v]) over a class of nodes: per selection entry `all` (h in M(v)) and `private`
// (M(v) = {h}), per species `total` (every node) and `orphan` (m(v) = 0).  Integers only: no order matters, no floating point on the device.
//
// Membership: the two routes of member_plan.hpp over the selected haplotypes (option depth_route), nw = ceil(K_s / 64) words per node on route 2.
// depth_hist_kernel: a histogram scatters over bins, so the node evidence kernel's reduction of K_s sums across the wave does not carry over: the
// counters live in LDS and take 64-bit LDS atomics.  One selected haplotype costs 2 classes x 96 bins x {n_nodes, len} x 8 B = 3 KB, so 64 of them do not fit
// beside a useful occupancy: the selected haplotypes of a species are taken in TILES of DP_HAPS = 8 (8 divides 64: a tile lies in one mask word), and the
// two species rows (total, orphan) ride along with tile 0 as two more counter rows.  The host cuts every species' nodes into CHUNKS of DP_CHUNK = 2048
// nodes and lists one item per (species, tile, chunk), tile-major, so the items of one (species, tile) are neighbours; a species of K_s selected haplotypes
// is read ceil(K_s / 8) times (once at K_s <= 8: 1.6 reported strains a species at cfg4).  A workgroup of 256 threads takes a CONTIGUOUS run of items and
// keeps its counters while (species, tile) stays the same: it flushes -- one pass over the 18 x 192 counters, one 64-bit global atomicAdd per NON-ZERO counter,
// the counter zeroed in the same pass -- only where the key changes and at the end of its run.  With runs of n_items / grid items the flushes number about
// grid + (species x tiles), not one per chunk: the zero-scan (3456 LDS words, 13.5 per thread) stands against at least one chunk of 2048 nodes read from
// HBM and against about 120 chunks at cfg4.  A chunk is taken in slabs of 1024 nodes, thread t the nodes t, t + 256, t + 512, t + 768 of the slab: every load
// instruction of a wave is one contiguous stretch, and four nodes' loads are in flight per thread before the first atomic.
//
// LDS per workgroup: 18 rows x 96 bins x 2 x 8 B = 27648 B (static).  Occupancy that leaves: 5 workgroups = 20 waves a CU of the 160 KB (LDS-bound; the
// kernel needs few registers), which is also the grid: 5 x CUs workgroups, every one resident (the test option depth_grid caps it lower).
// Algorithmic bytes (V nodes, C selection entries, S species), route 1 with K_s <= 8:  (4 + 8 + 8) V in (node_len, bases_per_node, membership word;
// node_base_cov is not read), 16 B per item, at most 3072 C + 3072 S out per flush.  In general a species of V_s nodes and T_s = max(1, ceil(K_s / 8)) tiles:
// route 1 20 T_s V_s, route 2 (12 + 8 nw) T_s V_s with nw = ceil(K_s / 64), behind the mask pass of WalkMasks.
// LDS atomics: per node 2 (total) + 2 per selected haplotype of the tile that walks it (+ 2 where it is private, + 2 where it is an orphan); nodes of one
// depth queue on one counter pair, which is what bounds the pass on a sample of even depth (DESIGN gives the measured figure).
#include <algorithm>
#include "common.hpp"
#include "depth_device.hpp"
#include "member_device.hpp"
#include "primitives.hpp"

namespace ptx {

namespace {

constexpr uint32_t DP_CHUNK = 2048;                      // nodes per item
constexpr uint32_t DP_SLAB = 1024;                       // nodes a workgroup holds in registers at a time: four per thread
constexpr uint32_t DP_HAPS = 8;                          // selected haplotypes per tile
constexpr uint32_t DP_ROW = DEPTH_BINS * 2;              // u64 counters of one histogram: [bin]{n_nodes, len}
constexpr uint32_t DP_ROWS = 2 + 2 * DP_HAPS;            // total, orphan, then {all, private} of the tile's haplotypes
constexpr uint32_t DP_WG_PER_CU = 5;
static_assert(64 % DP_HAPS == 0, "a tile lies in one mask word");
static_assert(DP_ROWS * DP_ROW * 8 * DP_WG_PER_CU <= 160 * 1024, "LDS of the resident workgroups");

struct DpSpecies { MemberRow m; uint32_t sel_base, pad; };   // sel_base: first selection entry of the species.  An item is a MemberChunk: tile = the selected haplotypes 8 tile .. 8 tile + 7

// the workgroup's counters -> global memory, zeroed on the way; between two barriers of the caller
__device__ __forceinline__ void dp_flush(unsigned long long *__restrict__ cnt, uint32_t species, uint32_t entry0, unsigned long long *__restrict__ hap_out,
                                         unsigned long long *__restrict__ sp_out) {
    for (uint32_t i = threadIdx.x; i < DP_ROWS * DP_ROW; i += 256u) {
        const unsigned long long x = cnt[i];
        if (x == 0ull) continue;
        cnt[i] = 0ull;
        if (i < 2u * DP_ROW) atomicAdd(sp_out + (uint64_t)species * (2u * DP_ROW) + i, x);   // (the species rows are added to only where sp_out is given)
        else atomicAdd(hap_out + (uint64_t)entry0 * (2u * DP_ROW) + (i - 2u * DP_ROW), x);   // row 2 + 2 j + class -> entry0 + j, class: the layout of hap_out
    }
}

__global__ void __launch_bounds__(256) depth_hist_kernel(uint32_t n_items, uint32_t per_block, const MemberChunk *__restrict__ items, const DpSpecies *__restrict__ tab,
                                                         const uint32_t *__restrict__ node_len, const unsigned long long *__restrict__ bases,
                                                         const unsigned long long *__restrict__ node_haps, const unsigned long long *__restrict__ mask,
                                                         const uint32_t *__restrict__ sel_hap, unsigned long long *__restrict__ hap_out /*[C][2][96][2]*/,
                                                         unsigned long long *__restrict__ sp_out /*[S][2][96][2] or null*/) {
    __shared__ unsigned long long s_cnt[DP_ROWS * DP_ROW];   // [total, orphan, all 0, private 0, all 1, ...][bin]{n_nodes, len}
    for (uint32_t i = threadIdx.x; i < DP_ROWS * DP_ROW; i += 256u) s_cnt[i] = 0ull;
    __syncthreads();
    const uint64_t begin64 = (uint64_t)blockIdx.x * per_block;
    if (begin64 >= n_items) return;                      // (uniform over the workgroup)
    const uint32_t begin = (uint32_t)begin64, end = (uint32_t)std::min<uint64_t>(begin64 + per_block, n_items);
    uint32_t cur_species = 0u, cur_entry0 = 0u, cur_tile = 0u;
    for (uint32_t c = begin; c < end; ++c) {             // (everything below is uniform over the workgroup but the thread's nodes)
        const MemberChunk it = items[c];
        const DpSpecies st = tab[it.species];
        if (c != begin && (it.species != cur_species || it.tile != cur_tile)) {
            __syncthreads();
            dp_flush(s_cnt, cur_species, cur_entry0, hap_out, sp_out);
            __syncthreads();
        }
        const uint32_t k0 = it.tile * DP_HAPS;
        cur_species = it.species; cur_tile = it.tile; cur_entry0 = st.sel_base + k0;
        const uint32_t nb = st.m.K > k0 ? std::min(DP_HAPS, st.m.K - k0) : 0u;   // haplotypes of the tile
        const uint32_t tile_bits = (1u << nb) - 1u;
        uint32_t pos[DP_HAPS];                           // route 1: where the tile's haplotypes sit in the node -> haplotype word
#pragma unroll
        for (uint32_t j = 0; j < DP_HAPS; ++j) pos[j] = (st.m.route == 1u && j < nb) ? sel_hap[st.sel_base + k0 + j] : 0u;
        const bool species_rows = it.tile == 0u && sp_out != nullptr;
        for (uint32_t t0 = 0; t0 < it.n; t0 += DP_SLAB) {
            uint32_t ln[4], tb[4], mm[4];
            unsigned long long bs[4];
            bool on[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t i = t0 + 256u * u + threadIdx.x;
                on[u] = i < it.n;
                const uint32_t v = it.first + (on[u] ? i : 0u);   // (a dead thread reads the item's first node and drops it)
                ln[u] = node_len[v]; bs[u] = bases[v];
                uint32_t m = 0u, t = 0u;
                if (st.m.route == 1u) {
                    const unsigned long long word = node_haps[v] & st.m.bits;
                    m = (uint32_t)__popcll(word);
#pragma unroll
                    for (uint32_t j = 0; j < DP_HAPS; ++j) t |= (uint32_t)((word >> pos[j]) & 1ull) << j;
                } else if (st.m.route == 2u) {
                    const uint64_t row = member_mask_row(st.m, v);
                    const uint32_t wt = k0 >> 6, sh = k0 & 63u;
                    for (uint32_t w = 0; w < st.m.nw; ++w) {
                        const unsigned long long x = mask[row + w];
                        m += (uint32_t)__popcll(x);
                        t = w == wt ? (uint32_t)(x >> sh) : t;
                    }
                }
                tb[u] = t & tile_bits;
                mm[u] = m;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!on[u]) continue;
                const uint32_t q = 2u * depth_bin(node_depth(bs[u], ln[u]));
                const unsigned long long len = ln[u];
                if (species_rows) {
                    atomicAdd(&s_cnt[q], 1ull); atomicAdd(&s_cnt[q + 1u], len);
                    if (mm[u] == 0u) { atomicAdd(&s_cnt[DP_ROW + q], 1ull); atomicAdd(&s_cnt[DP_ROW + q + 1u], len); }
                }
                for (uint32_t r = tb[u]; r; r &= r - 1u) {
                    const uint32_t row = 2u + 2u * (uint32_t)__builtin_ctz(r);
                    atomicAdd(&s_cnt[row * DP_ROW + q], 1ull); atomicAdd(&s_cnt[row * DP_ROW + q + 1u], len);
                    if (mm[u] == 1u) { atomicAdd(&s_cnt[(row + 1u) * DP_ROW + q], 1ull); atomicAdd(&s_cnt[(row + 1u) * DP_ROW + q + 1u], len); }
                }
            }
        }
    }
    __syncthreads();
    dp_flush(s_cnt, cur_species, cur_entry0, hap_out, sp_out);
}

}  // namespace

// sel_off [S+1], sel_hap validated by the caller (in range, no repeats within a species); species_out may be null
int depth_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, uint64_t *hap_out, uint64_t *species_out) {
    const uint32_t S = db->S;
    const uint64_t C = sel_off[S];
    if (C >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_depth: %llu selection entries exceed 32-bit positions", (unsigned long long)C);
    if (db->V >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_depth: %llu nodes exceed 32-bit positions", (unsigned long long)db->V);
    const bool by_node = member_by_node(db->nh_built, ctx->cfg.depth_route);
    const bool want_species = species_out != nullptr;
    std::vector<DpSpecies> tab(S ? S : 1);
    std::vector<MemberChunk> items;
    MemberPass ps;
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = sel_off[s + 1] - sel_off[s];
        tab[s] = DpSpecies{ps.wm.row(db, s, by_node, sel_hap + sel_off[s], K), (uint32_t)sel_off[s], 0u};
        const uint64_t tiles = K ? (K + DP_HAPS - 1) / DP_HAPS : (want_species ? 1 : 0);   // nothing selected: the species rows alone
        member_chunks_add(items, s, db->h_node_off[s], db->h_node_off[s + 1], DP_CHUNK, tiles);
    }
    if (items.size() >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_depth: %llu chunks of nodes", (unsigned long long)items.size());
    const size_t n_hap = (size_t)C * 2 * DP_ROW, n_sp = want_species ? (size_t)S * 2 * DP_ROW : 0;
    if (n_hap + n_sp == 0) return 0;
    DevBuf<DpSpecies> d_tab;
    DevBuf<uint32_t> d_sel_hap;
    DevBuf<MemberChunk> d_items;
    PTX_TRY(ps.open(ctx, db, n_hap + n_sp));   // one device block, zero-filled once: [hap C x 2 x 96 x 2][species S x 2 x 96 x 2]
    const uint32_t none = 0;
    if (!items.empty()) {
        PTX_TRY(upload(ctx, d_tab, tab.data(), tab.size()));
        PTX_TRY(upload(ctx, d_sel_hap, C ? sel_hap : &none, C ? (size_t)C : 1));
        PTX_TRY(upload(ctx, d_items, items.data(), items.size()));
        const int grid = grid_for(items.size(), 1, ctx->cfg.depth_grid > 0 ? ctx->cfg.depth_grid : ctx->n_cu * (int)DP_WG_PER_CU);
        const uint32_t per_block = (uint32_t)((items.size() + grid - 1) / grid);
        KTimer tm(ctx, "depth_hist_kernel");
        hipLaunchKernelGGL(depth_hist_kernel, dim3(grid), dim3(256), 0, ctx->stream, (uint32_t)items.size(), per_block, d_items.p, d_tab.p, db->d_node_len.p,
                           db->d_bases.p, by_node ? (const unsigned long long *)db->d_node_haps.p : (const unsigned long long *)nullptr, ps.wm.d_mask.p, d_sel_hap.p,
                           ps.d_out.p, want_species ? ps.d_out.p + n_hap : (unsigned long long *)nullptr);
    }
    return ps.close(ctx, hap_out, n_hap, species_out, n_sp);
}

}  // namespace ptx
