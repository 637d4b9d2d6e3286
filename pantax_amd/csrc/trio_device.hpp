// trio_device.hpp -- what the files of the unique-trio index (a7) share: stage_trio.hip (the build as named phases, the export order),
// stage_trio_tables.hip (the upload-time visit and run tables), stage_trio_uniq.hip (uniqueness: visit table, node blocks, buckets) and
// stage_trio_rows.hip (filing the rows).  The tile loop over the walks, the canonical window, the constants of the visit table, what filing a
// row writes (RowOut), and the host phases trio_index_build calls in the files that hold their kernels.
#pragma once
#include "primitives.hpp"
#include "wave.hpp"
#include "trio_plan.hpp"

namespace ptx {

// Work decomposition of every per-path-step kernel: one workgroup per tile = PATH_TILE consecutive
// positions of ONE haplotype (tile table built at db upload).  Tiles are ordered (species, chunk, hap):
// the haplotypes of a species are largely collinear, so neighbouring workgroups touch the same node
// buckets at the same time (L2 write-combining of the bucket scatter) and no per-position search for the
// owning haplotype is needed.
#define TRIO_GRAPH_ARGS const uint2 *__restrict__ tiles, const uint64_t *__restrict__ path_off, const uint32_t *__restrict__ path_nodes, \
                        const uint32_t *__restrict__ hap_species, const uint32_t *__restrict__ node_base
#define TILE_LOOP(q, h, qend)                                                         \
    const uint2 tile__ = tiles[blockIdx.x];                                           \
    const bool pad__ = tile__.x == 0xFFFFFFFFu;   /* filler that keeps chunk groups XCD-aligned */ \
    const uint32_t h = pad__ ? 0u : tile__.x;                                         \
    const uint64_t qend = pad__ ? 0ull : path_off[h + 1];                             \
    const uint64_t qt0__ = pad__ ? 0ull : path_off[h] + (uint64_t)tile__.y * PATH_TILE; \
    for (uint64_t q = qt0__ + threadIdx.x; q < qt0__ + PATH_TILE && q < qend; q += 256)

// canonical window that STARTS at q of hap h (profile.rs:672-678: the ends are swapped when w[0] > w[2], the middle stays):
// (a, b, c) = (smaller end, middle, larger end); false if q starts no window.  Every occurrence of a window -- either
// orientation, any haplotype -- has the same MIDDLE node, so g = the global index of b is the key every table of the index is
// grouped by (round 4; rounds 1-3 grouped by the smaller end, which made a position own up to two windows).
__device__ __forceinline__ bool window_of(uint64_t q, uint64_t qend, uint32_t nb, const uint32_t *__restrict__ path_nodes, uint32_t &g,
                                          uint32_t &a, uint32_t &b, uint32_t &c) {
    if (q + 2 >= qend) return false;
    a = path_nodes[q]; b = path_nodes[q + 1]; c = path_nodes[q + 2];
    if (a > c) { uint32_t t = a; a = c; c = t; }
    g = nb + b;
    return true;
}

// the visit table (stage_trio_tables.hip builds it, stage_trio_uniq.hip and stage_trio_rows.hip read it): interior positions of the walks node by
// node in groups of 64; TRIO_BLK / VIS_CHUNK_SHIFT, which the host-side tables are cut by as well, are trio_plan.hpp's
constexpr uint32_t VIS_PAD = 0xFFFFFFFFu;
constexpr int VIS_MAX = 64;            // visits of a node that one wave decides
struct __attribute__((packed, aligned(4))) U32x3 { uint32_t x, y, z; };
constexpr int VIS_REC = 8;             // records {window start, smaller end, larger end, middle} a group hands to trio_rows_kernel (trio_visit_kernel<.., ROWS>)

// ---- rows of the index ----------------------------------------------------------------------------------------------------------------
// A ROW is a unique window; its number is the place it is FILED at (round 5; rounds 1-4 numbered the rows in (species, hap, position) order,
// which cost a flag bit per path position, the ranks of those flags and a scattered store per row: 15.5 GB of traffic for 6 GB of payload at
// 1e4 strains).  Everything the step reads is indexed by that number: the lookup entry {smaller end, larger end} (the coverage pass finds a
// window under its MIDDLE node, whose record carries {first row, #rows}), the window's length (profile.rs:712), the haplotype that owns it,
// and the coverage pass's trio_bases.  The rows of a node are neighbours, sorted by their pair of ends -- a canonical order, the same on
// every build and on both routes of stage_trio_rows.hip -- and the rows of a species are one block.

// the haplotype whose walk holds path position q: last h in [h0, h1) with path_off[h] <= q
__device__ __forceinline__ uint32_t hap_of_position(const uint64_t *__restrict__ path_off, uint32_t h0, uint32_t h1, uint32_t q) {
    uint32_t lo = h0, hi = h1;
    while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if (path_off[mid] <= (uint64_t)q) lo = mid; else hi = mid; }
    return lo;
}
// what filing a row writes (dense stores in row order) -- KEYS: also the window start, from which the exporters make the
// (species, hap, position) order; FIRST (first build of a db): the rows per haplotype are counted (-> hap_trio_off)
struct RowOut {
    const uint32_t *node_len;
    const uint64_t *path_off, *hap_off;
    uint2 *ent;
    trio_len_t *len;
    uint16_t *hap;
    uint32_t *q;
    uint32_t *hap_cnt;
    __device__ __forceinline__ void put_len_hap(uint32_t row, uint32_t l, uint32_t h) const {
#if TRIO_LH_PACK
        len[row] = make_uint2(l, h);
#else
        len[row] = l; hap[row] = (uint16_t)h;
#endif
    }
};
// FIRST builds count the rows per haplotype.  One memory-side atomic per row on the ten counters of the species every wave of the GPU is filing at that
// moment took 104 ms at 1e4 strains (1.8e8 adds on 1e4 addresses, `r05_cfg4_kernel_stats`): a workgroup of the rows kernel counts in an LDS window of
// 1024 haplotypes from the species of its first group on (groups are in species order) and adds what it counted once, at its end.
constexpr uint32_t HAPCNT_WIN = 1024;
struct HapCount {
    uint32_t *lds;       // [HAPCNT_WIN] or null: straight to memory
    uint32_t base;       // global haplotype of lds[0]
    uint32_t *glob;
    __device__ __forceinline__ void add(uint32_t h) const {
        const uint32_t rel = h - base;
        if (lds && rel < HAPCNT_WIN) atomicAdd(&lds[rel], 1u); else atomicAdd(&glob[h], 1u);
    }
};
template <bool KEYS, bool FIRST>
__device__ __forceinline__ void row_file(const RowOut &o, uint32_t row, uint32_t q0, uint32_t lo, uint32_t hi, uint32_t mid, uint32_t sp, const HapCount &hc) {
    const uint32_t h0 = (uint32_t)o.hap_off[sp], h = hap_of_position(o.path_off, h0, (uint32_t)o.hap_off[sp + 1], q0);
    o.ent[row] = make_uint2(lo, hi);
    o.put_len_hap(row, o.node_len[lo] + o.node_len[mid] + o.node_len[hi], h - h0);
    if (KEYS) o.q[row] = q0;
    if (FIRST) hc.add(h);
}

// ---- host side ----
// the graph arguments of the kernels declared with TRIO_GRAPH_ARGS
#define TRIO_GRAPH(db) (db)->d_tiles.p, (db)->d_path_off.p, (db)->d_path_nodes.p, (db)->d_hap_species.p, (db)->d_node_base.p

// The phases of trio_index_build (stage_trio.hip) that launch kernels, each in the file that holds them; all enqueue on ctx->stream and follow the
// plan -- none decodes an option (tv_ablate, the word of -DTV_ABLATE builds, is handed through to the visit kernel as it is).
// stage_trio_uniq.hip: one flag bit per unique window start + the count of unique windows per node (visit kernel on the fast route: ballots + records)
int trio_visit_launch(Ctx *ctx, Db *db, const TrioPlan &pl);
int trio_block_launch(Ctx *ctx, Db *db, const TrioPlan &pl);
int trio_bucket_launch(Ctx *ctx, Db *db, const TrioPlan &pl);
// stage_trio_rows.hip: the one-pass rebuild; the first row of every group (fast route) and of every node (path route); the rows of either route
int trio_file_launch(Ctx *ctx, Db *db, const TrioPlan &pl, const RowOut &ro);
int trio_group_prefix(Ctx *ctx, Db *db, const TrioPlan &pl);
int trio_head_scan(Ctx *ctx, Db *db, const TrioPlan &pl);
int trio_rows_launch(Ctx *ctx, Db *db, const TrioPlan &pl, const RowOut &ro);
int trio_path_rows_launch(Ctx *ctx, Db *db, const TrioPlan &pl, const RowOut &ro);

}  // namespace ptx
