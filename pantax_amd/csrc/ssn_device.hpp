// ssn_device.hpp -- what the files of the node-order row sort share: sample_sort_nodes.hip (the entry point: checks, plan, the phases in order),
// ssn_sample.hip (samples -> splitter tree; a small segment sorted whole), ssn_node_pass.hip (the pass over the nodes: bucket ids, count matrix, staged
// rows), ssn_partition.hip (bucket starts, scatter, tie fills), ssn_local.hip (the sorts inside a bucket) and ssn_patterns.hip (runs of equal mask).
// The key, the kernels' one argument (Sn), a node's mask / abundance / covered bases for the samplers, the statistics partial of the fused pass, the
// splitter tree's indexing, a workgroup's tile range, the LDS bitonic network, and the host launch functions of every stage.  Constants the host
// needs too are ssn_plan.hpp's.
#pragma once
#include "primitives.hpp"
#include "wave.hpp"
#include "ssn_plan.hpp"

namespace ptx {

constexpr int SN_NSPLIT = SN_NLEAF - 1;          // 1023 splitters: three to four valid samples between two of them
constexpr int SN_CAP = 4096;
constexpr int SN_WAVE_CAP = 512;                 // rows a wave of the first local kernel sorts in registers (eight per lane)
constexpr int SN_WAVE_CAP2 = 1024;               // ... of the second one (sixteen per lane: more registers, fewer waves in flight)
constexpr uint16_t SN_NO_ROW = 0xFFFFu;
static_assert(sizeof(NodePartial) == 4 * SN_NODE_PARTIAL_WORDS && alignof(NodePartial) == 8, "ssn_plan lays out [S x G] NodePartial at an even word offset");

struct Key2 { uint64_t m, a; };
__device__ __forceinline__ bool less2(const Key2 &x, const Key2 &y) { return (x.m < y.m) | ((x.m == y.m) & (x.a < y.a)); }
__device__ __forceinline__ bool eq2(const Key2 &x, const Key2 &y) { return (x.m == y.m) & (x.a == y.a); }

struct Sn {
    const uint32_t *node_base;   // [S + 1] (device)
    const double *ab;            // [V] a_v (0 = no row)
    const uint64_t *mask;        // [V] membership mask (0 = no row); null: formed from the haplotype words (hp)
    RowMaskSource hp;
    NodeCovSource fz;            // fz.bases != null: the fused node pass -- no `ab`, no hp.cov; a and the covered bases are formed from the coverage arena
    NodePartial *npart;          // [S x G] fused: the statistics of the nodes a partition workgroup walked (a small segment: entry 0, from the sample kernel)
    uint32_t *ws;                // S x SN_WS_WORDS
    uint32_t *cntm;              // S x G x SN_NBUCKET: counts, then first slots
    uint16_t *ids;               // [V] bucket id of every staged row (same places as `stage`)
    uint32_t *stage_cnt;         // [S x G] rows a partition workgroup staged
    double *c0p, *c0;            // [S x G] / [S] (c0 null: not wanted) sum of the abundances of the nodes with a > 0 and an EMPTY mask: no rows, but |0 - a| of the objective
    uint32_t *seg_n, *seg_out;   // [S] rows of a segment, [S + 1] its first output row
    ulonglong2 *stage;           // [V] scratch: the rows that have to travel (even buckets), compacted per partition workgroup from the node of its first tile on
    ulonglong2 *rows;            // [V] scratch: those rows bucket by bucket, segment s from node_base[s]
    uint64_t *ksp, *km, *ka;     // output: {species, mask, a} (ksp null: species << pack_shift | mask in km)
    int pack_shift;
    uint32_t G, per;             // partition workgroups per segment, tiles each of them walks
    uint32_t skip_empty;         // segments without LP columns are not read by the histogram pass (option no_absent_skip: 0)
    uint32_t ablate;             // -DSSN_ABLATE / -DNODE_ROWS_ABLATE builds: parts of ssn_hist_kernel / node_rows_kernel left out (measurements; the results are wrong)
    uint32_t keys_all;           // 1: every row gets its key words (km, ksp) -- the caller reads them (pantax_hip_sort_rows); 0: only the rows ssn_heads_kernel reads do
                                 // (sn_keys_needed(), decided by sample_sort_nodes): `ka` is all the step keeps of the sorted rows
    __device__ __forceinline__ uint32_t *w(uint32_t s) const { return ws + (size_t)s * SN_WS_WORDS; }
    __device__ __forceinline__ uint64_t key_word(uint32_t s, uint64_t m) const { return pack_shift >= 0 ? (((uint64_t)s << pack_shift) | m) : m; }
    __device__ __forceinline__ void put(uint32_t s, uint32_t pos, uint64_t m, uint64_t a) const {
        km[pos] = key_word(s, m); ka[pos] = a;
        if (ksp) ksp[pos] = s;
    }
    // a row whose key words only ssn_heads_kernel could want: `read` = it lies where that kernel looks (a mixed bucket pair)
    __device__ __forceinline__ void put_if(bool read, uint32_t s, uint32_t pos, uint64_t m, uint64_t a) const {
        ka[pos] = a;
        if (keys_all || read) { km[pos] = key_word(s, m); if (ksp) ksp[pos] = s; }
    }
};

// mask == null: the membership mask of node v of segment (= species) s from its haplotype word -- bit k of the mask = some haplotype of
// column k visits the node (what mask_nodes_kernel writes, stage_lp_rows.hip); the plain loop, for the few nodes the samplers look at
__device__ __forceinline__ uint64_t sn_node_mask(const Sn &sn, uint32_t s, uint64_t v) {
    if (sn.mask) return sn.mask[v];
    const int p = sn.hp.sp_p[s];
    const uint64_t h0 = sn.hp.hap_off[s], nh = sn.hp.hap_off[s + 1] - h0;
    if (p <= 0 || p > 64 || nh > 64) return 0ull;
    unsigned long long hm = sn.hp.node_haps[v];
    uint64_t m = 0;
    while (hm) { const int j = __ffsll((long long)hm) - 1; hm &= hm - 1; const int bit = sn.hp.hap_bit[h0 + j]; if (bit >= 0) m |= 1ull << bit; }
    return m;
}

// fused node pass: the abundance and the covered bases of ONE node from the coverage arena (what node_cov_stats_kernel writes to `ab` / `cov`), for the
// few nodes the samplers look at
template <bool FUSED>
__device__ __forceinline__ double sn_node_ab(const Sn &sn, uint64_t v) {
    if constexpr (!FUSED) return sn.ab[v];
    return (double)(long long)sn.fz.bases[v] / (double)sn.hp.node_len[v];     // profile.rs:987-988
}
template <bool FUSED>
__device__ __forceinline__ uint32_t sn_node_cov(const Sn &sn, uint64_t v) {
    if constexpr (!FUSED) return sn.hp.cov[v];
    const uint32_t l = sn.hp.node_len[v];
    if ((sn.fz.full[v >> 5] >> (v & 31u)) & 1u) return l;                     // a step covered the whole node: a flag instead of marked bits
    if (l == 0u) return 0u;
    const uint64_t g0 = sn.fz.bit_off[v], g1 = g0 + l, w0 = g0 >> 5, w1 = (g1 - 1) >> 5;
    const uint32_t m0 = 0xFFFFFFFFu << (g0 & 31), m1 = 0xFFFFFFFFu >> (31 - (uint32_t)((g1 - 1) & 31));
    if (w0 == w1) return (uint32_t)__popc(sn.fz.bitmap[w0] & m0 & m1);
    uint32_t c = (uint32_t)__popc(sn.fz.bitmap[w0] & m0) + (uint32_t)__popc(sn.fz.bitmap[w1] & m1);
    for (uint64_t w = w0 + 1; w < w1; ++w) c += (uint32_t)__popc(sn.fz.bitmap[w]);
    return c;
}
struct NodeAcc {                                                              // a thread's share of a NodePartial
    double mx = -INFINITY, zs = 0.0;
    unsigned long long nv = 0, zc = 0;
    __device__ __forceinline__ void add(double ab, double min_depth) {
        mx = fmax(mx, ab);
        if (ab > 0.0) ++nv;
        const double o = ab > min_depth ? ab : 0.0;                           // :2941-2944
        if (o > 0.0) { zs += o; ++zc; }
    }
};
// the workgroup's NodePartial in a fixed shape (every thread its nodes in order, a wave reduction, the waves in order): the same bits from run to run
template <int NW>
__device__ __forceinline__ void sn_block_partial(NodeAcc a, NodePartial *dst) {
    __shared__ double s_mx[NW], s_zs[NW];
    __shared__ unsigned long long s_nv[NW], s_zc[NW];
    a.mx = wave_reduce(a.mx, [](double x, double y) { return fmax(x, y); });
    a.zs = wave_reduce(a.zs, [](double x, double y) { return x + y; });
    a.nv = wave_reduce(a.nv, [](unsigned long long x, unsigned long long y) { return x + y; });
    a.zc = wave_reduce(a.zc, [](unsigned long long x, unsigned long long y) { return x + y; });
    if ((threadIdx.x & 63) == 0) { const int q = threadIdx.x >> 6; s_mx[q] = a.mx; s_zs[q] = a.zs; s_nv[q] = a.nv; s_zc[q] = a.zc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        NodePartial p{s_mx[0], s_zs[0], s_nv[0], s_zc[0]};
        for (int q = 1; q < NW; ++q) { p.mx = fmax(p.mx, s_mx[q]); p.zs += s_zs[q]; p.nv += s_nv[q]; p.zc += s_zc[q]; }
        *dst = p;
    }
    __syncthreads();
}

// sorted rank (0-based, among the SN_NSPLIT splitters) of tree node k, and back
__device__ __forceinline__ uint32_t tree_rank(uint32_t k) {
    const uint32_t l = 31u - (uint32_t)__builtin_clz(k), p = k - (1u << l);
    return ((2u * p + 1u) << ((uint32_t)SN_LEVELS - 1u - l)) - 1u;
}
__device__ __forceinline__ uint32_t tree_node(uint32_t rank) {
    const uint32_t q = rank + 1u, tz = (uint32_t)__builtin_ctz(q);
    return (1u << ((uint32_t)SN_LEVELS - 1u - tz)) + ((q >> tz) >> 1);
}

// Bucket ids of N keys {km, ka} at once, level by level: at every level the N tree nodes are read from LDS together, one wait covers them, then the N
// compares follow -- SN_LEVELS + 1 dependent LDS round trips for the N keys where a descent per key makes N times as many.  Branch-free: every lane
// descends with whatever key it holds (any key stays inside the tree: node k of level l lies in [2^l, 2^(l+1)), so every read is of tree[1 .. SN_NLEAF - 1]),
// and a lane without a row discards its id.  The id is the serial loop's: lo = the splitters less than the key, 2 lo + 1 when the key equals splitter
// lo ("equal to splitter j" is its own bucket), the probe of a key above every splitter (lo = SN_NSPLIT: no such splitter) reads splitter 0 and is ignored.
template <int N>
__device__ __forceinline__ void sn_bucket_ids(const ulonglong2 *tree, const uint64_t (&km)[N], const uint64_t (&ka)[N], uint32_t (&id)[N]) {
    uint32_t k[N];                                               // 16 k through the levels: the node's byte offset, one shift a level saved
    ulonglong2 nd[N];
#pragma unroll
    for (int r = 0; r < N; ++r) k[r] = 16u;
#pragma unroll
    for (int l = 0; l < SN_LEVELS; ++l) {
#pragma unroll
        for (int r = 0; r < N; ++r) nd[r] = *reinterpret_cast<const ulonglong2 *>(reinterpret_cast<const char *>(tree) + k[r]);
#pragma unroll
        for (int r = 0; r < N; ++r) k[r] = (k[r] << 1) | (less2(Key2{nd[r].x, nd[r].y}, Key2{km[r], ka[r]}) ? 16u : 0u);
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
        k[r] = (k[r] >> 4) - (uint32_t)SN_NLEAF;                 // splitters less than the key
        nd[r] = tree[tree_node(k[r] < (uint32_t)SN_NSPLIT ? k[r] : 0u)];
    }
#pragma unroll
    for (int r = 0; r < N; ++r) id[r] = 2u * k[r] + (((k[r] < (uint32_t)SN_NSPLIT) & eq2(Key2{nd[r].x, nd[r].y}, Key2{km[r], ka[r]})) ? 1u : 0u);
}

// Bucket pair j (the even bucket 2j: the rows between splitters j - 1 and j; the tie bucket 2j + 1: the copies of splitter j) is MIXED when its even bucket
// may hold rows of more than one mask: the two splitters differ in their mask, or one of them does not exist (pair 0, the last pair).  Otherwise every row
// of bucket 2j has the mask of splitter j (*mv): the local sorts move `a` alone through their networks and store no key words for it (Sn::keys_all == 0),
// and ssn_heads_kernel, which reads the rows of the mixed pairs only, never looks at it.  The one spelling both sides share.
__device__ __forceinline__ bool sn_pair_mixed(const ulonglong2 *__restrict__ tree, uint32_t j, uint64_t *mv = nullptr) {
    if (j == 0 || j >= (uint32_t)SN_NSPLIT) { if (mv) *mv = 0; return true; }
    const uint64_t ma = tree[tree_node(j - 1)].x, mb = tree[tree_node(j)].x;
    if (mv) *mv = mb;
    return ma != mb;
}

// the tiles [t0, t1) of workgroup g of a segment of n nodes
__device__ __forceinline__ void sn_tiles(const Sn &sn, uint32_t n, uint32_t g, uint32_t &t0, uint32_t &t1) {
    const uint32_t nt = (n + SN_TILE - 1) / SN_TILE;
    t0 = g * sn.per; t1 = t0 + sn.per;
    if (t0 > nt) t0 = nt;
    if (t1 > nt) t1 = nt;
}

template <int NT>
__device__ __forceinline__ void bitonic2(uint64_t *km, uint64_t *ka, uint32_t N) {
    for (uint32_t k = 2; k <= N; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < N / 2; t += NT) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const Key2 x{km[i], ka[i]}, y{km[l], ka[l]};
                const bool up = (i & k) == 0;
                if (up ? less2(y, x) : less2(x, y)) { km[i] = y.m; ka[i] = y.a; km[l] = x.m; ka[l] = x.a; }
            }
            __syncthreads();
        }
}

// -DSSN_ABLATE + option ssn_ablate (tools/r6_ssn_ablate.sh): parts of ssn_hist_kernel left out, see there (measurements; the results are wrong)
#ifdef SSN_ABLATE
#define SSN_ABL(b) ((sn.ablate & (b)) != 0u)
#else
#define SSN_ABL(b) false
#endif
// -DNODE_ROWS_ABLATE + the same option: parts of node_rows_kernel left out -- 1 no bit-vector loads (covered bases of a node without a full-node flag: 0),
// 2 no tree descent (measurements; the results are wrong)
#ifdef NODE_ROWS_ABLATE
#define NRK_ABL(b) ((sn.ablate & (b)) != 0u)
#else
#define NRK_ABL(b) false
#endif

// ---- host side: the stages, each in the file that holds its kernels.  All enqueue on ctx->stream, S = the number of segments (grid.y or grid.x of
// every launch); the entry point times them under its KTimer labels and asks for the launch error once, at the end ----
// ssn_sample.hip: ssn_gather_kernel + ssn_sample_kernel<fused>
void ssn_sample_launch(Ctx *ctx, const Sn &sn, uint32_t S, bool fused);
// ssn_node_pass.hip: the resident step's one pass (node_rows_kernel + node_rows_final_kernel), or its two-kernel twin ssn_hist_kernel<haps>;
// max_haps sizes the column tables in dynamic LDS; node_bits (ssn_node_bits(), ssn_plan.hpp): 0 every node gathers its bit-vector words, 1 / 2 an item's
// stretch of the bit vector is loaded whole, that many words a lane
void ssn_node_rows_launch(Ctx *ctx, const Sn &sn, uint32_t S, uint32_t max_haps, int node_bits);
void ssn_hist_launch(Ctx *ctx, const Sn &sn, uint32_t S, bool haps, uint32_t max_haps);
// ssn_partition.hip: bucket starts and the segments' first output rows (*d_n = the row count); the travelling rows into their buckets; the tie buckets
// as fills (tie_grid: SsnPlan's)
void ssn_offsets_launch(Ctx *ctx, const Sn &sn, uint32_t S, uint32_t *d_n);
void ssn_scatter_launch(Ctx *ctx, const Sn &sn, uint32_t S);
void ssn_ties_launch(Ctx *ctx, const Sn &sn, uint32_t S, uint32_t tie_grid);
// ssn_local.hip: ssn_local_wave_kernel, ssn_local_wave2_kernel, ssn_local_kernel
void ssn_local_launch(Ctx *ctx, const Sn &sn, uint32_t S);
// ssn_patterns.hip: heads, their scan and the pattern tables; sub_k: [S][SN_NWH] words of the workspace
void ssn_patterns_launch(Ctx *ctx, const Sn &sn, uint32_t S, uint32_t *sub_k, const RowPatterns &pat, const uint32_t *d_n);

}  // namespace ptx
