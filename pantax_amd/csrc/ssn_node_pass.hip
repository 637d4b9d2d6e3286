// ssn_node_pass.hip -- node-order row sort, stage 2: the pass over the nodes.  Bucket id of every row (ten tree levels; "equal to splitter j" is its
// own bucket 2j+1), one LDS histogram per workgroup stored as a row of the segment's count matrix, the rows of the even buckets staged.
//
// EDIT TOGETHER.  This file holds two kernels and nothing else: ssn_hist_kernel<HAPS> (the stage calls and fallbacks) and node_rows_kernel (the
// resident step, fused with the node statistics; node_rows_final_kernel folds its partials).  They stay two kernels -- one shared body cost
// ssn_hist_kernel<true> 115 -> 127 VGPRs (see below).  What the two have in common, statement for statement, and has to be edited in both:
//   * the columns' sums of a node (c8 / l8 in registers, the columns beyond 8 by LDS atomics), the c0 sum, the row test (a > 0 and a mask), the
//     histogram atomic, the ballot and the staging of the row;
//   * the three epilogues (count matrix row, c0 partial, column sums).
// What differs since the bucket ids of node_rows_kernel are formed level by level for a half's four items (sn_bucket_ids, ssn_device.hpp):
//   * ssn_hist_kernel descends the tree per row, inside the row test (ten dependent LDS reads an item) -- the loop -DNODE_ROWS_SERIAL_DESCENT puts back
//     into node_rows_kernel for A/B builds.  Both spell the same bucket id: lo = the splitters less than the key, 2 lo + 1 for a copy of splitter lo;
//   * node_rows_kernel looks its column tables up four bytes at a time (its register peak), ssn_hist_kernel as the compiler unrolls them.
#include <type_traits>
#include "ssn_device.hpp"

namespace ptx {

namespace {
// HAPS: no mask array -- the mask of a node is formed here from its haplotype word through byte-wise column tables in (dynamic) LDS, and the
// candidates' covered bases and lengths (path_cov_ratio, profile.rs:1344-1361) are summed while it is in a register: mask_nodes_kernel's
// pass (16V in, 8V out) and this pass's own 8V of masks are gone
// -DSSN_ABLATE + option ssn_ablate (tools/r6_ssn_ablate.sh): 1 no column tables, 2 no column sums, 4 no sums beyond column 8, 8 no tree descent, 16 no
// histogram, 32 nothing staged.  Round 6 at cfg4: 1.98 ms whole, 1.34 ms with ALL of them left out -- the kernel is its four input streams (24 B a node
// at 4.5 TB/s); the LDS conflicts round 5's counters showed cost 0.1 ms (tables), 0.1 (sums), 0 (histogram), and 512-thread workgroups (six waves per
// SIMD behind the same tables instead of four) were slower, 2.06 ms
template <bool HAPS>
__global__ void __launch_bounds__(256) ssn_hist_kernel(Sn sn) {
    __shared__ ulonglong2 tree[SN_NLEAF];
    __shared__ uint32_t s_hist[SN_NBUCKET];
    extern __shared__ unsigned long long s_dyn_tab[];             // HAPS: [nbyte][256] columns of the haplotypes 8b .. 8b+7 set in a byte value
    __shared__ int s_bit[64];
    __shared__ unsigned long long s_acc[2 * 64];
    const uint32_t s = blockIdx.y, g = blockIdx.x, o = sn.node_base[s], n = sn.node_base[s + 1] - o;
    uint32_t *w = sn.w(s);
    if (n == 0 || w[SN_OFF_FLAGS] != 0) return;
    // a species without LP columns (the species level dropped it, or no haplotype passed the first filter) has no rows: an empty histogram, nothing staged,
    // nothing read (round 6: the work follows the species that are present in the sample; its c0 is never used -- objective_rows_kernel leaves such species out)
    if (HAPS && sn.skip_empty && sn.hp.sp_p[s] <= 0) {           // (workgroup-uniform)
        uint32_t *row0 = sn.cntm + ((size_t)s * sn.G + g) * SN_NBUCKET;
        for (int i = threadIdx.x; i < SN_NBUCKET; i += 256) row0[i] = 0u;
        if (threadIdx.x == 0) { sn.stage_cnt[(size_t)s * sn.G + g] = 0u; if (sn.c0) sn.c0p[(size_t)s * sn.G + g] = 0.0; }
        return;
    }
    uint32_t t0, t1;
    sn_tiles(sn, n, g, t0, t1);
    const ulonglong2 *gt = reinterpret_cast<const ulonglong2 *>(w + SN_OFF_TREE);
    __shared__ uint32_t s_nstage;
    for (int i = threadIdx.x; i < SN_NBUCKET; i += 256) s_hist[i] = 0;
    if (threadIdx.x == 0) s_nstage = 0;
    if (t0 < t1) for (int i = threadIdx.x; i < SN_NLEAF; i += 256) tree[i] = gt[i];
    int p0 = 0, nbyte = 0;
    uint64_t h0 = 0;
    if (HAPS) {
        h0 = sn.hp.hap_off[s];
        const uint64_t nh = sn.hp.hap_off[s + 1] - h0;
        p0 = sn.hp.sp_p[s];
        if (p0 <= 0 || p0 > 64 || nh > 64) p0 = 0;                // no columns (or a species the path walk serves: never with HAPS)
        nbyte = p0 ? (int)((nh + 7) / 8) : 0;
        if (threadIdx.x < 64) s_bit[threadIdx.x] = (p0 && threadIdx.x < nh) ? sn.hp.hap_bit[h0 + threadIdx.x] : -1;
        if (threadIdx.x < 128) s_acc[threadIdx.x] = 0;
    }
    __syncthreads();
    if (HAPS) {
        for (int b = 0; b < nbyte; ++b) {
            unsigned long long e = 0ull;
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int bit = s_bit[8 * b + i]; if (((threadIdx.x >> i) & 1u) && bit >= 0) e |= 1ull << bit; }
            s_dyn_tab[b * 256 + threadIdx.x] = e;
        }
        __syncthreads();
    }
    unsigned long long c8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, l8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // The rows of the EVEN buckets are the only ones that travel (a tie bucket is written as a fill): they are staged here, compacted and
    // with their bucket id, in the node range of this workgroup's tiles -- the scatter pass reads 18 bytes per such row instead of
    // abundance, mask and an id of EVERY node again
    const uint32_t stage0 = o + t0 * SN_TILE;
    const int lane = threadIdx.x & 63;
    double cacc = 0.0;                                           // abundances of this thread's nodes with an empty mask
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t base = t * SN_TILE + threadIdx.x;
        double av[SN_ITEMS];
        uint64_t mv[SN_ITEMS];
        uint32_t cv[SN_ITEMS], lv[SN_ITEMS];
#pragma unroll
        for (int r = 0; r < SN_ITEMS; ++r) {
            const uint32_t i = base + (uint32_t)r * 256u;
            av[r] = 0.0; mv[r] = 0; cv[r] = 0; lv[r] = 0;
            if (i < n) {
                av[r] = sn.ab[o + i];
                if (HAPS) { mv[r] = sn.hp.node_haps[o + i]; cv[r] = sn.hp.cov[o + i]; lv[r] = sn.hp.node_len[o + i]; }
                else mv[r] = sn.mask[o + i];
            }
        }
#pragma unroll
        for (int r = 0; r < SN_ITEMS; ++r) {
            if (HAPS) {                                           // haplotype word -> columns, and the columns' sums
                const unsigned long long hm = mv[r];
                unsigned long long m = 0ull;
                if (SSN_ABL(1u)) m = hm & ((p0 >= 64 ? 0ull : (1ull << p0)) - 1ull);
                else
                for (int b = 0; b < nbyte; ++b) m |= s_dyn_tab[b * 256 + (int)((hm >> (8 * b)) & 255ull)];
                mv[r] = m;
                if (m && !SSN_ABL(2u)) {
                    const unsigned long long c = cv[r], l = lv[r];
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < p0) { const bool on = (m >> k) & 1ull; c8[k] += on ? c : 0ull; l8[k] += on ? l : 0ull; }   // (block-uniform: the columns that exist)
                    unsigned long long rest = SSN_ABL(4u) ? 0ull : m >> 8;
                    while (rest) {
                        const int k = __ffsll((long long)rest) - 1 + 8;
                        rest &= rest - 1;
                        if (c) atomicAdd(&s_acc[2 * k], c);
                        atomicAdd(&s_acc[2 * k + 1], l);
                    }
                }
            }
            uint32_t id = SN_NO_ROW;
            const uint64_t abits = (uint64_t)__double_as_longlong(av[r]);
            if (av[r] > 0.0 && mv[r] == 0ull) cacc += av[r];
            if (av[r] > 0.0 && mv[r] != 0ull) {                  // (nodes behind the segment's end were loaded as zeros)
                const Key2 key{mv[r], abits};
                uint32_t k = 1;
                if (SSN_ABL(8u)) k = (uint32_t)SN_NLEAF + ((uint32_t)(abits >> 30) & (uint32_t)(SN_NLEAF - 1));
                else
#pragma unroll
                for (int l = 0; l < SN_LEVELS; ++l) { const ulonglong2 nd = tree[k]; k = 2u * k + (less2(Key2{nd.x, nd.y}, key) ? 1u : 0u); }
                const uint32_t lo = k - (uint32_t)SN_NLEAF;   // splitters less than the key
                uint32_t eq = 0;
                if (lo < (uint32_t)SN_NSPLIT && !SSN_ABL(8u)) { const ulonglong2 nd = tree[tree_node(lo)]; eq = eq2(Key2{nd.x, nd.y}, key) ? 1u : 0u; }
                id = 2u * lo + eq;
                if (!SSN_ABL(16u)) atomicAdd(&s_hist[id], 1u);
            }
            const bool travels = id != SN_NO_ROW && !(id & 1u) && !SSN_ABL(32u);
            const unsigned long long bal = __ballot(travels);
            if (bal) {                                           // (wave-uniform)
                uint32_t wbase = 0;
                if (lane == 0) wbase = atomicAdd(&s_nstage, (uint32_t)__popcll(bal));
                wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
                if (travels) {
                    const uint32_t pos = stage0 + wbase + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                    sn.stage[pos] = make_ulonglong2(mv[r], abits);
                    sn.ids[pos] = (uint16_t)id;
                }
            }
        }
    }
    __syncthreads();
    uint32_t *row = sn.cntm + ((size_t)s * sn.G + g) * SN_NBUCKET;
    for (int i = threadIdx.x; i < SN_NBUCKET; i += 256) row[i] = s_hist[i];
    if (threadIdx.x == 0) sn.stage_cnt[(size_t)s * sn.G + g] = s_nstage;
    if (sn.c0) {                                                 // (block-uniform) fixed-shape sum: deterministic
        __shared__ double s_c[4];
        cacc = wave_reduce(cacc, [](double x, double y) { return x + y; });
        if (lane == 0) s_c[threadIdx.x >> 6] = cacc;
        __syncthreads();
        if (threadIdx.x == 0) sn.c0p[(size_t)s * sn.G + g] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
    }
    if (HAPS && p0 > 0 && sn.hp.ratio) {                         // (block-uniform) exact integer sums: any order
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k >= p0) break;
            const unsigned long long cs = wave_reduce(c8[k], [](unsigned long long x, unsigned long long y) { return x + y; });
            const unsigned long long ls = wave_reduce(l8[k], [](unsigned long long x, unsigned long long y) { return x + y; });
            if (lane == 0) {
                if (cs) atomicAdd(&s_acc[2 * k], cs);
                if (ls) atomicAdd(&s_acc[2 * k + 1], ls);
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * p0 && s_acc[threadIdx.x]) atomicAdd(&sn.hp.ratio[2 * h0 + threadIdx.x], s_acc[threadIdx.x]);
    }
}

// The same pass for the resident step, FUSED with the node statistics (node_rows_kernel).  It has no abundance array and no covered-base counts to read:
// it takes a node from `bases`, the bit vector, the full-node flags and the haplotype word to {covered bases, a, statistics, mask, column sums, bucket
// id, staged row} in registers, which is node_cov_stats_kernel<false>'s work (stage_node_stats.hip) in front of this pass's own -- the 12 bytes a node that
// kernel wrote and this one read back, and the second read of the lengths, are gone.
// A kernel of its own, not a third instantiation of ssn_hist_kernel: one shared body changed the register allocation of ssn_hist_kernel<true>
// (115 -> 127 VGPRs, node_pass=split 0.6 ms a step slower than the parent at cfg4), and the two-kernel path of the stage calls and fallbacks has to stay
// what it was.  The price: the statements the two share (listed at the head of this file) have to be edited together.
// A wave's item is 64 consecutive nodes: their first bit comes from ONE wave-uniform load of bit_off plus a DPP prefix sum of the lengths (no running
// offset: a workgroup's tiles are not consecutive for a wave).  A tile is walked in two halves of four items -- the statistics kernel's depth: eight
// items' lengths, bases, flag, haplotype and bit-vector words beside the sixteen column sums do not fit the registers of four waves per SIMD (153 VGPRs)
// -- and a half's streams are all requested before its first dependent bit-vector load.  The covered bases of a node have ONE consumer here, the column
// sums of path_cov_ratio: a node without a column (empty mask), or one a step covered whole (flag), does not fetch its bit-vector words at all.
// Instruction issue (round 26: the kernel is bound by VALU / SALU issue and the serial LDS chain of the descent, not by bytes): the tiles that lie
// wholly inside the segment -- all but a segment's last -- take a body without any `i < n` select or exec region, with the streams at a wave-uniform
// base of the half plus the lane's offset; the last tile alone takes the guarded body.  The bucket ids of a half's four items come from ONE level-major
// descent after the streams' registers are free.
constexpr int SN_HALF = SN_ITEMS >= 8 ? SN_ITEMS / 2 : SN_ITEMS;
static_assert(SN_ITEMS % SN_HALF == 0, "whole halves");
// NB (options node_bits / node_bits_words; ssn_node_bits(), ssn_plan.hpp): where a node's bit-vector words come from.
//   0 ("gather"): every node that has a consumer for its count loads its first, last and interior words itself, behind the scan of the lengths -- a
//      second round trip to memory (and one per interior word) that practically every half pays in full: among its 256 nodes one nearly always counts.
//   1, 2 ("range", the default: 2): the words of an item's 64 consecutive nodes are ONE contiguous stretch of the bit vector, from bit_off of the item's
//      first node to bit_off of the node behind its last (the array has V + 1 entries).  Both ends are wave-uniform and DB-static: lane l & 7 of a wave
//      requests end (l & 1) of item (l >> 1) of the COMING half at the top of a half (the first half's: beside the tree copy), and they move to scalar
//      registers where the half's streams have arrived -- two VGPRs.  Lane l then loads word l (and word 64 + l with NB = 2) of each stretch IN FRONT of
//      the four streams (a scheduling barrier keeps the order), so the half's first wait covers them: one level of the dependent chain is gone, and the
//      gathers are one or two coalesced requests per item.  Served from registers: the words' prefix of set bits (DPP scan, no LDS) and the word a node
//      starts in come from the lane that holds them by two shuffles (ds_bpermute; four with NB = 2); the set bits below the node's first bit follow,
//      and a node's covered bases are the NEXT lane's value minus its own (DPP shift; the last lane's neighbour is the stretch's end, wave-uniform) --
//      interior words need no loop.  An item whose stretch is longer than 64 NB words (2 048 / 4 096 bits) takes the gather loads instead
//      (wave-uniform), so any graph stays exact.  Every shuffle runs with all lanes of the wave active, under wave-uniform conditions only.
// Which nodes are counted and the order of every sum are the same for all three: the covered bases are integers.
constexpr int SN_HALVES = SN_ITEMS / SN_HALF;
static_assert(2 * SN_HALF <= 64, "a lane per end of the half's items");
template <int NB>
__global__ void __launch_bounds__(256) node_rows_kernel(Sn sn) {
    __shared__ ulonglong2 tree[SN_NLEAF];
    __shared__ uint32_t s_hist[SN_NBUCKET];
    extern __shared__ unsigned long long s_dyn_tab[];             // [nbyte][256] columns of the haplotypes 8b .. 8b+7 set in a byte value
    __shared__ int s_bit[64];
    __shared__ unsigned long long s_acc[2 * 64];
    const uint32_t s = blockIdx.y, g = blockIdx.x, o = sn.node_base[s], n = sn.node_base[s + 1] - o;
    uint32_t *w = sn.w(s);
    if (n == 0 || w[SN_OFF_FLAGS] != 0) return;                  // (a small segment: rows, column sums and statistics are the sample kernel's)
    uint32_t t0, t1;
    sn_tiles(sn, n, g, t0, t1);
    // a species without LP columns (the species level dropped it, or no haplotype passed the first filter) has no rows: an empty histogram, nothing staged
    if (sn.skip_empty && sn.hp.sp_p[s] <= 0) {                   // (workgroup-uniform)
        uint32_t *row0 = sn.cntm + ((size_t)s * sn.G + g) * SN_NBUCKET;
        for (int i = threadIdx.x; i < SN_NBUCKET; i += 256) row0[i] = 0u;
        if (threadIdx.x == 0) { sn.stage_cnt[(size_t)s * sn.G + g] = 0u; if (sn.c0) sn.c0p[(size_t)s * sn.G + g] = 0.0; }
        // a species that is PRESENT but has no column still reports its statistics (the single-path frequencies_mean, strain_finish) -- from lengths
        // and bases alone; one the species level dropped has zeros (node_rows_final_kernel), as node_cov_stats_kernel writes them without reading
        if (!sn.fz.active || sn.fz.active[s]) {
            NodeAcc acc;
            for (uint32_t t = t0; t < t1; ++t)
#pragma unroll
                for (int r = 0; r < SN_ITEMS; ++r) {
                    const uint32_t i = t * SN_TILE + (uint32_t)r * 256u + threadIdx.x;
                    if (i < n) acc.add((double)(long long)sn.fz.bases[o + i] / (double)sn.hp.node_len[o + i], sn.fz.min_depth);
                }
            sn_block_partial<4>(acc, sn.npart + (size_t)s * sn.G + g);
        }
        return;
    }
    const ulonglong2 *gt = reinterpret_cast<const ulonglong2 *>(w + SN_OFF_TREE);
    __shared__ uint32_t s_nstage;
    const int lane = threadIdx.x & 63;
    const uint32_t wave64 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) << 6;
    constexpr int HALF = SN_HALF;                                // items in flight together
    // NB: this lane's end of the items of half q of the segment (a half is HALF * 256 consecutive nodes; behind the segment's end: the end itself, an empty stretch)
    auto end_of = [&](uint32_t q) -> uint64_t {
        const uint32_t i = q * (uint32_t)(HALF * 256) + (uint32_t)((lane >> 1) % HALF) * 256u + wave64 + (uint32_t)(lane & 1) * 64u;
        return sn.fz.bit_off[o + (i < n ? i : n)];
    };
    uint64_t endv = 0;
    if (NB && t0 < t1) endv = end_of(t0 * (uint32_t)SN_HALVES);
    for (int i = threadIdx.x; i < SN_NBUCKET; i += 256) s_hist[i] = 0;
    if (threadIdx.x == 0) s_nstage = 0;
    if (t0 < t1) for (int i = threadIdx.x; i < SN_NLEAF; i += 256) tree[i] = gt[i];
    const uint64_t h0 = sn.hp.hap_off[s], nh = sn.hp.hap_off[s + 1] - h0;
    int p0 = sn.hp.sp_p[s];
    if (p0 <= 0 || p0 > 64 || nh > 64) p0 = 0;                    // no columns
    const int nbyte = p0 ? (int)((nh + 7) / 8) : 0;
    if (threadIdx.x < 64) s_bit[threadIdx.x] = (p0 && threadIdx.x < nh) ? sn.hp.hap_bit[h0 + threadIdx.x] : -1;
    if (threadIdx.x < 128) s_acc[threadIdx.x] = 0;
    __syncthreads();
    for (int b = 0; b < nbyte; ++b) {
        unsigned long long e = 0ull;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const int bit = s_bit[8 * b + i]; if (((threadIdx.x >> i) & 1u) && bit >= 0) e |= 1ull << bit; }
        s_dyn_tab[b * 256 + threadIdx.x] = e;
    }
    __syncthreads();
    uint64_t eb[2 * HALF];                                       // NB: the ends of the coming half's items (wave-uniform: scalar registers)
#pragma unroll
    for (int k = 0; k < 2 * HALF; ++k) eb[k] = NB ? lane_get(endv, k) : 0ull;
    unsigned long long c8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, l8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t stage0 = o + t0 * SN_TILE;                    // (the staged rows: see ssn_hist_kernel)
    double cacc = 0.0;                                           // abundances of this thread's nodes with an empty mask
    NodeAcc nacc;                                                // statistics of this thread's nodes
    // One half of tile t (items hb .. hb + HALF - 1).  GUARD = false: the tile lies wholly inside the segment (workgroup-uniform) -- no lane is behind the
    // segment's end, the streams are loaded from a wave-uniform 64-bit base of the half plus the lane's 32-bit offset inside it, nothing is selected.
    // GUARD = true, a segment's last tile: a lane behind the end loads the segment's last node and takes zeros afterwards.
    static_assert((uint64_t)SN_TILE * sizeof(unsigned long long) < (1ull << 20), "a lane's byte offset from the half's base: 32 bits with room to spare");
    auto half = [&](auto guard, const uint32_t t, const int hb) __attribute__((always_inline)) {
        constexpr bool GUARD = decltype(guard)::value;
        __builtin_amdgcn_sched_barrier(0);                       // (a half's requests stay behind the half before it: the registers are one half's)
        const uint32_t hbase = t * SN_TILE + (uint32_t)hb * 256u, base = hbase + threadIdx.x;   // (hbase < n: the half's first node in the segment, unless GUARD)
        double av[HALF];
        uint64_t mv[HALF];
        uint32_t cv[HALF], lv[HALF];
        {
            unsigned long long bs[HALF];
            uint32_t fw[HALF];
            uint64_t gb[HALF];                                   // first bit of the wave's 64 nodes (wave-uniform)
            uint32_t bw0[HALF], bw1[HALF];                       // NB, an item that fits: words lane and 64 + lane of its stretch; otherwise a node's first and last word
            bool fits[HALF];                                     // NB: the stretch was loaded (wave-uniform)
            uint32_t nwv[HALF], tbv[HALF];                       // NB: words and bits of the item's stretch (wave-uniform)
            if (NB) {                                            // the items' stretches of the bit vector: requested in front of the streams, so the first wait covers them
#pragma unroll
                for (int r = 0; r < HALF; ++r) {
                    const uint64_t b0 = eb[2 * r], b1 = eb[2 * r + 1], w0 = b0 >> 5;
                    const uint32_t nw = b1 > b0 ? (uint32_t)(((b1 - 1) >> 5) - w0) + 1u : 0u, cap = 64u * (uint32_t)NB;
                    gb[r] = b0;
                    nwv[r] = nw;
                    tbv[r] = (uint32_t)(b1 - b0);
                    fits[r] = nw <= cap && !NRK_ABL(1u);
                    // no branch: a lane behind the stretch's last word (or behind the capacity) loads that word again; an empty stretch (behind the segment's end) word 0
                    const uint32_t top = nw ? (nw < cap ? nw : cap) - 1u : 0u;
                    const uint32_t *wp = sn.fz.bitmap + (nw ? w0 : 0ull);
                    bw0[r] = wp[(uint32_t)lane < top ? (uint32_t)lane : top];
                    bw1[r] = NB > 1 ? wp[(uint32_t)lane + 64u < top ? (uint32_t)lane + 64u : top] : 0u;
                }
                endv = end_of(t * (uint32_t)SN_HALVES + (uint32_t)(hb / HALF) + 1u);   // the coming half's ends: a whole half ahead of their use
                __builtin_amdgcn_sched_barrier(0);               // (these requests stay in front of the streams)
            }
#pragma unroll
            for (int r = 0; r < HALF; ++r) {                     // the four streams of the half
                if constexpr (GUARD) {                           // (n > 0: a lane behind the end loads node n - 1)
                    const uint32_t i = base + (uint32_t)r * 256u;
                    const bool in = i < n;
                    const uint32_t v = o + (in ? i : n - 1u);
                    const uint32_t l = sn.hp.node_len[v], f = sn.fz.full[v >> 5];
                    const unsigned long long b = sn.fz.bases[v], h = sn.hp.node_haps[v];
                    lv[r] = in ? l : 0u; bs[r] = in ? b : 0ull; fw[r] = in ? f : 0u; mv[r] = in ? h : 0ull;
                } else {                                         // node v0 + j: the 64-bit part of the address is the half's (scalar), j < SN_TILE
                    const uint32_t v0 = o + hbase, j = threadIdx.x + (uint32_t)r * 256u;
                    lv[r] = (sn.hp.node_len + v0)[j];
                    bs[r] = (sn.fz.bases + v0)[j];
                    fw[r] = (sn.fz.full + (v0 >> 5))[((v0 & 31u) + j) >> 5];
                    mv[r] = (sn.hp.node_haps + v0)[j];
                }
            }
            if (!NB) {
#pragma unroll
                for (int r = 0; r < HALF; ++r) {                 // first bit of the wave's 64 nodes (wave-uniform)
                    const uint32_t i0 = t * SN_TILE + (uint32_t)(hb + r) * 256u + wave64;
                    gb[r] = i0 < n ? sn.fz.bit_off[o + i0] : 0ull;
                    fits[r] = false; nwv[r] = tbv[r] = 0u;
                }
            }
            if (NB) {                                            // (the streams have arrived, and the ends requested before them)
#pragma unroll
                for (int k = 0; k < 2 * HALF; ++k) eb[k] = lane_get(endv, k);
            }
            bool whole[HALF];
#pragma unroll
            for (int r = 0; r < HALF; ++r) {                     // haplotype word -> columns
                const unsigned long long hm = mv[r];
                unsigned long long m = 0ull;
#pragma unroll 4
                for (int b = 0; b < nbyte; ++b) m |= s_dyn_tab[b * 256 + (int)((hm >> (8 * b)) & 255ull)];   // (four lookups in flight: eight were the kernel's register peak)
                mv[r] = m;
                whole[r] = (fw[r] >> ((o + base + (uint32_t)r * 256u) & 31u)) & 1u;   // a step covered the whole node: a flag instead of marked bits
            }
#pragma unroll
            for (int r = 0; r < HALF; ++r) {                     // gather: first and last bit-vector word of every node that has a consumer for its count: independent loads, issued together
                if (NB && fits[r]) continue;                     // (wave-uniform)
                const bool count = lv[r] != 0u && mv[r] != 0ull && !whole[r] && !NRK_ABL(1u);   // (l = 0 behind the segment's end)
                const uint64_t g0 = gb[r] + (wave_incl_scan_dpp(lv[r]) - lv[r]);
                bw0[r] = count ? sn.fz.bitmap[g0 >> 5] : 0u;
                bw1[r] = count ? sn.fz.bitmap[(g0 + lv[r] - 1) >> 5] : 0u;
            }
#pragma unroll
            for (int r = 0; r < HALF; ++r) {
                const uint32_t i = base + (uint32_t)r * 256u;
                const bool count = lv[r] != 0u && mv[r] != 0ull && !whole[r] && !NRK_ABL(1u);
                // the node's first bit from the item's (a species' bases fit 32 bits: checked at upload).  Formed where it is used: four items' worth held from the
                // streams' arrival on cost four registers at the kernel's peak.  Every lane of the wave is active HERE, at the top of an item: the per-lane arms
                // further down (`else if (count)` with its interior-word loop, `i < n`) have closed again before the next item begins -- no scan or shuffle may move
                // into them.  An item that takes the gather fallback forms this scan twice (once for its loads above): six VALU on the rare path
                const uint32_t exr = wave_incl_scan_dpp(lv[r]) - lv[r];
                uint32_t c = whole[r] ? lv[r] : 0u;
                if (NB && fits[r]) {                             // (wave-uniform: every lane takes part in the shuffles)
                    // E = the set bits of the stretch below the node's first bit, from the words' prefix of set bits (DPP scan) and the word the bit lies in, both
                    // fetched from the lane that holds them.  The nodes of a wave follow each other in the bit vector, so a node's covered bases are the NEXT
                    // lane's E minus its own, and the last lane's neighbour is the stretch's end (wave-uniform): no loop over interior words, no last word
                    const uint32_t nw = nwv[r], last = nw ? nw - 1u : 0u;
                    const uint32_t q0 = (uint32_t)lane < nw ? __popc(bw0[r]) : 0u, s0 = wave_incl_scan_dpp(q0);
                    uint32_t q1 = 0u, s1 = 0u;
                    if (NB > 1) { q1 = (uint32_t)lane + 64u < nw ? __popc(bw1[r]) : 0u; s1 = wave_incl_scan_dpp(q1) + lane_get(s0, 63); }
                    const uint32_t f0 = ((uint32_t)gb[r] & 31u) + exr, j0 = f0 >> 5;   // bits from the stretch's first word on
                    uint32_t x = (uint32_t)__shfl((int)bw0[r], (int)(j0 & 63u)), px = (uint32_t)__shfl((int)(s0 - q0), (int)(j0 & 63u));
                    if (NB > 1) {
                        const uint32_t y = (uint32_t)__shfl((int)bw1[r], (int)(j0 & 63u)), py = (uint32_t)__shfl((int)(s1 - q1), (int)(j0 & 63u));
                        if (j0 & 64u) { x = y; px = py; }
                    }
                    // the end: the prefix of the last word less its bits behind the stretch's last bit (they are the next item's)
                    const uint32_t fe = ((uint32_t)gb[r] & 31u) + tbv[r];
                    uint32_t wl = lane_get(bw0[r], (int)(last & 63u)), sl = lane_get(s0, (int)(last & 63u));
                    if (NB > 1 && last >= 64u) { wl = lane_get(bw1[r], (int)(last & 63u)); sl = lane_get(s1, (int)(last & 63u)); }
                    const uint32_t ce = sl - (uint32_t)__popc(wl & ~(0xFFFFFFFFu >> (31u - ((fe - 1u) & 31u))));
                    const uint32_t e = j0 >= nw ? ce : px + (uint32_t)__popc(x & ((1u << (f0 & 31u)) - 1u));   // (a lane behind the segment's end, or a node that starts where the stretch ends)
                    const uint32_t cc = wave_shl1(e, ce) - e;
                    if (count) c = cc;
                } else if (count) {
                    const uint64_t g0 = gb[r] + exr, g1 = g0 + lv[r], w0 = g0 >> 5, w1 = (g1 - 1) >> 5;
                    const uint32_t m0 = 0xFFFFFFFFu << (g0 & 31), m1 = 0xFFFFFFFFu >> (31 - (uint32_t)((g1 - 1) & 31));
                    c = w0 == w1 ? __popc(bw0[r] & m0 & m1) : __popc(bw0[r] & m0) + __popc(bw1[r] & m1);
                    for (uint64_t ww = w0 + 1; ww < w1; ++ww) c += __popc(sn.fz.bitmap[ww]);   // nodes of more than 33 bases
                }
                cv[r] = c;
                av[r] = 0.0;
                if (!GUARD || i < n) {
                    av[r] = (double)(long long)bs[r] / (double)lv[r];   // profile.rs:987-988, as node_cov_stats_kernel forms it
                    nacc.add(av[r], sn.fz.min_depth);
                }
                if constexpr (!GUARD) __builtin_amdgcn_sched_barrier(0);   // (one item's shuffles at a time: four items' temporaries do not fit beside the sums)
            }
        }
        [[maybe_unused]] uint32_t idv[HALF];
#ifndef NODE_ROWS_SERIAL_DESCENT
        {                                                        // the bucket ids of the half's items, level by level (sn_bucket_ids): the streams' registers are free here
            uint64_t ka[HALF];
#pragma unroll
            for (int r = 0; r < HALF; ++r) ka[r] = (uint64_t)__double_as_longlong(av[r]);
            if (NRK_ABL(2u)) {
#pragma unroll
                for (int r = 0; r < HALF; ++r) idv[r] = 2u * ((uint32_t)(ka[r] >> 30) & (uint32_t)(SN_NLEAF - 1));
            } else sn_bucket_ids<HALF>(tree, mv, ka, idv);
        }
#endif
        // ---- from here on the statements this kernel shares with ssn_hist_kernel<true> (edit both): the list at the head of this file says which.  The bucket id
        // is not among them: it is idv[r] from above, or -- -DNODE_ROWS_SERIAL_DESCENT, A/B builds only -- ssn_hist_kernel's descent per row
#pragma unroll
        for (int r = 0; r < HALF; ++r) {
            {                                                     // the columns' sums
                const unsigned long long m = mv[r];
                if (m) {
                    const unsigned long long c = cv[r], l = lv[r];
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < p0) { const bool on = (m >> k) & 1ull; c8[k] += on ? c : 0ull; l8[k] += on ? l : 0ull; }   // (block-uniform: the columns that exist)
                    unsigned long long rest = m >> 8;
                    while (rest) {
                        const int k = __ffsll((long long)rest) - 1 + 8;
                        rest &= rest - 1;
                        if (c) atomicAdd(&s_acc[2 * k], c);
                        atomicAdd(&s_acc[2 * k + 1], l);
                    }
                }
            }
            uint32_t id = SN_NO_ROW;
            const uint64_t abits = (uint64_t)__double_as_longlong(av[r]);
            if (av[r] > 0.0 && mv[r] == 0ull) cacc += av[r];
            if (av[r] > 0.0 && mv[r] != 0ull) {                  // (nodes behind the segment's end were loaded as zeros)
#ifdef NODE_ROWS_SERIAL_DESCENT
                const Key2 key{mv[r], abits};
                uint32_t k = 1;
                if (NRK_ABL(2u)) k = (uint32_t)SN_NLEAF + ((uint32_t)(abits >> 30) & (uint32_t)(SN_NLEAF - 1));
                else
#pragma unroll
                for (int l = 0; l < SN_LEVELS; ++l) { const ulonglong2 nd = tree[k]; k = 2u * k + (less2(Key2{nd.x, nd.y}, key) ? 1u : 0u); }
                const uint32_t lo = k - (uint32_t)SN_NLEAF;   // splitters less than the key
                uint32_t eq = 0;
                if (lo < (uint32_t)SN_NSPLIT && !NRK_ABL(2u)) { const ulonglong2 nd = tree[tree_node(lo)]; eq = eq2(Key2{nd.x, nd.y}, key) ? 1u : 0u; }
                id = 2u * lo + eq;
#else
                id = idv[r];
#endif
                atomicAdd(&s_hist[id], 1u);
            }
            const bool travels = id != SN_NO_ROW && !(id & 1u);
            const unsigned long long bal = __ballot(travels);
            if (bal) {                                           // (wave-uniform)
                uint32_t wbase = 0;
                if (lane == 0) wbase = atomicAdd(&s_nstage, (uint32_t)__popcll(bal));
                wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
                if (travels) {
                    const uint32_t pos = stage0 + wbase + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                    sn.stage[pos] = make_ulonglong2(mv[r], abits);
                    sn.ids[pos] = (uint16_t)id;
                }
            }
        }
    };
    const uint32_t tf = n / SN_TILE < t1 ? n / SN_TILE : t1;     // (workgroup-uniform) the tiles before tf lie wholly inside the segment; only a segment's last tile may not
    for (uint32_t t = t0; t < tf; ++t) {
#pragma unroll
        for (int hb = 0; hb < SN_ITEMS; hb += HALF) half(std::false_type{}, t, hb);
    }
    if (t0 < t1 && tf < t1) {                                    // the segment's last tile (tf = t1 - 1 >= t0: t1 is at most the segment's tiles, n / SN_TILE one less at least)
#pragma unroll
        for (int hb = 0; hb < SN_ITEMS; hb += HALF) half(std::true_type{}, tf, hb);
    }
    __syncthreads();
    sn_block_partial<4>(nacc, sn.npart + (size_t)s * sn.G + g);
    uint32_t *row = sn.cntm + ((size_t)s * sn.G + g) * SN_NBUCKET;
    for (int i = threadIdx.x; i < SN_NBUCKET; i += 256) row[i] = s_hist[i];
    if (threadIdx.x == 0) sn.stage_cnt[(size_t)s * sn.G + g] = s_nstage;
    if (sn.c0) {                                                 // (block-uniform) fixed-shape sum: deterministic
        __shared__ double s_c[4];
        cacc = wave_reduce(cacc, [](double x, double y) { return x + y; });
        if (lane == 0) s_c[threadIdx.x >> 6] = cacc;
        __syncthreads();
        if (threadIdx.x == 0) sn.c0p[(size_t)s * sn.G + g] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
    }
    if (p0 > 0 && sn.hp.ratio) {                                 // (block-uniform) exact integer sums: any order
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k >= p0) break;
            const unsigned long long cs = wave_reduce(c8[k], [](unsigned long long x, unsigned long long y) { return x + y; });
            const unsigned long long ls = wave_reduce(l8[k], [](unsigned long long x, unsigned long long y) { return x + y; });
            if (lane == 0) {
                if (cs) atomicAdd(&s_acc[2 * k], cs);
                if (ls) atomicAdd(&s_acc[2 * k + 1], ls);
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * p0 && s_acc[threadIdx.x]) atomicAdd(&sn.hp.ratio[2 * h0 + threadIdx.x], s_acc[threadIdx.x]);
    }
}

// fused: a species' statistics from the partials of its partition workgroups, in workgroup order (one wave per species: lane l combines workgroups
// l, l + 64, ..., then a fixed-shape wave reduction -- node_stats_final_kernel's shape over the (species, workgroup) layout)
__global__ void __launch_bounds__(64) node_rows_final_kernel(Sn sn) {
    const uint32_t s = blockIdx.x, n = sn.node_base[s + 1] - sn.node_base[s];
    double mx = -INFINITY, zs = 0.0; unsigned long long nv = 0, zc = 0;
    if (n != 0 && sn.fz.active && !sn.fz.active[s]) mx = 0.0;    // dropped by the species level: the zeros node_cov_stats_kernel writes without reading
    else if (n != 0) {
        const uint32_t nt = (n + SN_TILE - 1) / SN_TILE, ng = n <= (uint32_t)SN_SAMPLE ? 1u : (nt + sn.per - 1) / sn.per;   // (a small segment: the sample kernel's)
        for (uint32_t g = threadIdx.x; g < ng; g += 64) { const NodePartial p = sn.npart[(size_t)s * sn.G + g]; mx = fmax(mx, p.mx); zs += p.zs; nv += p.nv; zc += p.zc; }
    }
    mx = wave_reduce(mx, [](double x, double y) { return fmax(x, y); });
    zs = wave_reduce(zs, [](double x, double y) { return x + y; });
    nv = wave_reduce(nv, [](unsigned long long x, unsigned long long y) { return x + y; });
    zc = wave_reduce(zc, [](unsigned long long x, unsigned long long y) { return x + y; });
    if (threadIdx.x == 0) { sn.fz.amax[s] = mx; sn.fz.nvalid[s] = (uint32_t)nv; sn.fz.nzsum[s] = zs; sn.fz.nzcnt[s] = (uint32_t)zc; }
}
}  // namespace

void ssn_node_rows_launch(Ctx *ctx, const Sn &sn, uint32_t S, uint32_t max_haps, int node_bits) {
    const size_t lds = (size_t)((max_haps + 7) / 8) * 256 * sizeof(unsigned long long);
    if (node_bits == 0) hipLaunchKernelGGL(node_rows_kernel<0>, dim3(sn.G, S), dim3(256), lds, ctx->stream, sn);
    else if (node_bits == 1) hipLaunchKernelGGL(node_rows_kernel<1>, dim3(sn.G, S), dim3(256), lds, ctx->stream, sn);
    else hipLaunchKernelGGL(node_rows_kernel<2>, dim3(sn.G, S), dim3(256), lds, ctx->stream, sn);
    hipLaunchKernelGGL(node_rows_final_kernel, dim3(S), dim3(64), 0, ctx->stream, sn);
}

void ssn_hist_launch(Ctx *ctx, const Sn &sn, uint32_t S, bool haps, uint32_t max_haps) {
    if (haps) hipLaunchKernelGGL(ssn_hist_kernel<true>, dim3(sn.G, S), dim3(256), (size_t)((max_haps + 7) / 8) * 256 * sizeof(unsigned long long), ctx->stream, sn);
    else hipLaunchKernelGGL(ssn_hist_kernel<false>, dim3(sn.G, S), dim3(256), 0, ctx->stream, sn);
}

}  // namespace ptx
