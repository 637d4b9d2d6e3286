// stage_hap_pairs.hip -- pairwise strain distinguishability of a db (pantax_hip_db_hap_pairs, the --db-pairs mode): for every two selected haplotypes of a
// species the nodes both walk, as { n_nodes, len }.  Not a stage of the reference; it reads no sample.
//
// Contract (include/pantax_hip.h, DESIGN.md "Pairwise strain distinguishability"): Sel_s, K_s, M(v), m(v) of pantax_hip_strain_evidence; Q(v) = (1, node_len[v])
// as u64; pair[a][b] = sum of Q over the nodes v with the haplotypes at positions a and b of the species' list both in M(v); per species total (every node),
// none (m = 0), core (m = K_s, K_s >= 1).  That is C = B^T diag(Q) B over the 0/1 membership rows B.  Integers only: no order matters.
//
// Membership: the two routes of member_plan.hpp over the selected haplotypes (option hap_pairs_route), nw = ceil(K_s / 64) words per node on route 2.
// The unit of work is a BLOCK PAIR (wa, wb), wa <= wb, of mask words (hap_pairs_plan.hpp): a species has nw (nw + 1) / 2 of them, one on route 1.  The host
// cuts every species' nodes into chunks, once per block pair; a chunk goes to a WAVE (four in flight per workgroup, no workgroup barrier anywhere).
// hap_pairs_kernel<KB>: the wave takes its chunk 64 nodes at a time, lane l loading word wa, word wb and the length of node l (one contiguous stretch per
// load instruction, the next 64 nodes' loads issued ahead of the work on these), and walks the 64 nodes with readlane, so that a node's two words and its
// length are wave-uniform.  Lane i owns ROW bit i of word wa and keeps one counter per COLUMN bit j < KB of word wb in registers, { n_nodes << 48 | len }
// in one u64: for a node whose word wa holds bit i the lane adds the node into the counters of the set bits of wb (an AND with a scalar 0 / ~0 per
// column, fully unrolled, no branch).  KB = 8, 16, 32, 64 is the smallest that covers the live column bits (hap_pairs_cols): the kernel is compiled per KB, the host sorts the chunks
// by it, and a species of six haplotypes pays for eight columns, not for 64.
//   core nodes   a node whose two words hold ALL live bits is summed by the lane that loaded it into one counter of its own, 64 nodes at a time, and never
//                walked; the flush adds the wave's sum to every live (row, column).  They are the bulk -- the same bits node after node.  A node with an
//                empty word is dropped the same way; the wave walks the rest, found by one ballot.
//   flush        once per chunk: lane i, for every live column j, one 64-bit atomicAdd per non-zero half of its counter into pair[a(i)][b(j)].
//                The chunk is sized so that these are few beside the loads (hap_pairs_chunk); the lower triangle of a species of several words is
//                mirrored on the host (hap_pairs_mirror).
//   species sums in the chunks of block pair (0, 0) alone, so that a node is counted once: lane l looks at ALL nw words of its node for m(v), sums in lane
//                registers, one DPP wave reduction per sum at the end of the chunk.  A species with nothing selected has one such tile and no block pair.
// No floating point, no inline assembly, vector stores and vector atomics only.
//
// The coverage form (pantax_hip_strain_pair_evidence, the --strain-pair-evidence report; DESIGN.md "Pairwise strain evidence"): Q(v) = (1, node_len[v],
// node_base_cov[v], bases_per_node[v]), the evidence call's, summed over the same block pairs into pair [..][4] and species [S][3][4].  pair_evidence_kernel<KB>
// walks a chunk once per PLANE with the same KB counters: plane 0 { n_nodes << 48 | len } as above, plane 1 covered (<= len a node, so a chunk's sum
// stays under 2^47), plane 2 bases (a free u64: its counter is a whole u64 and wraps as the evidence call's sum does).  Three u64 a column in one pass do
// not fit the register file at KB = 64 (the db-only kernel is at 153 VGPRs); a plane costs one more walk of tiles that are L2-hot by then and no register
// beyond the tile's quantity widening to 64 bits.  The species sums take all four quantities in tile 0, as the evidence kernel's lanes do.
//
// Algorithmic bytes (V nodes), route 1: (4 + 8) V in for the pairs, the species sums from the same loads; out 16 K_s^2 + 48 per species.
// Route 2, a species of V_s nodes and nw words: nw (nw + 1) / 2 passes of 4 + 8 (diagonal) or 4 + 16 bytes per node, + 8 nw V_s once for m(v),
// behind the mask pass (walk_masks.hip).
#include <algorithm>
#include "common.hpp"
#include "hap_pairs_plan.hpp"
#include "member_device.hpp"
#include "primitives.hpp"

namespace ptx {

namespace {

constexpr unsigned long long HP_ONE = 1ull << 48;              // a node in a packed counter: n_nodes above bit 48, len below
constexpr unsigned long long HP_LEN = HP_ONE - 1ull;
static_assert((uint64_t)HAP_PAIRS_CHUNK_MAX <= 0xFFFFull && (uint64_t)HAP_PAIRS_CHUNK_MAX * 0xFFFFFFFFull < HP_ONE, "a chunk's sums fit the packed counter");
// the planes of the coverage form: what a node adds to a counter.  covered is a u32 a node (<= len): a chunk's sum fits 48 bits as len's does, though its
// counter is a plain u64; bases has the whole u64 and wraps as every u64 sum of it does
constexpr int HP_PLANES = 3;
static_assert((uint64_t)HAP_PAIRS_CHUNK_MAX * 0xFFFFFFFFull < (1ull << 48), "a chunk's covered bases fit the 48-bit field of a counter");

struct HpSpecies { MemberRow m; uint32_t bit_base, pad; unsigned long long pair_base; };   // bit_base: first entry of the species in bit_pos; pair_base: pair_off[s]

struct HpTile { unsigned long long a, b; uint32_t len; };      // lane l: the two words and the length of node t0 + l (zeros beyond the chunk)
struct HpTileQ { unsigned long long a, b, q; };                // the coverage form: the plane's quantity of the node, as it goes into a counter

__device__ __forceinline__ HpTile hp_load(const MemberChunk ch, const MemberRow m, uint32_t wa, uint32_t wb, uint32_t t0, int lane, const uint32_t *__restrict__ node_len,
                                          const unsigned long long *__restrict__ node_haps, const unsigned long long *__restrict__ mask) {
    const uint32_t i = t0 + (uint32_t)lane;
    const bool on = i < ch.n;
    const uint32_t v = ch.first + (on ? i : 0u);   // (a dead lane reads the chunk's first node and drops it)
    HpTile t;
    t.len = on ? node_len[v] : 0u;
    if (m.route == 1u) { t.a = node_haps[v] & m.bits; t.b = t.a; }
    else {
        const uint64_t row = member_mask_row(m, v);
        t.a = mask[row + wa];
        t.b = wb == wa ? t.a : mask[row + wb];
    }
    if (!on) { t.a = 0ull; t.b = 0ull; }
    return t;
}
// the coverage form's tile: the same two words, and the quantity of `plane` (wave-uniform) in place of the length
__device__ __forceinline__ HpTileQ hp_load_q(const MemberChunk ch, const MemberRow m, uint32_t wa, uint32_t wb, uint32_t t0, int lane, int plane, const uint32_t *__restrict__ node_len,
                                             const uint32_t *__restrict__ cov, const unsigned long long *__restrict__ bases, const unsigned long long *__restrict__ node_haps,
                                             const unsigned long long *__restrict__ mask) {
    const uint32_t i = t0 + (uint32_t)lane;
    const bool on = i < ch.n;
    const uint32_t v = ch.first + (on ? i : 0u);
    HpTileQ t;
    if (plane == 0) t.q = HP_ONE | (unsigned long long)node_len[v];
    else if (plane == 1) t.q = (unsigned long long)cov[v];
    else t.q = bases[v];
    if (m.route == 1u) { t.a = node_haps[v] & m.bits; t.b = t.a; }
    else {
        const uint64_t row = member_mask_row(m, v);
        t.a = mask[row + wa];
        t.b = wb == wa ? t.a : mask[row + wb];
    }
    if (!on) { t.a = 0ull; t.b = 0ull; t.q = 0ull; }
    return t;
}

template <int KB>
__global__ void __launch_bounds__(256) hap_pairs_kernel(uint32_t c_begin, uint32_t c_end, const MemberChunk *__restrict__ chunks, const HpSpecies *__restrict__ tab,
                                                        const uint32_t *__restrict__ node_len, const unsigned long long *__restrict__ node_haps,
                                                        const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ bit_pos,
                                                        unsigned long long *__restrict__ pair_out /*[..][2]*/, unsigned long long *__restrict__ sp_out /*[S][3][2]*/) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (uniform to the compiler too: the chunk and its species come in scalar registers)
    for (uint32_t c = c_begin + blockIdx.x * 4u + wave; c < c_end; c += gridDim.x * 4u) {
        const MemberChunk ch = chunks[c];
        const HpSpecies st = tab[ch.species];
        const MemberRow m = st.m;
        // ---- the species sums: block pair (0, 0) alone, every word of the node
        if (ch.tile == 0u) {
            unsigned long long tot = 0ull, non = 0ull, cor = 0ull;
            for (uint32_t t0 = 0; t0 < ch.n; t0 += 64u) {
                const uint32_t i = t0 + (uint32_t)lane;
                if (i < ch.n) {
                    const uint32_t v = ch.first + i;
                    uint32_t cnt = 0u;
                    if (m.route == 1u) cnt = (uint32_t)__popcll(node_haps[v] & m.bits);
                    else if (m.route == 2u) {
                        const uint64_t row = member_mask_row(m, v);
                        for (uint32_t w = 0; w < m.nw; ++w) cnt += (uint32_t)__popcll(mask[row + w]);
                    }
                    const unsigned long long q = HP_ONE | (unsigned long long)node_len[v];
                    tot += q;
                    non += cnt == 0u ? q : 0ull;
                    cor += (m.K != 0u && cnt == m.K) ? q : 0ull;
                }
            }
            const auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
            tot = wave_reduce(tot, add); non = wave_reduce(non, add); cor = wave_reduce(cor, add);
            if (lane < 3) {   // lane 0 total, 1 none, 2 core
                const unsigned long long x = lane == 0 ? tot : lane == 1 ? non : cor;
                unsigned long long *const o = sp_out + (uint64_t)ch.species * 6u + (uint32_t)lane * 2u;
                if (x >> 48) atomicAdd(o, x >> 48);
                if (x & HP_LEN) atomicAdd(o + 1, x & HP_LEN);
            }
        }
        if (m.route == 0u) continue;   // nothing selected: no block pair
        // ---- the block pair
        const HapPairsTile bp = hap_pairs_tile(m.nw, ch.tile);
        const unsigned long long live_a = m.route == 1u ? m.bits : hap_pairs_live(m.K, bp.wa);
        const unsigned long long live_b = m.route == 1u ? m.bits : hap_pairs_live(m.K, bp.wb);
        unsigned long long acc[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) acc[j] = 0ull;
        unsigned long long core = 0ull;   // per lane: its nodes that hold every live bit of both words
        HpTile cur = hp_load(ch, m, bp.wa, bp.wb, 0u, lane, node_len, node_haps, mask);
        for (uint32_t t0 = 0; t0 < ch.n; t0 += 64u) {
            HpTile nxt{0ull, 0ull, 0u};
            if (t0 + 64u < ch.n) nxt = hp_load(ch, m, bp.wa, bp.wb, t0 + 64u, lane, node_len, node_haps, mask);
            const bool some = cur.a != 0ull && cur.b != 0ull, full = some && cur.a == live_a && cur.b == live_b;
            core += full ? (HP_ONE | (unsigned long long)cur.len) : 0ull;
            // the nodes that go through the counters, one after the other.  The body holds no branch: the counters are updated where they are
            // (under a wave-uniform `if` per node or per column the compiler keeps a second set of them and copies it back)
            for (unsigned long long todo = __builtin_amdgcn_ballot_w64(some && !full); todo; todo &= todo - 1ull) {
                const int l = __builtin_ctzll(todo);
                const unsigned long long a = lane_get(cur.a, l), b = lane_get(cur.b, l);
                const unsigned long long q = HP_ONE | (unsigned long long)lane_get(cur.len, l);
                const unsigned long long mine = ((a >> lane) & 1ull) ? q : 0ull;
#pragma unroll
                for (int j = 0; j < KB; ++j) acc[j] += mine & (0ull - ((b >> j) & 1ull));   // an AND with a scalar 0 / ~0 per column
            }
            cur = nxt;
        }
        core = wave_reduce(core, [](unsigned long long x, unsigned long long y) { return x + y; });
        // ---- flush: lane i owns row bit i; the positions of the row and column haplotypes in the species' list
        const bool row_on = (live_a >> lane) & 1ull;
        const uint32_t pos_a = row_on ? bit_pos[st.bit_base + 64u * bp.wa + (uint32_t)lane] : MEMBER_NO_ENTRY;
        const uint32_t pos_b_mine = ((live_b >> lane) & 1ull) ? bit_pos[st.bit_base + 64u * bp.wb + (uint32_t)lane] : MEMBER_NO_ENTRY;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            if (!((live_b >> j) & 1ull)) continue;
            const uint32_t pos_b = lane_get(pos_b_mine, j);
            const unsigned long long x = acc[j] + core;
            if (row_on && pos_a != MEMBER_NO_ENTRY && pos_b != MEMBER_NO_ENTRY) {
                unsigned long long *const o = pair_out + (st.pair_base + (uint64_t)pos_a * m.K + pos_b) * 2u;
                if (x >> 48) atomicAdd(o, x >> 48);
                if (x & HP_LEN) atomicAdd(o + 1, x & HP_LEN);
            }
        }
    }
}

// The coverage form, a sibling of the kernel above with its block pair, its walk and its flush: four columns, the chunk walked once per plane
template <int KB>
__global__ void __launch_bounds__(256) pair_evidence_kernel(uint32_t c_begin, uint32_t c_end, const MemberChunk *__restrict__ chunks, const HpSpecies *__restrict__ tab,
                                                            const uint32_t *__restrict__ node_len, const uint32_t *__restrict__ cov, const unsigned long long *__restrict__ bases,
                                                            const unsigned long long *__restrict__ node_haps, const unsigned long long *__restrict__ mask,
                                                            const uint32_t *__restrict__ bit_pos, unsigned long long *__restrict__ pair_out /*[..][4]*/,
                                                            unsigned long long *__restrict__ sp_out /*[S][3][4]*/) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint32_t c = c_begin + blockIdx.x * 4u + wave; c < c_end; c += gridDim.x * 4u) {
        const MemberChunk ch = chunks[c];
        const HpSpecies st = tab[ch.species];
        const MemberRow m = st.m;
        // ---- the species sums: block pair (0, 0) alone, every word of the node, all four quantities (the evidence kernel's sums)
        if (ch.tile == 0u) {
            MemberQ tot{0ull, 0ull, 0ull, 0ull}, orp{0ull, 0ull, 0ull, 0ull}, cor{0ull, 0ull, 0ull, 0ull};
            for (uint32_t t0 = 0; t0 < ch.n; t0 += 64u) {
                const uint32_t i = t0 + (uint32_t)lane;
                if (i < ch.n) {
                    const uint32_t v = ch.first + i;
                    uint32_t cnt = 0u;
                    if (m.route == 1u) cnt = (uint32_t)__popcll(node_haps[v] & m.bits);
                    else if (m.route == 2u) {
                        const uint64_t row = member_mask_row(m, v);
                        for (uint32_t w = 0; w < m.nw; ++w) cnt += (uint32_t)__popcll(mask[row + w]);
                    }
                    const uint32_t ln = node_len[v], cv = cov[v];
                    const unsigned long long bs = bases[v];
                    mq_add(tot, true, ln, cv, bs);
                    mq_add(orp, cnt == 0u, ln, cv, bs);
                    mq_add(cor, m.K != 0u && cnt == m.K, ln, cv, bs);
                }
            }
            tot = mq_wave_sum(tot); orp = mq_wave_sum(orp); cor = mq_wave_sum(cor);
            if (lane == 0) {
                unsigned long long *const o = sp_out + (uint64_t)ch.species * 12u;
                mq_flush(o, tot); mq_flush(o + 4, orp); mq_flush(o + 8, cor);
            }
        }
        if (m.route == 0u) continue;   // nothing selected: no block pair
        // ---- the block pair, once per plane: one quantity per counter
        const HapPairsTile bp = hap_pairs_tile(m.nw, ch.tile);
        const unsigned long long live_a = m.route == 1u ? m.bits : hap_pairs_live(m.K, bp.wa);
        const unsigned long long live_b = m.route == 1u ? m.bits : hap_pairs_live(m.K, bp.wb);
#pragma unroll   // (unrolled: the plane's quantity is then a fixed load; as a loop <64> compiles to 172 VGPRs and two waves per SIMD, unrolled to 167 and three)
        for (int plane = 0; plane < HP_PLANES; ++plane) {
            unsigned long long acc[KB];
#pragma unroll
            for (int j = 0; j < KB; ++j) acc[j] = 0ull;
            unsigned long long core = 0ull;   // per lane: its nodes that hold every live bit of both words
            HpTileQ cur = hp_load_q(ch, m, bp.wa, bp.wb, 0u, lane, plane, node_len, cov, bases, node_haps, mask);
            for (uint32_t t0 = 0; t0 < ch.n; t0 += 64u) {
                HpTileQ nxt{0ull, 0ull, 0ull};
                if (t0 + 64u < ch.n) nxt = hp_load_q(ch, m, bp.wa, bp.wb, t0 + 64u, lane, plane, node_len, cov, bases, node_haps, mask);
                const bool some = cur.a != 0ull && cur.b != 0ull, full = some && cur.a == live_a && cur.b == live_b;
                core += full ? cur.q : 0ull;
                // (no branch in the body, as above)
                for (unsigned long long todo = __builtin_amdgcn_ballot_w64(some && !full); todo; todo &= todo - 1ull) {
                    const int l = __builtin_ctzll(todo);
                    const unsigned long long a = lane_get(cur.a, l), b = lane_get(cur.b, l), q = lane_get(cur.q, l);
                    const unsigned long long mine = ((a >> lane) & 1ull) ? q : 0ull;
#pragma unroll
                    for (int j = 0; j < KB; ++j) acc[j] += mine & (0ull - ((b >> j) & 1ull));
                }
                cur = nxt;
            }
            core = wave_reduce(core, [](unsigned long long x, unsigned long long y) { return x + y; });
            // ---- flush: plane 0 into columns 0 and 1, plane 1 into column 2, plane 2 into column 3
            const bool row_on = (live_a >> lane) & 1ull;
            const uint32_t pos_a = row_on ? bit_pos[st.bit_base + 64u * bp.wa + (uint32_t)lane] : MEMBER_NO_ENTRY;
            const uint32_t pos_b_mine = ((live_b >> lane) & 1ull) ? bit_pos[st.bit_base + 64u * bp.wb + (uint32_t)lane] : MEMBER_NO_ENTRY;
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                if (!((live_b >> j) & 1ull)) continue;
                const uint32_t pos_b = lane_get(pos_b_mine, j);
                const unsigned long long x = acc[j] + core;
                if (row_on && pos_a != MEMBER_NO_ENTRY && pos_b != MEMBER_NO_ENTRY) {
                    unsigned long long *const o = pair_out + (st.pair_base + (uint64_t)pos_a * m.K + pos_b) * 4u;
                    if (plane == 0) {
                        if (x >> 48) atomicAdd(o, x >> 48);
                        if (x & HP_LEN) atomicAdd(o + 1, x & HP_LEN);
                    } else if (x) atomicAdd(o + 1 + plane, x);
                }
            }
        }
    }
}

template <int KB, bool COV>
void hp_launch(Ctx *ctx, uint32_t c0, uint32_t c1, const MemberChunk *chunks, const HpSpecies *tab, const Db *db, bool by_node, const unsigned long long *mask,
               const uint32_t *bit_pos, unsigned long long *pair_out, unsigned long long *sp_out, const char *name) {
    if (c0 == c1) return;
    KTimer tm(ctx, name);
    const dim3 grid(grid_for(c1 - c0, 4, ctx->n_cu * 16));
    const unsigned long long *const nh = by_node ? (const unsigned long long *)db->d_node_haps.p : (const unsigned long long *)nullptr;
    if constexpr (COV)
        hipLaunchKernelGGL(pair_evidence_kernel<KB>, grid, dim3(256), 0, ctx->stream, c0, c1, chunks, tab, db->d_node_len.p, (const uint32_t *)db->d_cov.p,
                           (const unsigned long long *)db->d_bases.p, nh, mask, bit_pos, pair_out, sp_out);
    else hipLaunchKernelGGL(hap_pairs_kernel<KB>, grid, dim3(256), 0, ctx->stream, c0, c1, chunks, tab, db->d_node_len.p, nh, mask, bit_pos, pair_out, sp_out);
}

// both calls behind their checks.  COV: Q has four columns and the db holds the coverage result of pantax_hip_node_coverage (the caller checked)
template <bool COV>
int hp_run(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *pair_off, uint64_t *pair_out, uint64_t *species_out) {
    constexpr size_t NQ = COV ? 4 : 2;
    const char *const what = COV ? "strain_pair_evidence" : "db_hap_pairs";
    const uint32_t S = db->S;
    const uint64_t H = db->H, C = sel_off[S], n_pair = pair_off[S];
    if (H + C >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: %llu haplotypes + selection entries exceed 32-bit positions", what, (unsigned long long)(H + C));
    if (db->V >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: %llu nodes exceed 32-bit positions", what, (unsigned long long)db->V);
    const bool by_node = member_by_node(db->nh_built, ctx->cfg.hap_pairs_route);
    std::vector<HpSpecies> tab(S ? S : 1);
    std::vector<uint32_t> bit_pos(H + C + 1, MEMBER_NO_ENTRY);   // [bit_base of the species + bit] -> position in the species' list
    std::vector<MemberChunk> by_cols[5];                         // chunks by the kernel's columns: 0 (species sums alone), 8, 16, 32, 64
    MemberPass ps;
    for (uint32_t s = 0; s < S; ++s) {
        HpSpecies &st = tab[s];
        const uint32_t *haps = sel_hap + sel_off[s];
        st.m = ps.wm.row(db, s, by_node, haps, sel_off[s + 1] - sel_off[s]);
        st.bit_base = member_bit_base(st.m.route, db->h_hap_off[s], H, sel_off[s]);
        st.pair_base = pair_off[s];
        member_file_bits(st.m.route, haps, st.m.K, 0, [&](uint64_t bit, uint64_t k) { bit_pos[st.bit_base + bit] = (uint32_t)k; });
        const uint64_t v0 = db->h_node_off[s], v1 = db->h_node_off[s + 1];
        if (st.m.route == 0u) { member_chunks_add(by_cols[0], s, v0, v1, hap_pairs_chunk(0, 0, ctx->cfg.hap_pairs_chunk), 1); continue; }
        for (uint32_t t = 0; t < hap_pairs_tiles(st.m.nw); ++t) {   // one call per tile: the chunk size and the columns are the block pair's
            const HapPairsTile bp = hap_pairs_tile(st.m.nw, t);
            const unsigned long long live_a = st.m.route == 1u ? st.m.bits : hap_pairs_live(st.m.K, bp.wa), live_b = st.m.route == 1u ? st.m.bits : hap_pairs_live(st.m.K, bp.wb);
            const uint32_t cols = hap_pairs_cols(live_b);
            std::vector<MemberChunk> &out = by_cols[cols == 8 ? 1 : cols == 16 ? 2 : cols == 32 ? 3 : 4];
            const size_t before = out.size();
            member_chunks_add(out, s, v0, v1, hap_pairs_chunk((uint32_t)__builtin_popcountll(live_a), (uint32_t)__builtin_popcountll(live_b), ctx->cfg.hap_pairs_chunk), 1);
            for (size_t i = before; i < out.size(); ++i) out[i].tile = t;
        }
    }
    std::vector<MemberChunk> chunks;
    uint32_t cut[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 5; ++k) { chunks.insert(chunks.end(), by_cols[k].begin(), by_cols[k].end()); cut[k + 1] = (uint32_t)chunks.size(); }
    if (chunks.size() >= 0xFFFFFFF0ull) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: %llu chunks exceed 32-bit positions", what, (unsigned long long)chunks.size());
    const size_t n_out = (size_t)n_pair * NQ + (size_t)S * 3 * NQ;
    if (n_out == 0) return 0;
    DevBuf<HpSpecies> d_tab;
    DevBuf<uint32_t> d_bit_pos;
    DevBuf<MemberChunk> d_chunks;
    PTX_TRY(ps.open(ctx, db, n_out));   // one device block, zero-filled once: [pair n_pair x NQ][species S x 3 NQ]
    if (!chunks.empty()) {
        PTX_TRY(upload(ctx, d_tab, tab.data(), tab.size()));
        PTX_TRY(upload(ctx, d_bit_pos, bit_pos.data(), bit_pos.size()));
        PTX_TRY(upload(ctx, d_chunks, chunks.data(), chunks.size()));
        unsigned long long *const sp = ps.d_out.p + (size_t)n_pair * NQ;
        // (the chunks without a block pair run the narrowest kernel: it leaves them behind the species sums)
        hp_launch<8, COV>(ctx, cut[0], cut[2], d_chunks.p, d_tab.p, db, by_node, ps.wm.d_mask.p, d_bit_pos.p, ps.d_out.p, sp, COV ? "pair_evidence_kernel<8>" : "hap_pairs_kernel<8>");
        hp_launch<16, COV>(ctx, cut[2], cut[3], d_chunks.p, d_tab.p, db, by_node, ps.wm.d_mask.p, d_bit_pos.p, ps.d_out.p, sp, COV ? "pair_evidence_kernel<16>" : "hap_pairs_kernel<16>");
        hp_launch<32, COV>(ctx, cut[3], cut[4], d_chunks.p, d_tab.p, db, by_node, ps.wm.d_mask.p, d_bit_pos.p, ps.d_out.p, sp, COV ? "pair_evidence_kernel<32>" : "hap_pairs_kernel<32>");
        hp_launch<64, COV>(ctx, cut[4], cut[5], d_chunks.p, d_tab.p, db, by_node, ps.wm.d_mask.p, d_bit_pos.p, ps.d_out.p, sp, COV ? "pair_evidence_kernel<64>" : "hap_pairs_kernel<64>");
    }
    // into host scratch first: a failure on the way leaves the caller's arrays as given
    std::vector<uint64_t> h_pair(n_pair * NQ ? n_pair * NQ : 1), h_sp((size_t)S * 3 * NQ ? (size_t)S * 3 * NQ : 1);
    PTX_TRY(ps.close(ctx, h_pair.data(), (size_t)n_pair * NQ, h_sp.data(), (size_t)S * 3 * NQ));
    for (uint32_t s = 0; s < S; ++s) hap_pairs_mirror(h_pair.data() + pair_off[s] * NQ, sel_off[s + 1] - sel_off[s], (uint32_t)NQ);
    if (n_pair) std::copy(h_pair.begin(), h_pair.begin() + (ptrdiff_t)(n_pair * NQ), pair_out);
    if (species_out && S) std::copy(h_sp.begin(), h_sp.begin() + (ptrdiff_t)((size_t)S * 3 * NQ), species_out);
    return 0;
}

}  // namespace

// sel_off [S+1], sel_hap validated by the caller (in range, no repeats within a species, K_s <= HAP_PAIRS_MAX_K); pair_off [S+1] = hap_pairs_offsets
int hap_pairs_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *pair_off, uint64_t *pair_out, uint64_t *species_out) {
    return hp_run<false>(ctx, db, sel_off, sel_hap, pair_off, pair_out, species_out);
}
// ... and the db holding the coverage result of pantax_hip_node_coverage: pair_out [..][4], species_out [S][3][4]
int pair_evidence_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *pair_off, uint64_t *pair_out, uint64_t *species_out) {
    return hp_run<true>(ctx, db, sel_off, sel_hap, pair_off, pair_out, species_out);
}

}  // namespace ptx
