// stage_near_miss.hip -- unreported-strain near misses (pantax_hip_strain_near_miss, the --strain-near-miss report): which haplotypes of the db that are
// NOT in the strain table would explain the coverage on the nodes no reported strain walks (the evidence report's `orphan`).  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Unreported-strain near misses"): Sel_s = the reported haplotypes of a species (K_s), Cand_s = the candidates
// (J_s), disjoint.  Every node v of the species is counted once; M(v) / N(v) = the haplotypes of Sel_s / Cand_s whose walk visits v (node-level membership),
// m = |M|, n = |N|, Q(v) = (1, node_len[v], node_base_cov[v], bases_per_node[v]) as u64.  Per candidate entry: novel = sum of Q over m(v) = 0 and h in N(v),
// exclusive = over m(v) = 0 and N(v) = {h}.  Per species: orphan (m = 0), claimed (m = 0, n >= 1), contested (m = 0, n >= 2).  Integers only.
//
// Membership: the two routes of member_plan.hpp (option near_miss_route) over the LIST Sel_s ++ Cand_s, laid out by near_miss_layout:
//   route 1 -- one word per node, x = node_haps[v]; orphan: x & Sel's bits = 0; candidate word: x & cand_bits, bit = haplotype index;
//   route 2 -- bit = position in the list.  Sel ends at bit K_s, in the middle of word K_s / 64: that word serves both sets under two masks.
// near_miss_node_kernel: chunks of NM_CHUNK nodes of one species, a chunk per WAVE, tiles of 256 nodes, lane l the nodes l, l + 64, l + 128, l + 192 -- the
// mapping of evidence_node_kernel.  What differs is that J is not small (every unreported haplotype of a species, possibly all 64 bits of a word) and that
// only orphan nodes add to anything:
//   1. the wave loads the membership word(s) of Sel alone and forms the orphan predicate; one ballot per tile: a tile without an orphan loads nothing
//      else (not node_len, cov, bases; on route 2 not its candidate words) and does no per-candidate work;
//   2. the orphan lanes load Q and their candidate words, ONCE (a word shared with Sel is kept from step 1); non-orphan lanes hold zeros;
//   3. species sums (orphan, claimed, contested) in lane registers over the chunk, one DPP reduction per sum at its end;
//   4. candidate sums are reduced over the WAVE per set bit (not a lane per orphan node with LDS atomics: the nodes of a tile share their candidates, so
//      the lanes would queue on the same few counters, 64 deep on a core node).  Per candidate word of the tile: one OR-reduction says which bits occur
//      at all; one AND-reduction over the claimed nodes finds the bits EVERY claimed node of the tile carries -- those bits' novel sums all equal the
//      tile's claimed sum, reduced once (four reductions) however many they are; every other occurring bit costs four reductions (novel), and a bit that
//      is some node's only candidate four more (exclusive).  All lanes hold a reduced sum; lane b adds it to the counters of bit b.
//   The counters are [candidate word][novel n, len, cov, bases, exclusive n, len, cov, bases][bit] u64 in LDS, 4 KB per wave and candidate word; lane b is
//   the only lane that ever touches the counters of bit b (zero, add, flush), so the pass needs no barrier and no LDS atomic.  At the end of the chunk
//   lane b flushes them, one 64-bit atomicAdd per non-zero counter.
// A wave counts up to W = min(4, the db's widest candidate set in words) candidate words in ONE pass over its nodes (dynamic LDS: 16 KB x W a workgroup).  A
// species with more candidate words than W goes through its chunk once per W words (the counters are tiled over the words); every pass still reads all
// the candidate words of an orphan node, for n(v).  The species sums are formed in the first pass.  No floating point.
//
// Algorithmic bytes (V nodes, V_o of them in tiles that hold an orphan, J candidate entries, S species), route 1: 8 V + 16 V_o in, 64 J + 96 S out.
// Route 2, a species of nw words, sw = ceil(K_s / 64) of them Sel's, cw candidate words: 8 sw V_s + (16 + 8 cw) V_o,s per pass (lanes of non-orphan nodes in a
// loaded tile are masked off; their cache lines still travel), behind the mask pass's 4 P_list + 8 nw V_s (zero fill) + one 8-byte atomic per visit.
#include <algorithm>
#include "common.hpp"
#include "member_device.hpp"
#include "primitives.hpp"

namespace ptx {

namespace {

constexpr uint32_t NM_CHUNK = 1024;   // nodes per chunk (one wave)
constexpr uint32_t NM_TILE = 256;     // nodes the wave holds in registers at a time: four per lane
constexpr uint32_t NM_WORDS = 4;      // candidate words a wave counts per pass, at most (16 KB of LDS a wave)

struct NmSpecies {
    MemberRow m;                    // over Sel ++ Cand, but K and (route 1) bits are Sel's alone
    unsigned long long cand_bits;   // route 1: bit j = haplotype j is a candidate
    uint32_t J, w0, cwn;            // candidates; near_miss_layout: the word of the first candidate bit, the candidate words of a node
    uint32_t bit_base;              // candidate word k (from w0), bit b -> bit_entry[bit_base + 64 k + b]
};

// lane `lane` adds a wave-uniform sum to its own counters of class `cls` (0: novel, 1: exclusive) where its bit is in `bits`
__device__ __forceinline__ void nm_count(unsigned long long *cnt, int lane, unsigned long long bits, int cls, const MemberQ &a) {
    if ((bits >> lane) & 1ull) {
        cnt[(cls * 4 + 0) * 64 + lane] += a.n; cnt[(cls * 4 + 1) * 64 + lane] += a.len;
        cnt[(cls * 4 + 2) * 64 + lane] += a.cov; cnt[(cls * 4 + 3) * 64 + lane] += a.bases;
    }
}

// MAXW: the candidate words a lane holds in registers per node (1: no species of the launch has more than one candidate word -- the whole of route 1)
template <uint32_t MAXW>
__global__ void __launch_bounds__(256) near_miss_node_kernel(uint32_t n_chunks, uint32_t W /* candidate words per pass: 1 .. MAXW */, const MemberChunk *__restrict__ chunks,
                                                             const NmSpecies *__restrict__ tab, const uint32_t *__restrict__ node_len, const uint32_t *__restrict__ cov,
                                                             const unsigned long long *__restrict__ bases, const unsigned long long *__restrict__ node_haps,
                                                             const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ bit_entry,
                                                             unsigned long long *__restrict__ cand_out /*[J][2][4]*/, unsigned long long *__restrict__ sp_out /*[S][3][4]*/) {
    extern __shared__ unsigned long long s_cnt[];   // per wave: [W][novel n, len, cov, bases, exclusive n, len, cov, bases][bit]
    const int lane = threadIdx.x & 63;
    unsigned long long *const cnt = s_cnt + (size_t)(threadIdx.x >> 6) * W * 512u;
    const auto bit_or = [](unsigned long long x, unsigned long long y) { return x | y; };
    const auto bit_and = [](unsigned long long x, unsigned long long y) { return x & y; };
    for (uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n_chunks; c += gridDim.x * 4) {   // (everything below is uniform over the wave but the lane's nodes)
        const MemberChunk ch = chunks[c];
        const NmSpecies st = tab[ch.species];
        MemberQ orp{0ull, 0ull, 0ull, 0ull}, cla{0ull, 0ull, 0ull, 0ull}, con{0ull, 0ull, 0ull, 0ull};
        // route 2: Sel's words are 0 .. sw - 1, the last of them cut at bit K % 64; the candidates start at that bit of word w0
        const uint32_t sw = st.m.route == 2u ? member_words(st.m.K) : 0u;
        const unsigned long long sel_last = (st.m.K & 63u) ? (1ull << (st.m.K & 63u)) - 1ull : ~0ull;
        const uint32_t passes = st.cwn ? (st.cwn + W - 1u) / W : 1u;
        for (uint32_t p = 0; p < passes; ++p) {
            const uint32_t k0 = p * W, kn = st.cwn > k0 ? min(W, st.cwn - k0) : 0u;   // this pass counts the candidate words k0 .. k0 + kn - 1
            for (uint32_t k = 0; k < kn; ++k)
#pragma unroll
                for (int q = 0; q < 8; ++q) cnt[(k * 8u + q) * 64u + lane] = 0ull;
            for (uint32_t t0 = 0; t0 < ch.n; t0 += NM_TILE) {
                uint32_t vv[4];
                unsigned long long first[4];   // route 1: the node's word; route 2: word w0 where Sel's last word is also the candidates' first
                bool orph[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t i = t0 + 64u * j + (uint32_t)lane;
                    const bool on = i < ch.n;
                    vv[j] = ch.first + (on ? i : 0u);   // (a dead lane reads the chunk's first node and drops it)
                    first[j] = 0ull;
                    bool free_of_sel = true;
                    if (st.m.route == 1u) { first[j] = node_haps[vv[j]]; free_of_sel = (first[j] & st.m.bits) == 0ull; }
                    else if (st.m.route == 2u) {
                        const uint64_t row = member_mask_row(st.m, vv[j]);
                        for (uint32_t w = 0; w < sw; ++w) {
                            const unsigned long long x = mask[row + w];
                            free_of_sel = free_of_sel && (x & (w + 1u == sw ? sel_last : ~0ull)) == 0ull;
                            first[j] = w == st.w0 ? x : first[j];
                        }
                    }
                    orph[j] = on && free_of_sel;
                }
                if (__builtin_amdgcn_ballot_w64(orph[0] | orph[1] | orph[2] | orph[3]) == 0ull) continue;   // no orphan in the tile: nothing to load, nothing to count
                uint32_t ln[4], cv[4], nn[4];
                unsigned long long bs[4], wd[4][MAXW];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ln[j] = 0u; cv[j] = 0u; bs[j] = 0ull; nn[j] = 0u;
#pragma unroll
                    for (uint32_t kk = 0; kk < MAXW; ++kk) wd[j][kk] = 0ull;
                    if (!orph[j]) continue;
                    ln[j] = node_len[vv[j]]; cv[j] = cov[vv[j]]; bs[j] = bases[vv[j]];
                    if (st.m.route == 1u) { wd[j][0] = first[j] & st.cand_bits; nn[j] = (uint32_t)__popcll(wd[j][0]); }   // (cwn <= 1: k0 = 0)
                    else if (st.m.route == 2u) {
                        const uint64_t row = member_mask_row(st.m, vv[j]) + st.w0;
                        for (uint32_t k = 0; k < st.cwn; ++k) {   // every candidate word for n(v); the words of this pass stay in registers
                            unsigned long long x = (k == 0u && st.w0 < sw) ? first[j] : mask[row + k];
                            if (k == 0u) x &= ~((1ull << (st.m.K & 63u)) - 1ull);   // the bits below K % 64 of word w0 are Sel's
                            nn[j] += (uint32_t)__popcll(x);
                            const uint32_t r = k - k0;
#pragma unroll
                            for (uint32_t kk = 0; kk < MAXW; ++kk) wd[j][kk] = r == kk ? x : wd[j][kk];
                        }
                    }
                }
                if (p == 0u) {   // the species sums see every node once: in the first pass
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        mq_add(orp, orph[j], ln[j], cv[j], bs[j]);
                        mq_add(cla, orph[j] & (nn[j] >= 1u), ln[j], cv[j], bs[j]);
                        mq_add(con, orph[j] & (nn[j] >= 2u), ln[j], cv[j], bs[j]);
                    }
                }
                if (__builtin_amdgcn_ballot_w64((nn[0] | nn[1] | nn[2] | nn[3]) != 0u) == 0ull) continue;   // orphans no candidate walks
                bool have_claimed = false;
                MemberQ claimed{0ull, 0ull, 0ull, 0ull};   // the tile's claimed sum, reduced when the first word needs it
#pragma unroll
                for (uint32_t kk = 0; kk < MAXW; ++kk) {
                    if (kk >= kn) break;
                    unsigned long long *const ck = cnt + kk * 512u;
                    const unsigned long long occurs = wave_reduce(wd[0][kk] | wd[1][kk] | wd[2][kk] | wd[3][kk], bit_or);
                    if (occurs == 0ull) continue;
                    // bits every claimed node of the tile carries: their novel sums are the tile's claimed sum
                    unsigned long long every = ~0ull, alone = 0ull;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { every &= nn[j] >= 1u ? wd[j][kk] : ~0ull; alone |= nn[j] == 1u ? wd[j][kk] : 0ull; }
                    every = wave_reduce(every, bit_and);
                    if (every) {
                        if (!have_claimed) {
                            MemberQ a{0ull, 0ull, 0ull, 0ull};
#pragma unroll
                            for (int j = 0; j < 4; ++j) mq_add(a, nn[j] >= 1u, ln[j], cv[j], bs[j]);
                            claimed = mq_wave_sum(a);
                            have_claimed = true;
                        }
                        nm_count(ck, lane, every, 0, claimed);
                    }
                    for (unsigned long long rem = occurs & ~every; rem; rem &= rem - 1ull) {   // novel: the nodes that carry the bit
                        const int b = __builtin_ctzll(rem);
                        MemberQ a{0ull, 0ull, 0ull, 0ull};
#pragma unroll
                        for (int j = 0; j < 4; ++j) mq_add(a, (wd[j][kk] >> b) & 1ull, ln[j], cv[j], bs[j]);
                        nm_count(ck, lane, 1ull << b, 0, mq_wave_sum(a));
                    }
                    for (unsigned long long rem = wave_reduce(alone, bit_or); rem; rem &= rem - 1ull) {   // exclusive: the nodes whose only candidate it is
                        const int b = __builtin_ctzll(rem);
                        MemberQ a{0ull, 0ull, 0ull, 0ull};
#pragma unroll
                        for (int j = 0; j < 4; ++j) mq_add(a, (nn[j] == 1u) & (bool)((wd[j][kk] >> b) & 1ull), ln[j], cv[j], bs[j]);
                        nm_count(ck, lane, 1ull << b, 1, mq_wave_sum(a));
                    }
                }
            }
            for (uint32_t k = 0; k < kn; ++k) {   // lane b owns bit b of every word
                const uint32_t e = bit_entry[st.bit_base + 64u * (k0 + k) + (uint32_t)lane];
                if (e == MEMBER_NO_ENTRY) continue;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const unsigned long long x = cnt[(k * 8u + q) * 64u + lane];
                    if (x) atomicAdd(cand_out + (uint64_t)e * 8u + q, x);
                }
            }
        }
        orp = mq_wave_sum(orp); cla = mq_wave_sum(cla); con = mq_wave_sum(con);
        if (lane == 0) {
            unsigned long long *const o = sp_out + (uint64_t)ch.species * 12u;
            mq_flush(o, orp); mq_flush(o + 4, cla); mq_flush(o + 8, con);
        }
    }
}

}  // namespace

// both sets validated by the caller (in range, no repeats within a species, disjoint)
int near_miss_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *cand_off, const uint32_t *cand_hap, uint64_t *cand_out,
                     uint64_t *species_out) {
    const uint32_t S = db->S;
    const uint64_t J = cand_off[S];
    if (db->H + sel_off[S] + J >= 0xFFFFFFFFull)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_near_miss: %llu haplotypes + entries exceed 32-bit positions", (unsigned long long)(db->H + sel_off[S] + J));
    if (db->V >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_near_miss: %llu nodes exceed 32-bit positions", (unsigned long long)db->V);
    const bool by_node = member_by_node(db->nh_built, ctx->cfg.near_miss_route);
    std::vector<NmSpecies> tab(S ? S : 1);
    std::vector<uint32_t> bit_entry(1, MEMBER_NO_ENTRY);   // [species' bit_base + 64 candidate word + bit] -> candidate entry
    std::vector<MemberChunk> chunks;
    std::vector<uint32_t> list;
    MemberPass ps;
    uint32_t widest = 1;
    for (uint32_t s = 0; s < S; ++s) {
        NmSpecies &st = tab[s];
        const uint32_t *sel = sel_hap + sel_off[s], *cand = cand_hap + cand_off[s];
        const uint64_t K = sel_off[s + 1] - sel_off[s], Js = cand_off[s + 1] - cand_off[s];
        list.assign(sel, sel + K); list.insert(list.end(), cand, cand + Js);
        const MemberRow row = ps.wm.row(db, s, by_node, list.data(), K + Js);
        const NearMissLayout lay = near_miss_layout(K, Js, row.route);
        st = NmSpecies{row, row.route == 1u ? member_bits(cand, Js) : 0ull, (uint32_t)Js, lay.w0, lay.cwn, (uint32_t)bit_entry.size()};
        st.m.K = (uint32_t)K; st.m.bits &= ~st.cand_bits;   // (the sets are disjoint)
        bit_entry.resize(bit_entry.size() + 64ull * st.cwn, MEMBER_NO_ENTRY);
        member_file_bits(row.route, cand, Js, lay.cand0, [&](uint64_t bit, uint64_t i) { bit_entry[st.bit_base + bit] = (uint32_t)(cand_off[s] + i); });
        widest = std::max(widest, st.cwn);
        if (bit_entry.size() >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_near_miss: %llu candidate bits exceed 32-bit positions", (unsigned long long)bit_entry.size());
        member_chunks_add(chunks, s, db->h_node_off[s], db->h_node_off[s + 1], NM_CHUNK, 1);
    }
    const int cap = ctx->cfg.near_miss_words;
    if (cap < 0 || cap > (int)NM_WORDS) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_near_miss: near_miss_words %d (1 .. %u)", cap, NM_WORDS);
    const uint32_t W = std::min(widest, cap ? (uint32_t)cap : NM_WORDS);
    const size_t n_out = (size_t)J * 8 + (size_t)S * 12;
    if (n_out == 0) return 0;
    DevBuf<NmSpecies> d_tab;
    DevBuf<uint32_t> d_bit_entry;
    DevBuf<MemberChunk> d_chunks;
    PTX_TRY(ps.open(ctx, db, n_out));   // one device block, zero-filled once: [candidates J x 8][species S x 12]
    if (!chunks.empty()) {
        PTX_TRY(upload(ctx, d_tab, tab.data(), tab.size()));
        PTX_TRY(upload(ctx, d_bit_entry, bit_entry.data(), bit_entry.size()));
        PTX_TRY(upload(ctx, d_chunks, chunks.data(), chunks.size()));
        KTimer tm(ctx, "near_miss_node_kernel");
        hipLaunchKernelGGL(W == 1u ? near_miss_node_kernel<1> : near_miss_node_kernel<NM_WORDS>, dim3(grid_for(chunks.size(), 4, ctx->n_cu * 16)), dim3(256), 4u * W * 512u * sizeof(unsigned long long), ctx->stream,
                           (uint32_t)chunks.size(), W, d_chunks.p, d_tab.p, db->d_node_len.p, db->d_cov.p, db->d_bases.p,
                           by_node ? (const unsigned long long *)db->d_node_haps.p : (const unsigned long long *)nullptr, ps.wm.d_mask.p, d_bit_entry.p, ps.d_out.p,
                           ps.d_out.p + (size_t)J * 8);
    }
    return ps.close(ctx, cand_out, (size_t)J * 8, species_out, (size_t)S * 12);
}

}  // namespace ptx
