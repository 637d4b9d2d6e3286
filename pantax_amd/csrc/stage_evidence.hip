// stage_evidence.hip -- per-strain node evidence (pantax_hip_strain_evidence, the --strain-evidence report): what in the sample separates a reported
// strain from the other reported strains of its species, and how much of the species' coverage no reported strain explains.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Per-strain node evidence"): for the selected haplotypes Sel_s of a species (K_s of them) every node v of the
// species is counted once; M(v) = the selected haplotypes whose walk visits v (node-level membership: a node walked twice counts once), m(v) = |M(v)|,
// Q(v) = (1, node_len[v], node_base_cov[v], bases_per_node[v]) as u64.  Per selection entry: all = sum of Q over the nodes the haplotype visits, private =
// over the nodes with M(v) = {the haplotype}.  Per species: total (every node), orphan (m = 0), core (m = K_s, K_s >= 1).  Integers only: no order matters.
//
// Membership: the two routes of member_plan.hpp over the selected haplotypes (option evidence_route), nw = ceil(K_s / 64) words per node on route 2.
// evidence_node_kernel: the host cuts every species' nodes into chunks of EV_CHUNK nodes; a chunk goes to a WAVE (four chunks in flight per workgroup: a
// species of a few thousand nodes still spreads over several CUs, and nothing in the pass needs a workgroup barrier).  The wave takes its chunk in
// tiles of 256 nodes, lane l the nodes l, l + 64, l + 128, l + 192 of the tile: every load instruction is one contiguous stretch of 256 or 512 bytes.
//   species sums   in lane registers over the whole chunk, one DPP wave reduction per sum at its end, one 64-bit atomicAdd per non-zero sum;
//   haplotype sums the WAVE reduces per selected bit (not a lane per set bit with LDS atomics): K_s is small -- 1.6 reported strains a species at cfg4 --
//                  while a core node sets the same bits in every lane, so 64 lanes would queue on the same K_s LDS counters at every node; here a bit
//                  costs eight DPP reductions per 256 nodes, and a bit no node of the tile carries is skipped after one ballot.  Lane 0 adds the
//                  reduced sums to the wave's 64 x 2 x 4 u64 counters in LDS (4 KB a wave; a plain add: the counters have one writer), and at the end
//                  of the chunk lane b flushes the counters of bit b, one 64-bit atomicAdd per non-zero counter.
// A species of more than 64 selected haplotypes goes through the chunk once per mask word, word w serving the candidates 64w .. 64w + 63 through the same
// counters; private (one bit over ALL words) and core (popcount over all words = K_s) look at every word of the node in each pass.  No floating point.
//
// Algorithmic bytes (V nodes, C selection entries, S species), route 1:  (4 + 4 + 8 + 8) V in, 64 C + 96 S out.
// Route 2, a species of V_s nodes and nw = ceil(K_s / 64) words: nw passes that each read (4 + 4 + 8) + 8 nw bytes per node = (16 nw + 8 nw^2) V_s (the
// repeats come from L2 at best), behind the mask pass's 4 P_sel + 8 nw V_s (zero fill) + one 8-byte atomic per visit.
#include <algorithm>
#include "common.hpp"
#include "member_device.hpp"
#include "primitives.hpp"

namespace ptx {

namespace {

constexpr uint32_t EV_CHUNK = 1024;   // nodes per chunk (one wave)
constexpr uint32_t EV_TILE = 256;     // nodes the wave holds in registers at a time: four per lane

struct EvSpecies { MemberRow m; uint32_t bit_base, pad; };   // bit_base: first entry of the species in bit_entry

__global__ void __launch_bounds__(256) evidence_node_kernel(uint32_t n_chunks, const MemberChunk *__restrict__ chunks, const EvSpecies *__restrict__ tab,
                                                            const uint32_t *__restrict__ node_len, const uint32_t *__restrict__ cov,
                                                            const unsigned long long *__restrict__ bases, const unsigned long long *__restrict__ node_haps,
                                                            const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ bit_entry,
                                                            unsigned long long *__restrict__ hap_out /*[C][2][4]*/, unsigned long long *__restrict__ sp_out /*[S][3][4]*/) {
    __shared__ unsigned long long s_cnt[4][8 * 64];   // per wave: [all n, len, cov, bases, private n, len, cov, bases][bit]
    const int lane = threadIdx.x & 63;
    unsigned long long *const cnt = s_cnt[threadIdx.x >> 6];
    for (uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n_chunks; c += gridDim.x * 4) {   // (everything below is uniform over the wave but the lane's nodes)
        const MemberChunk ch = chunks[c];
        const EvSpecies st = tab[ch.species];
        MemberQ tot{0ull, 0ull, 0ull, 0ull}, orp{0ull, 0ull, 0ull, 0ull}, cor{0ull, 0ull, 0ull, 0ull};
        const uint32_t passes = st.m.route ? st.m.nw : 1u;
        for (uint32_t w = 0; w < passes; ++w) {
            // the bits of word w that stand for a selected haplotype
            const uint32_t left = st.m.route == 2u ? st.m.K - 64u * w : 0u;
            const unsigned long long live = st.m.route == 1u ? st.m.bits : (st.m.route == 2u ? (left >= 64u ? ~0ull : (1ull << left) - 1ull) : 0ull);
#pragma unroll
            for (int q = 0; q < 8; ++q) cnt[q * 64 + lane] = 0ull;
            member_wave_sync();
            for (uint32_t t0 = 0; t0 < ch.n; t0 += EV_TILE) {
                uint32_t ln[4], cv[4];
                unsigned long long bs[4], wd[4];
                bool on[4], one[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t i = t0 + 64u * j + (uint32_t)lane;
                    on[j] = i < ch.n;
                    const uint32_t v = ch.first + (on[j] ? i : 0u);   // (a dead lane reads the chunk's first node and drops it)
                    ln[j] = node_len[v]; cv[j] = cov[v]; bs[j] = bases[v];
                    unsigned long long word = 0ull;
                    uint32_t m = 0u;
                    if (st.m.route == 1u) { word = node_haps[v] & st.m.bits; m = (uint32_t)__popcll(word); }
                    else if (st.m.route == 2u) {
                        const uint64_t row = member_mask_row(st.m, v);
                        for (uint32_t w2 = 0; w2 < st.m.nw; ++w2) {
                            const unsigned long long x = mask[row + w2];
                            m += (uint32_t)__popcll(x);
                            word = w2 == w ? x : word;
                        }
                    }
                    wd[j] = on[j] ? word : 0ull;
                    one[j] = m == 1u;
                    if (w == 0u) {   // the species sums see every node once: in the first pass
                        mq_add(tot, on[j], ln[j], cv[j], bs[j]);
                        mq_add(orp, on[j] & (m == 0u), ln[j], cv[j], bs[j]);
                        mq_add(cor, on[j] & (st.m.K != 0u) & (m == st.m.K), ln[j], cv[j], bs[j]);
                    }
                }
                const unsigned long long mine = wd[0] | wd[1] | wd[2] | wd[3];
                for (unsigned long long rem = live; rem; rem &= rem - 1ull) {
                    const int b = __builtin_ctzll(rem);
                    if (__builtin_amdgcn_ballot_w64((mine >> b) & 1ull) == 0ull) continue;   // no node of the tile carries the bit
                    MemberQ a{0ull, 0ull, 0ull, 0ull}, p{0ull, 0ull, 0ull, 0ull};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool has = (wd[j] >> b) & 1ull;
                        mq_add(a, has, ln[j], cv[j], bs[j]);
                        mq_add(p, has & one[j], ln[j], cv[j], bs[j]);
                    }
                    a = mq_wave_sum(a);
                    p = mq_wave_sum(p);
                    if (lane == 0) {
                        cnt[0 * 64 + b] += a.n; cnt[1 * 64 + b] += a.len; cnt[2 * 64 + b] += a.cov; cnt[3 * 64 + b] += a.bases;
                        cnt[4 * 64 + b] += p.n; cnt[5 * 64 + b] += p.len; cnt[6 * 64 + b] += p.cov; cnt[7 * 64 + b] += p.bases;
                    }
                }
            }
            member_wave_sync();
            if ((live >> lane) & 1ull) {   // lane b owns bit b of this word
                const uint32_t e = bit_entry[st.bit_base + 64u * w + (uint32_t)lane];
                if (e != MEMBER_NO_ENTRY) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const unsigned long long x = cnt[q * 64 + lane];
                        if (x) atomicAdd(hap_out + (uint64_t)e * 8u + q, x);
                    }
                }
            }
            member_wave_sync();   // (the counters are zeroed again by the next pass or chunk)
        }
        tot = mq_wave_sum(tot); orp = mq_wave_sum(orp); cor = mq_wave_sum(cor);
        if (lane == 0) {
            unsigned long long *const o = sp_out + (uint64_t)ch.species * 12u;
            mq_flush(o, tot); mq_flush(o + 4, orp); mq_flush(o + 8, cor);
        }
    }
}

}  // namespace

// sel_off [S+1], sel_hap validated by the caller (in range, no repeats within a species)
int evidence_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, uint64_t *hap_out, uint64_t *species_out) {
    const uint32_t S = db->S;
    const uint64_t H = db->H, C = sel_off[S];
    if (H + C >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_evidence: %llu haplotypes + selection entries exceed 32-bit positions", (unsigned long long)(H + C));
    if (db->V >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_evidence: %llu nodes exceed 32-bit positions", (unsigned long long)db->V);
    const bool by_node = member_by_node(db->nh_built, ctx->cfg.evidence_route);
    std::vector<EvSpecies> tab(S ? S : 1);
    std::vector<uint32_t> bit_entry(H + C + 1, MEMBER_NO_ENTRY);   // [bit_base of the species + bit] -> selection entry
    std::vector<MemberChunk> chunks;
    MemberPass ps;
    for (uint32_t s = 0; s < S; ++s) {
        EvSpecies &st = tab[s];
        st.m = ps.wm.row(db, s, by_node, sel_hap + sel_off[s], sel_off[s + 1] - sel_off[s]);
        st.bit_base = member_bit_base(st.m.route, db->h_hap_off[s], H, sel_off[s]);
        member_file_bits(st.m.route, sel_hap + sel_off[s], st.m.K, 0, [&](uint64_t bit, uint64_t k) { bit_entry[st.bit_base + bit] = (uint32_t)(sel_off[s] + k); });
        member_chunks_add(chunks, s, db->h_node_off[s], db->h_node_off[s + 1], EV_CHUNK, 1);
    }
    const size_t n_out = (size_t)C * 8 + (size_t)S * 12;
    if (n_out == 0) return 0;
    DevBuf<EvSpecies> d_tab;
    DevBuf<uint32_t> d_bit_entry;
    DevBuf<MemberChunk> d_chunks;
    PTX_TRY(ps.open(ctx, db, n_out));   // one device block, zero-filled once: [hap C x 8][species S x 12]
    if (!chunks.empty()) {
        PTX_TRY(upload(ctx, d_tab, tab.data(), tab.size()));
        PTX_TRY(upload(ctx, d_bit_entry, bit_entry.data(), bit_entry.size()));
        PTX_TRY(upload(ctx, d_chunks, chunks.data(), chunks.size()));
        KTimer tm(ctx, "evidence_node_kernel");
        hipLaunchKernelGGL(evidence_node_kernel, dim3(grid_for(chunks.size(), 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, (uint32_t)chunks.size(), d_chunks.p, d_tab.p,
                           db->d_node_len.p, db->d_cov.p, db->d_bases.p, by_node ? (const unsigned long long *)db->d_node_haps.p : (const unsigned long long *)nullptr,
                           ps.wm.d_mask.p, d_bit_entry.p, ps.d_out.p, ps.d_out.p + (size_t)C * 8);
    }
    return ps.close(ctx, hap_out, (size_t)C * 8, species_out, (size_t)S * 12);
}

}  // namespace ptx
