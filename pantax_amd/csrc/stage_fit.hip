// stage_fit.hip -- model fit per strain (pantax_hip_strain_fit, the --strain-fit report): how far the coverages a table of strains predicts are from the
// sample, node by node -- the nodes without coverage included, which the LP of the strain step never sees.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Model fit per strain"): Sel_s, K_s, M(v), m(v) as in the evidence call; every selection entry carries a
// predicted coverage sel_w.  p(v) = the f64 sum of sel_w over M(v), from +0.0, in ascending haplotype index, plain IEEE additions; t(v) = p(v) * (double)
// node_len[v], one IEEE multiplication; E(v) = 0 when !(t > 0), 2^62 when t >= 2^62, else t rounded to the nearest integer, ties to even (v_rndne_f64);
// b(v) = bases_per_node[v].  Q(v) = (1, len, b, E, excess = max(b - E, 0), deficit = max(E - b, 0), blind = (b == 0 && E > 0), blind ? E : 0) as u64.
// Per selection entry: all = sum of Q over the nodes the haplotype visits, private = over the nodes with M(v) = {the haplotype}.  Per species: total
// (every node), explained (m >= 1), orphan (m = 0).  E(v) is a function of the inputs alone and the sums are integers: no order matters.
//
// Membership: the two routes of member_plan.hpp over the selected haplotypes (option fit_route), nw = ceil(K_s / 64) words per node on route 2.  The
// launcher hands every species' list to the plan SORTED by haplotype index, so on both routes ascending bit order (over all words of the node) is the
// contract's order of the sum; bit_w holds the weight of every bit beside bit_entry, its selection entry.
// fit_node_kernel: the shape of evidence_node_kernel (stage_evidence.hip) -- a chunk of FIT_CHUNK nodes to a wave, four chunks in flight per workgroup,
// tiles of 256 nodes, lane l the nodes l, l + 64, l + 128, l + 192; nothing needs a workgroup barrier.
//   p(v), E(v)     per lane and node: a walk over the set bits of the node's word(s) in ascending order, one gathered 8-byte weight and one v_add_f64 a bit;
//   species sums   total (8 sums) and orphan (3: on an orphan node E = 0, so its Q is (1, len, b, 0, b, 0, 0, 0)) in lane registers over the chunk, one
//                  DPP wave reduction per sum at its end; explained = total - orphan, column by column; one 64-bit atomicAdd per non-zero sum;
//   haplotype sums the wave reduces per selected bit, 16 DPP reductions per 256 nodes and bit; a bit no node of the tile carries is skipped after one
//                  ballot.  Lane 0 adds to the wave's 64 x 2 x 8 u64 counters in LDS (8 KB a wave, 32 KB a workgroup: five workgroups a CU; a plain add:
//                  the counters have one writer), lane b flushes the counters of bit b at the chunk's end, one 64-bit atomicAdd per non-zero counter.
// A species of more than 64 selected haplotypes goes through the chunk once per mask word; p, m and E look at every word of the node in each pass.
//
// Algorithmic bytes (V nodes, C selection entries, S species), route 1:  (4 + 8 + 8) V in (node_base_cov is not read), 128 C + 192 S out; the weights
// (8 C) stay in cache.  Route 2, a species of V_s nodes and nw words: nw passes that each read (4 + 8) + 8 nw bytes per node = (12 nw + 8 nw^2) V_s,
// behind the mask pass's 4 P_sel + 8 nw V_s (zero fill) + one 8-byte atomic per visit.
#include <algorithm>
#include <numeric>
#include "common.hpp"
#include "member_device.hpp"
#include "primitives.hpp"

namespace ptx {

namespace {

constexpr uint32_t FIT_CHUNK = 1024;   // nodes per chunk (one wave)
constexpr uint32_t FIT_TILE = 256;     // nodes the wave holds in registers at a time: four per lane
constexpr int FIT_N = 8;               // sums a class: {n_nodes, len, bases, expected, excess, deficit, blind_nodes, blind_expected}

struct FitSpecies { MemberRow m; uint32_t bit_base, pad; };   // bit_base: first entry of the species in bit_entry and bit_w

// p += the weights of the set bits of x in ascending order (w: the weight of bit 0 of this word); no contraction, no reassociation
__device__ __forceinline__ double fit_weights(double p, unsigned long long x, const double *__restrict__ w) {
#pragma clang fp contract(off)
    for (; x; x &= x - 1ull) p = __dadd_rn(p, w[__builtin_ctzll(x)]);
    return p;
}
// E(v) of the contract from p(v) and the node's length
__device__ __forceinline__ unsigned long long fit_expected(double p, uint32_t len) {
#pragma clang fp contract(off)
    const double t = __dmul_rn(p, (double)len);
    if (!(t > 0.0)) return 0ull;
    if (t >= 4611686018427387904.0) return 1ull << 62;
    return (unsigned long long)__builtin_rint(t);   // v_rndne_f64: nearest, ties to even
}
__device__ __forceinline__ void fit_add(unsigned long long (&a)[FIT_N], bool on, uint32_t len, unsigned long long b, unsigned long long e) {
    const bool blind = b == 0ull && e != 0ull;
    a[0] += on ? 1ull : 0ull; a[1] += on ? (unsigned long long)len : 0ull; a[2] += on ? b : 0ull; a[3] += on ? e : 0ull;
    a[4] += on && b > e ? b - e : 0ull; a[5] += on && e > b ? e - b : 0ull;
    a[6] += on && blind ? 1ull : 0ull; a[7] += on && blind ? e : 0ull;
}
__device__ __forceinline__ unsigned long long fit_wave_sum(unsigned long long x) {
    return wave_reduce(x, [](unsigned long long a, unsigned long long b) { return a + b; });
}

__global__ void __launch_bounds__(256) fit_node_kernel(uint32_t n_chunks, const MemberChunk *__restrict__ chunks, const FitSpecies *__restrict__ tab,
                                                       const uint32_t *__restrict__ node_len, const unsigned long long *__restrict__ bases,
                                                       const unsigned long long *__restrict__ node_haps, const unsigned long long *__restrict__ mask,
                                                       const uint32_t *__restrict__ bit_entry, const double *__restrict__ bit_w,
                                                       unsigned long long *__restrict__ hap_out /*[C][2][8]*/, unsigned long long *__restrict__ sp_out /*[S][3][8]*/) {
    __shared__ unsigned long long s_cnt[4][2 * FIT_N * 64];   // per wave: [all x 8, private x 8][bit]
    const int lane = threadIdx.x & 63;
    unsigned long long *const cnt = s_cnt[threadIdx.x >> 6];
    for (uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n_chunks; c += gridDim.x * 4) {   // (everything below is uniform over the wave but the lane's nodes)
        const MemberChunk ch = chunks[c];
        const FitSpecies st = tab[ch.species];
        const double *const sw = bit_w + st.bit_base;
        unsigned long long tot[FIT_N] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, orp[3] = {0ull, 0ull, 0ull};
        const uint32_t passes = st.m.route ? st.m.nw : 1u;
        for (uint32_t w = 0; w < passes; ++w) {
            // the bits of word w that stand for a selected haplotype
            const uint32_t left = st.m.route == 2u ? st.m.K - 64u * w : 0u;
            const unsigned long long live = st.m.route == 1u ? st.m.bits : (st.m.route == 2u ? (left >= 64u ? ~0ull : (1ull << left) - 1ull) : 0ull);
#pragma unroll
            for (int q = 0; q < 2 * FIT_N; ++q) cnt[q * 64 + lane] = 0ull;
            member_wave_sync();
            for (uint32_t t0 = 0; t0 < ch.n; t0 += FIT_TILE) {
                uint32_t ln[4];
                unsigned long long bs[4], ex[4], wd[4];
                bool one[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t i = t0 + 64u * j + (uint32_t)lane;
                    const bool on = i < ch.n;
                    const uint32_t v = ch.first + (on ? i : 0u);   // (a dead lane reads the chunk's first node and drops it)
                    ln[j] = node_len[v]; bs[j] = bases[v];
                    unsigned long long word = 0ull;
                    uint32_t m = 0u;
                    double p = 0.0;
                    if (st.m.route == 1u) { word = node_haps[v] & st.m.bits; m = (uint32_t)__popcll(word); p = fit_weights(p, word, sw); }
                    else if (st.m.route == 2u) {
                        const uint64_t row = member_mask_row(st.m, v);
                        for (uint32_t w2 = 0; w2 < st.m.nw; ++w2) {   // every word, in order: the sum runs over all of M(v)
                            const unsigned long long x = mask[row + w2];
                            m += (uint32_t)__popcll(x);
                            p = fit_weights(p, x, sw + 64u * w2);
                            word = w2 == w ? x : word;
                        }
                    }
                    ex[j] = on ? fit_expected(p, ln[j]) : 0ull;
                    wd[j] = on ? word : 0ull;
                    one[j] = m == 1u;
                    if (w == 0u) {   // the species sums see every node once: in the first pass
                        fit_add(tot, on, ln[j], bs[j], ex[j]);
                        const bool o = on & (m == 0u);
                        orp[0] += o ? 1ull : 0ull; orp[1] += o ? (unsigned long long)ln[j] : 0ull; orp[2] += o ? bs[j] : 0ull;
                    }
                }
                const unsigned long long mine = wd[0] | wd[1] | wd[2] | wd[3];
                for (unsigned long long rem = live; rem; rem &= rem - 1ull) {
                    const int b = __builtin_ctzll(rem);
                    if (__builtin_amdgcn_ballot_w64((mine >> b) & 1ull) == 0ull) continue;   // no node of the tile carries the bit
                    unsigned long long a[FIT_N] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, pv[FIT_N] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool has = (wd[j] >> b) & 1ull;
                        fit_add(a, has, ln[j], bs[j], ex[j]);
                        fit_add(pv, has & one[j], ln[j], bs[j], ex[j]);
                    }
#pragma unroll
                    for (int q = 0; q < FIT_N; ++q) { a[q] = fit_wave_sum(a[q]); pv[q] = fit_wave_sum(pv[q]); }
                    if (lane == 0) {
#pragma unroll
                        for (int q = 0; q < FIT_N; ++q) { cnt[q * 64 + b] += a[q]; cnt[(FIT_N + q) * 64 + b] += pv[q]; }
                    }
                }
            }
            member_wave_sync();
            if ((live >> lane) & 1ull) {   // lane b owns bit b of this word
                const uint32_t e = bit_entry[st.bit_base + 64u * w + (uint32_t)lane];
                if (e != MEMBER_NO_ENTRY) {
#pragma unroll
                    for (int q = 0; q < 2 * FIT_N; ++q) {
                        const unsigned long long x = cnt[q * 64 + lane];
                        if (x) atomicAdd(hap_out + (uint64_t)e * (2 * FIT_N) + q, x);
                    }
                }
            }
            member_wave_sync();   // (the counters are zeroed again by the next pass or chunk)
        }
#pragma unroll
        for (int q = 0; q < FIT_N; ++q) tot[q] = fit_wave_sum(tot[q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) orp[q] = fit_wave_sum(orp[q]);
        if (lane == 0) {
            unsigned long long *const o = sp_out + (uint64_t)ch.species * (3 * FIT_N);
            const unsigned long long orphan[FIT_N] = {orp[0], orp[1], orp[2], 0ull, orp[2], 0ull, 0ull, 0ull};   // E = 0 there: excess = bases
#pragma unroll
            for (int q = 0; q < FIT_N; ++q) {
                const unsigned long long explained = tot[q] - orphan[q];
                if (tot[q]) atomicAdd(o + q, tot[q]);
                if (explained) atomicAdd(o + FIT_N + q, explained);
                if (orphan[q]) atomicAdd(o + 2 * FIT_N + q, orphan[q]);
            }
        }
    }
}

}  // namespace

// sel_off [S+1], sel_hap, sel_w validated by the caller (in range, no repeats within a species, weights finite and >= 0)
int fit_launch(Ctx *ctx, Db *db, const uint64_t *sel_off, const uint32_t *sel_hap, const double *sel_w, uint64_t *hap_out, uint64_t *species_out) {
    const uint32_t S = db->S;
    const uint64_t H = db->H, C = sel_off[S];
    if (H + C >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_fit: %llu haplotypes + selection entries exceed 32-bit positions", (unsigned long long)(H + C));
    if (db->V >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_fit: %llu nodes exceed 32-bit positions", (unsigned long long)db->V);
    const bool by_node = member_by_node(db->nh_built, ctx->cfg.fit_route);
    std::vector<FitSpecies> tab(S ? S : 1);
    std::vector<uint32_t> bit_entry(H + C + 1, MEMBER_NO_ENTRY);   // [bit_base of the species + bit] -> selection entry ...
    std::vector<double> bit_w(H + C + 1, 0.0);                     // ... and its weight
    std::vector<MemberChunk> chunks;
    std::vector<uint64_t> ord;
    std::vector<uint32_t> sorted;
    MemberPass ps;
    for (uint32_t s = 0; s < S; ++s) {
        FitSpecies &st = tab[s];
        const uint64_t c0 = sel_off[s], K = sel_off[s + 1] - c0;
        // the species' list in ascending haplotype index: bit order = the order of the sum on both routes; ord[k] = the caller's position of sorted entry k
        ord.resize(K);
        std::iota(ord.begin(), ord.end(), (uint64_t)0);
        std::sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) { return sel_hap[c0 + a] < sel_hap[c0 + b]; });
        sorted.resize(K);
        for (uint64_t k = 0; k < K; ++k) sorted[k] = sel_hap[c0 + ord[k]];
        st.m = ps.wm.row(db, s, by_node, sorted.data(), K);
        st.bit_base = member_bit_base(st.m.route, db->h_hap_off[s], H, c0);
        member_file_bits(st.m.route, sorted.data(), st.m.K, 0, [&](uint64_t bit, uint64_t k) {
            bit_entry[st.bit_base + bit] = (uint32_t)(c0 + ord[k]);
            bit_w[st.bit_base + bit] = sel_w[c0 + ord[k]];
        });
        member_chunks_add(chunks, s, db->h_node_off[s], db->h_node_off[s + 1], FIT_CHUNK, 1);
    }
    const size_t n_hap = (size_t)C * 2 * FIT_N, n_species = (size_t)S * 3 * FIT_N;
    if (n_hap + n_species == 0) return 0;
    DevBuf<FitSpecies> d_tab;
    DevBuf<uint32_t> d_bit_entry;
    DevBuf<double> d_bit_w;
    DevBuf<MemberChunk> d_chunks;
    PTX_TRY(ps.open(ctx, db, n_hap + n_species));   // one device block, zero-filled once: [hap C x 16][species S x 24]
    if (!chunks.empty()) {
        PTX_TRY(upload(ctx, d_tab, tab.data(), tab.size()));
        PTX_TRY(upload(ctx, d_bit_entry, bit_entry.data(), bit_entry.size()));
        PTX_TRY(upload(ctx, d_bit_w, bit_w.data(), bit_w.size()));
        PTX_TRY(upload(ctx, d_chunks, chunks.data(), chunks.size()));
        KTimer tm(ctx, "fit_node_kernel");
        hipLaunchKernelGGL(fit_node_kernel, dim3(grid_for(chunks.size(), 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, (uint32_t)chunks.size(), d_chunks.p, d_tab.p,
                           db->d_node_len.p, db->d_bases.p, by_node ? (const unsigned long long *)db->d_node_haps.p : (const unsigned long long *)nullptr,
                           ps.wm.d_mask.p, d_bit_entry.p, d_bit_w.p, ps.d_out.p, ps.d_out.p + n_hap);
    }
    return ps.close(ctx, hap_out, n_hap, species_out, n_species);
}

}  // namespace ptx
