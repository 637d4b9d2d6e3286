// stage_read_support.hip -- per-strain read support (pantax_hip_strain_read_support, the --strain-read-support report): how many reads support every
// candidate strain, how many support it alone, how many fit no candidate, and which candidates the reads cannot tell apart.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Per-strain read support"): a counted read, N(r), C(r) and the assigned strain are those of the per-read strain
// assignment (stage_read_strain.hip).  Q(r) = (1, #steps, span), span = pend - pstart (0 if pend < pstart), all u64.  Per candidate entry the sums of Q over
// the reads with the candidate in C(r) (compatible), with C(r) = {the candidate} (unique), and assigned to it; per species over every counted read
// (counted), over |C(r)| = 0 (unexplained), >= 2 (ambiguous), = K_s (uninformative); per pair of candidates of a species of K_s <= 64 the number of reads
// with both in C(r).  Integers only: no order matters.
//
// read_support_kernel forms C(r) exactly as read_strain_kernel does (read_pass_device.hpp: a wave per 64-step group, a lane per step, the segmented AND on
// the DPP path; the lane of a walk's last step decides), but writes nothing per read: the WAVE reduces.  It takes the species of its first deciding lane
// and handles the deciding lanes of that species, then the next species, until none is left (rs_species_rounds: one or two rounds).  Per round:
//   species sums    n_reads = popcount of a ballot, n_steps and span one DPP wave reduction each; a class no lane falls in is skipped after its ballot;
//   candidate sums  per candidate bit of the species one ballot over the lanes that carry it (none: skipped), then the same for unique and assigned.  Not a
//                   lane per set bit: the lanes of a round share a species and core reads set the same bits, so 64 lanes would queue on K_s counters;
//   pair counts     one ballot + popcount per pair of bits present in the round: at most K_s (K_s - 1) / 2 <= 2016 ballots a round, none when one bit is present.
// Lane 0 issues one 64-bit atomicAdd per non-zero sum.  The pair block is filled in one triangle (either of [a][b], [b][a]); the host mirrors it.
// Species of more than one mask word (route 2 with K_s > 64; they own no pair block) take a plain path: the deciding lane adds once per set bit of C(r).
// Correct, and pinned by the tests; not fast, and not meant to be: such candidate sets do not come out of a strain step.
// Walks of more than 64 steps AND their per-group partials into the per-slot words of the per-read pass (long_nw words a slot, the only per-slot array
// of the call, allocated only when the reads hold such walks); read_support_long_kernel takes a lane per slot and reduces the same way.
//
// Algorithmic bytes of read_support_kernel (T' padded steps, R' slots), route 1:
//   4T' (node ids) + 1T' (step codes) + 8T' (mask words) + 16R' (read records) + 8R' (slot records) in; out: 72 C + 96 S + 8 P bytes of counters.
#include <algorithm>
#include <cmath>
#include "common.hpp"
#include "read_pass_device.hpp"

namespace ptx {

namespace {

struct SupSpecies {
    uint64_t pair_base;   // first entry of the species' K x K block in the pair counts (own_pair)
    uint32_t K;           // candidates
    uint32_t ent0;        // first candidate entry of the species
    uint32_t own_pair;    // 1: K <= 64, the species owns a pair block
    uint32_t pad;
};
struct SupOut {
    unsigned long long *hap;    // [C][3][3]  compatible, unique, assigned  x  n_reads, n_steps, span
    unsigned long long *sp;     // [S][4][3]  counted, unexplained, ambiguous, uninformative
    unsigned long long *pair;   // [P]
};
// what a deciding lane knows of its read
struct SupRead {
    unsigned long long m0;   // word 0 of C(r) (species of one word: all of it)
    uint32_t n;              // |C(r)|
    uint32_t besti;          // bit of the assigned candidate (n > 0)
    uint32_t first;          // lowest bit of C(r) (n > 0)
    double best;
};

// one mask word of C(r), ascending: count, argmax of the weight (the first of equal weights: the smallest haplotype index; a set whose weights are all
// NaN or -inf keeps its lowest bit).  plain: a species of several words -- the lane files the read under every candidate it is compatible with itself.
__device__ __forceinline__ void sup_take(unsigned long long m, uint32_t w, const RsSpecies &st, bool plain, const double *__restrict__ bit_w,
                                         const uint32_t *__restrict__ bit_entry, unsigned long long *__restrict__ hap_out, uint32_t steps, uint32_t span,
                                         SupRead &r) {
    if (w == 0u) r.m0 = m;
    while (m) {
        const uint32_t idx = w * 64u + (uint32_t)__builtin_ctzll(m);
        m &= m - 1ull;
        const double x = bit_w[st.bit_base + idx];
        if (r.n == 0u) { r.first = idx; r.besti = idx; }
        ++r.n;
        if (x > r.best) { r.best = x; r.besti = idx; }
        if (plain) {
            const uint32_t e = bit_entry[st.bit_base + idx];
            if (e != MEMBER_NO_ENTRY) rs_add3(hap_out + (uint64_t)e * 9u, 1ull, steps, span);
        }
    }
}
// plain path, after the last word: unique and assigned
__device__ __forceinline__ void sup_plain_finish(const RsSpecies &st, const uint32_t *__restrict__ bit_entry, unsigned long long *__restrict__ hap_out,
                                                 uint32_t steps, uint32_t span, const SupRead &r) {
    if (r.n == 0u) return;
    if (r.n == 1u) {
        const uint32_t e = bit_entry[st.bit_base + r.first];
        if (e != MEMBER_NO_ENTRY) rs_add3(hap_out + (uint64_t)e * 9u + 3u, 1ull, steps, span);
    }
    const uint32_t e = bit_entry[st.bit_base + r.besti];
    if (e != MEMBER_NO_ENTRY) rs_add3(hap_out + (uint64_t)e * 9u + 6u, 1ull, steps, span);
}

// the deciding lanes of the wave -> the counters, species by species.  All 64 lanes call it with everything but the per-lane values uniform.
__device__ __forceinline__ void sup_wave_reduce(int lane, bool decide, uint32_t sp, const SupRead &r, uint32_t steps, uint32_t span,
                                                const RsSpecies *__restrict__ tab, const SupSpecies *__restrict__ sup, const uint32_t *__restrict__ bit_entry,
                                                const SupOut &out) {
    rs_species_rounds(decide, sp, [&](uint32_t s0, bool mine, unsigned long long mb) {
        const RsSpecies st = tab[s0];
        const SupSpecies su = sup[s0];
        unsigned long long *const so = out.sp + (uint64_t)s0 * 12u;
        rs_reduce_add(lane, mine, mb, steps, span, so);                      // counted
        if (st.m.route == 0u) return;
        {
            const bool un = mine && r.n == 0u, am = mine && r.n >= 2u, ui = mine && r.n == su.K;
            const unsigned long long b_un = __builtin_amdgcn_ballot_w64(un), b_am = __builtin_amdgcn_ballot_w64(am), b_ui = __builtin_amdgcn_ballot_w64(ui);
            if (b_un) rs_reduce_add(lane, un, b_un, steps, span, so + 3);
            if (b_am) rs_reduce_add(lane, am, b_am, steps, span, so + 6);
            if (b_ui) rs_reduce_add(lane, ui, b_ui, steps, span, so + 9);
        }
        if (st.m.nw > 1u) return;                                              // plain path: the lanes have filed their candidates themselves
        const unsigned long long bits = st.m.route == 1u ? st.m.bits : (su.K >= 64u ? ~0ull : (1ull << su.K) - 1ull);
        const unsigned long long mm = mine ? r.m0 : 0ull;
        unsigned long long present = 0ull;
        for (unsigned long long q = bits; q; q &= q - 1ull) {
            const int b = __builtin_ctzll(q);
            const bool has = (mm >> b) & 1ull;
            const unsigned long long cb = __builtin_amdgcn_ballot_w64(has);
            if (cb == 0ull) continue;                                        // no read of the round is compatible with this candidate
            const uint32_t e = bit_entry[st.bit_base + (uint32_t)b];
            if (e == MEMBER_NO_ENTRY) continue;
            present |= 1ull << b;
            unsigned long long *const ho = out.hap + (uint64_t)e * 9u;
            rs_reduce_add(lane, has, cb, steps, span, ho);
            const bool uq = has && r.n == 1u, as = has && r.besti == (uint32_t)b;
            const unsigned long long b_uq = __builtin_amdgcn_ballot_w64(uq), b_as = __builtin_amdgcn_ballot_w64(as);
            if (b_uq) rs_reduce_add(lane, uq, b_uq, steps, span, ho + 3);
            if (b_as) rs_reduce_add(lane, as, b_as, steps, span, ho + 6);
            if (su.own_pair && lane == 0) {
                const uint64_t pa = e - su.ent0;
                atomicAdd(out.pair + su.pair_base + pa * su.K + pa, (unsigned long long)__popcll(cb));
            }
        }
        if (!su.own_pair) return;
        for (unsigned long long qa = present; qa; qa &= qa - 1ull) {
            const int a = __builtin_ctzll(qa);
            for (unsigned long long qb = qa & (qa - 1ull); qb; qb &= qb - 1ull) {
                const int b = __builtin_ctzll(qb);
                const unsigned long long both = __builtin_amdgcn_ballot_w64(((mm >> a) & (mm >> b) & 1ull) != 0ull);
                if (both && lane == 0) {
                    const uint64_t pa = bit_entry[st.bit_base + (uint32_t)a] - su.ent0, pb = bit_entry[st.bit_base + (uint32_t)b] - su.ent0;
                    atomicAdd(out.pair + su.pair_base + pa * su.K + pb, (unsigned long long)__popcll(both));
                }
            }
        }
    });
}

__global__ void __launch_bounds__(256) read_support_kernel(uint32_t n_groups, uint32_t n_slots, const uint32_t *__restrict__ group_slot,
                                                           const uint8_t *__restrict__ step_code, const uint32_t *__restrict__ g_node_id,
                                                           const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                           const RsSpecies *__restrict__ tab, const SupSpecies *__restrict__ sup,
                                                           const unsigned long long *__restrict__ node_haps, const unsigned long long *__restrict__ mask,
                                                           const double *__restrict__ bit_w, const uint32_t *__restrict__ bit_entry,
                                                           unsigned long long *__restrict__ long_acc, uint32_t long_nw, SupOut out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * 4) {
        const uint32_t gs = group_slot[g];                                   // (wave-uniform) NO_SLOT: a group of pads only
        if (gs == RS_NO_SLOT) continue;
        const RsLane L = rs_lane(g, gs, lane, n_slots, step_code, g_node_id, read_rec, slot_rec, tab);
        const uint32_t nw_max = wave_reduce(L.nw, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
        const bool decide = L.last && L.counted && !L.is_long;
        const uint32_t steps = L.rr.y, span = rs_span(L.rr);
        SupRead r{0ull, 0u, 0u, 0u, -INFINITY};
        for (uint32_t w = 0; w < nw_max; ++w) {                              // (wave-uniform trip count: seg_and wants every lane)
            const unsigned long long m = rs_lane_word(L, w, lane, node_haps, mask);
            if (L.tail && w < L.nw) {
                if (L.is_long) rs_long_partial(long_acc, long_nw, L.slot, w, m);
                else if (L.last) sup_take(m, w, L.st, L.nw > 1u, bit_w, bit_entry, out.hap, steps, span, r);
            }
        }
        if (decide && L.nw > 1u) sup_plain_finish(L.st, bit_entry, out.hap, steps, span, r);
        sup_wave_reduce(lane, decide, L.sr.x, r, steps, span, tab, sup, bit_entry, out);
    }
}

// walks of more than 64 steps: the AND of their per-group partials, a lane per slot, the same reduction
__global__ void __launch_bounds__(256) read_support_long_kernel(uint32_t n_slots, const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                                const RsSpecies *__restrict__ tab, const SupSpecies *__restrict__ sup,
                                                                const unsigned long long *__restrict__ long_acc, uint32_t long_nw,
                                                                const double *__restrict__ bit_w, const uint32_t *__restrict__ bit_entry, SupOut out) {
    const int lane = threadIdx.x & 63;
    for (uint64_t base = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64u; base < n_slots; base += (uint64_t)gridDim.x * 256u) {   // (wave-uniform)
        const RsLongSlot t = rs_long_slot(base, lane, n_slots, read_rec, slot_rec);
        RsSpecies st{};
        if (t.decide) st = tab[t.sp];
        const uint32_t nw = st.m.route ? st.m.nw : 0u;
        const uint32_t steps = t.rr.y, span = rs_span(t.rr);
        SupRead r{0ull, 0u, 0u, 0u, -INFINITY};
        for (uint32_t w = 0; w < nw; ++w) sup_take(long_acc[t.s * long_nw + w], w, st, nw > 1u, bit_w, bit_entry, out.hap, steps, span, r);
        if (t.decide && nw > 1u) sup_plain_finish(st, bit_entry, out.hap, steps, span, r);
        sup_wave_reduce(lane, t.decide, t.sp, r, steps, span, tab, sup, bit_entry, out);
    }
}

}  // namespace

// the candidates of every species in ascending haplotype order (cand_hap, cand_w), entry_of[c] = the caller's entry of sorted candidate c; pair_off [S+1]
// as the caller gets it; every array validated by the caller.  hap_out [C][3][3] in the caller's order, species_out [S][4][3], pair_out [pair_off[S]].
int read_support_launch(Ctx *ctx, Db *db, Reads *rd, const uint64_t *cand_off, const uint32_t *cand_hap, const double *cand_w, const uint64_t *entry_of,
                        const uint64_t *pair_off, uint64_t *hap_out, uint64_t *species_out, uint64_t *pair_out) {
    const uint32_t S = db->S;
    const uint64_t H = db->H, C = cand_off[S], P = pair_off[S];
    PTX_TRY(rs_check_bits(ctx, "strain_read_support", H, C));
    std::vector<double> bit_w(H + C + 1, 0.0);
    std::vector<uint32_t> bit_entry(H + C + 1, MEMBER_NO_ENTRY);
    RsTable rt;
    rs_table_build(ctx, db, cand_off, cand_hap, rt, [&](uint64_t at, uint64_t c) { bit_w[at] = cand_w[c]; bit_entry[at] = (uint32_t)entry_of[c]; });
    std::vector<SupSpecies> sup(S ? S : 1, SupSpecies{0ull, 0u, 0u, 0u, 0u});
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = cand_off[s + 1] - cand_off[s];
        sup[s] = SupSpecies{pair_off[s], (uint32_t)K, (uint32_t)cand_off[s], (K >= 1 && K <= 64) ? 1u : 0u, 0u};
    }
    const size_t n_out = (size_t)C * 9 + (size_t)S * 12 + (size_t)P;
    if (n_out == 0) return 0;
    RsCounters cnt;
    RsLongAcc lng;
    DevBuf<RsSpecies> d_tab;
    DevBuf<SupSpecies> d_sup;
    DevBuf<double> d_bit_w;
    DevBuf<uint32_t> d_bit_entry;
    PTX_TRY(cnt.init(ctx, n_out));
    const SupOut out{cnt.take((size_t)C * 9), cnt.take((size_t)S * 12), cnt.take((size_t)P)};
    PTX_TRY(upload(ctx, d_tab, rt.tab.data(), rt.tab.size()));
    PTX_TRY(upload(ctx, d_sup, sup.data(), sup.size()));
    PTX_TRY(upload(ctx, d_bit_w, bit_w.data(), bit_w.size()));
    PTX_TRY(upload(ctx, d_bit_entry, bit_entry.data(), bit_entry.size()));
    PTX_TRY(rt.wm.build(ctx, db));
    PTX_TRY(lng.init(ctx, rd, rt.long_nw));
    rs_launch_groups(ctx, rd, "read_support_kernel", read_support_kernel, d_tab.p, d_sup.p, rs_node_haps(rt, db), rt.wm.d_mask.p, d_bit_w.p, d_bit_entry.p,
                     lng.d_acc.p, rt.long_nw, out);
    rs_launch_slots(ctx, rd, "read_support_long_kernel", read_support_long_kernel, d_tab.p, d_sup.p, lng.d_acc.p, rt.long_nw, d_bit_w.p, d_bit_entry.p, out);
    PTX_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> h_pair(P ? P : 1);
    if (C) PTX_TRY(download(ctx, (unsigned long long *)hap_out, out.hap, (size_t)C * 9));
    if (S) PTX_TRY(download(ctx, (unsigned long long *)species_out, out.sp, (size_t)S * 12));
    if (P) PTX_TRY(download(ctx, h_pair.data(), out.pair, (size_t)P));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    // the device filled one of [a][b], [b][a] of every pair: mirror
    for (uint32_t s = 0; s < S && P; ++s) {
        if (!sup[s].own_pair) continue;
        const uint64_t K = sup[s].K;
        const unsigned long long *src = h_pair.data() + pair_off[s];
        uint64_t *dst = pair_out + pair_off[s];
        for (uint64_t a = 0; a < K; ++a)
            for (uint64_t b = 0; b < K; ++b) dst[a * K + b] = a == b ? src[a * K + a] : src[a * K + b] + src[b * K + a];
    }
    return 0;
}

}  // namespace ptx
