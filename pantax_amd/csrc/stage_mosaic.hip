// stage_mosaic.hip -- mosaic reads (pantax_hip_strain_mosaic, the --strain-mosaic report): a read that fits no single candidate strain is cut into the
// fewest stretches that each fit one, and the strains it switches between and the places where it switches are counted.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Mosaic reads"): a counted read, Q(r) = (1, #steps, span) and the argmax rule are those of the read support
// pass (stage_read_support.hip).  M(v) = the candidates of the species that walk node v, one u64 (species of 1 <= K_s <= 64).  A read with an empty M(v) is
// foreign; every other read is cut greedily from the left: a segment grows while the AND of its steps' M stays non-zero.  Integers only: no order matters.
//
// mosaic_kernel walks the locus-grouped step stream as the other read passes do (read_pass_device.hpp: a wave per 64-step group, a lane per step).
// Walks of at most 64 steps lie inside their group:
//   foreign     one ballot of the lanes with M = 0; a lane ANDs it with its walk's lanes.  Foreign walks leave the cut (their lanes carry all ones);
//   cut         rounds of the segmented AND (seg_and).  After a round the first lane of a walk whose prefix is zero is a break: the lowest bit of the ballot
//               of zero lanes inside [my segment's first lane, my walk's last lane].  The lanes of the walk at and behind it move their segment's first lane
//               up to it and the AND is formed again; a round finds one break per walk of the wave, so the loop is wave-uniform and ends after the largest
//               k of the wave.  A wave without a mosaic read -- nearly every wave -- takes one round;
//   segments    the lane ahead of a break and the lane of the walk's last step hold A_j and take the argmax; a break lane fetches the strain of the left
//               segment from the lane below and the strain of its own segment from that segment's last lane (the ballot of such lanes, ctz at and above
//               the own lane), both through ds_bpermute;
//   counters    counted and compatible take nearly every read: per species of the wave one ballot, two DPP reductions and one 64-bit atomicAdd per
//               non-zero sum from lane 0 (rs_species_rounds, rs_reduce_add).  The rare classes (mosaic, foreign), the per-candidate segments, the switches and
//               the junction records add per lane; the break lanes of a wave share one returning atomic on the break counter.
// A walk of more than 64 steps cannot be cut group by group in any order: the cut is sequential.  The wave that meets its first step takes the whole
// walk: a pass over its groups for the foreign steps, then chunk by chunk the words into the lanes and a wave-uniform loop over the chunk's lanes that
// carries the running word, the open segment's steps and the left strain from chunk to chunk.  Waves that meet a later group of the walk skip its lanes.
//
// Algorithmic bytes of mosaic_kernel (T' padded steps, R' slots), route 1: those of read_support_kernel in -- 4T' (node ids) + 1T' (step codes) + 8T' (mask
// words) + 16R' (read records) + 8R' (slot records); out: 16 C + 168 S + 8 P bytes of counters and 12 bytes per break.  Nothing R-sized is allocated.
#include <algorithm>
#include <cmath>
#include "common.hpp"
#include "mosaic_plan.hpp"
#include "read_pass_device.hpp"

namespace ptx {

namespace {

struct MosSpecies {
    uint64_t pair_base;   // first entry of the species' K x K block of the switch counts
    uint32_t K;           // candidates
    uint32_t ent0;        // first candidate entry of the species
};
struct MosOut {
    unsigned long long *hap;        // [C][2]     segments, steps
    unsigned long long *sp;         // [S][6][3]  MosaicClass x {n_reads, n_steps, span}
    unsigned long long *extra;      // [S][3]     n_segments, n_breaks, foreign_steps
    unsigned long long *pair;       // [P]
    unsigned long long *n_breaks;   // [1]        the breaks of the call: the next place in `junction`
    uint32_t *junction;             // [cap][3]   species, node_a, node_b (species-local); null when cap = 0
    unsigned long long cap;
};

// the candidate entry a segment with the non-zero word `a` is assigned: bits ascend with the haplotype index, the first of equal weights wins (a set whose
// weights are all NaN or -inf keeps its lowest bit)
__device__ __forceinline__ uint32_t mos_assigned(unsigned long long a, const RsSpecies &st, const double *__restrict__ bit_w, const uint32_t *__restrict__ bit_entry) {
    uint32_t besti = (uint32_t)__builtin_ctzll(a);
    double best = -INFINITY;
    while (a) {
        const uint32_t idx = (uint32_t)__builtin_ctzll(a);
        a &= a - 1ull;
        const double x = bit_w[st.bit_base + idx];
        if (x > best) { best = x; besti = idx; }
    }
    return bit_entry[st.bit_base + besti];
}
__device__ __forceinline__ bool mos_served(const RsSpecies &st) { return st.m.route != 0u && st.m.nw == 1u; }   // 1 <= K_s <= 64
__device__ __forceinline__ void mos_file_junction(const MosOut &out, unsigned long long at, uint32_t species, uint32_t node_a, uint32_t node_b) {
    if (at >= out.cap) return;   // (cap = 0: not collected; beyond the cap the counter goes on counting and nothing is written)
    uint32_t *const j = out.junction + at * 3ull;
    j[0] = species; j[1] = node_a; j[2] = node_b;
}
__device__ __forceinline__ void mos_add_switch(const MosOut &out, const MosSpecies &ms, uint32_t e_left, uint32_t e_right) {
    if (e_left == MEMBER_NO_ENTRY || e_right == MEMBER_NO_ENTRY) return;
    atomicAdd(out.pair + ms.pair_base + (uint64_t)(e_left - ms.ent0) * ms.K + (e_right - ms.ent0), 1ull);
}
__device__ __forceinline__ void mos_add_segment(const MosOut &out, uint32_t e, uint32_t steps) {
    if (e == MEMBER_NO_ENTRY) return;
    atomicAdd(out.hap + (uint64_t)e * 2u, 1ull);
    atomicAdd(out.hap + (uint64_t)e * 2u + 1u, (unsigned long long)steps);
}

// A walk of more than 64 steps whose first step is lane l0 of the group the wave holds: the whole walk, sequentially.  Every value but the chunk's words
// and nodes is wave-uniform; lane 0 adds.
__device__ __forceinline__ void mos_long_walk(int lane, int l0, const RsLane &L, const uint32_t *__restrict__ g_node_id, const RsSpecies *__restrict__ tab,
                                              const MosSpecies *__restrict__ mos, const unsigned long long *__restrict__ node_haps,
                                              const unsigned long long *__restrict__ mask, const double *__restrict__ bit_w,
                                              const uint32_t *__restrict__ bit_entry, const MosOut &out) {
    const uint4 rr = make_uint4(lane_get(L.rr.x, l0), lane_get(L.rr.y, l0), lane_get(L.rr.z, l0), lane_get(L.rr.w, l0));
    const uint32_t sp = lane_get(L.sr.x, l0), node_off = lane_get(L.sr.y, l0);
    if ((int32_t)sp < 0) return;                                              // not counted
    const RsSpecies st = tab[sp];
    const uint32_t steps = rr.y, span = rs_span(rr);
    unsigned long long *const so = out.sp + (uint64_t)sp * (3u * MOS_N_CLASSES);
    if (lane == 0) rs_add3(so + 3u * MOS_COUNTED, 1ull, steps, span);
    if (!mos_served(st)) return;
    const uint64_t t0 = rr.x, t1 = (uint64_t)rr.x + rr.y;
    unsigned long long foreign_steps = 0;
    for (uint64_t base = t0 & ~63ull; base < t1; base += 64u) {              // (wave-uniform)
        const uint64_t t = base + (uint64_t)lane;
        const bool in = t >= t0 && t < t1;
        const unsigned long long m = in ? rs_word1(st, g_node_id[t] + node_off, node_haps, mask) : ~0ull;
        foreign_steps += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(in && m == 0ull));
    }
    if (foreign_steps) {
        if (lane == 0) { rs_add3(so + 3u * MOS_FOREIGN, 1ull, steps, span); atomicAdd(out.extra + (uint64_t)sp * 3u + 2u, foreign_steps); }
        return;
    }
    const MosSpecies ms = mos[sp];
    unsigned long long run = ~0ull, k = 1;
    uint32_t run_steps = 0, e_left = MEMBER_NO_ENTRY, v_prev = 0;
    bool have_left = false;
    for (uint64_t base = t0 & ~63ull; base < t1; base += 64u) {
        const uint64_t t = base + (uint64_t)lane;
        const bool in = t >= t0 && t < t1;
        const uint32_t v = in ? g_node_id[t] + node_off : 0u;
        const unsigned long long m = in ? rs_word1(st, v, node_haps, mask) : ~0ull;
        const int lo = base < t0 ? (int)(t0 - base) : 0, hi = t1 - base < 64u ? (int)(t1 - base) : 64;
        for (int l = lo; l < hi; ++l) {                                       // (wave-uniform)
            const unsigned long long ml = lane_get(m, l);
            const uint32_t vl = lane_get(v, l);
            if ((run & ml) == 0ull) {                                         // this step would empty the open segment: it opens the next one
                const uint32_t e = mos_assigned(run, st, bit_w, bit_entry);
                if (lane == 0) {
                    mos_add_segment(out, e, run_steps);
                    if (have_left) mos_add_switch(out, ms, e_left, e);
                    mos_file_junction(out, atomicAdd(out.n_breaks, 1ull), sp, v_prev - st.m.node_base, vl - st.m.node_base);
                }
                e_left = e; have_left = true;
                run = ml; run_steps = 1; ++k;
            } else { run &= ml; ++run_steps; }
            v_prev = vl;
        }
    }
    if (lane != 0) return;
    rs_add3(so + 3u * mosaic_class_of(k), 1ull, steps, span);
    if (k < 2) return;
    const uint32_t e = mos_assigned(run, st, bit_w, bit_entry);
    mos_add_segment(out, e, run_steps);
    mos_add_switch(out, ms, e_left, e);
    atomicAdd(out.extra + (uint64_t)sp * 3u, k);
    atomicAdd(out.extra + (uint64_t)sp * 3u + 1u, k - 1ull);
}

__global__ void __launch_bounds__(256) mosaic_kernel(uint32_t n_groups, uint32_t n_slots, const uint32_t *__restrict__ group_slot,
                                                     const uint8_t *__restrict__ step_code, const uint32_t *__restrict__ g_node_id,
                                                     const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec, const RsSpecies *__restrict__ tab,
                                                     const MosSpecies *__restrict__ mos, const unsigned long long *__restrict__ node_haps,
                                                     const unsigned long long *__restrict__ mask, const double *__restrict__ bit_w,
                                                     const uint32_t *__restrict__ bit_entry, MosOut out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * 4) {
        const uint32_t gs = group_slot[g];                                   // (wave-uniform) NO_SLOT: a group of pads only
        if (gs == RS_NO_SLOT) continue;
        const RsLane L = rs_lane(g, gs, lane, n_slots, step_code, g_node_id, read_rec, slot_rec, tab);
        const bool served = L.counted && mos_served(L.st);
        const bool cut = served && !L.is_long;                               // a step of a walk that lies inside this group
        const bool decide = L.last && L.counted && !L.is_long;
        const uint32_t steps = L.rr.y, span = rs_span(L.rr);
        const int end = cut ? min(L.seg + (int)L.rr.y - 1, 63) : lane;       // my walk's last lane (the layout keeps such a walk inside its group)
        const unsigned long long walk = rs_lanes(L.seg, end);
        const unsigned long long m = cut ? rs_word1(L.st, L.v, node_haps, mask) : ~0ull;
        // foreign walks are voted out before the first round
        const unsigned long long fz = __builtin_amdgcn_ballot_w64(cut && m == 0ull) & walk;
        const bool foreign = cut && fz != 0ull, active = cut && !foreign;
        const unsigned long long word = active ? m : ~0ull;
        int seg = L.seg;                                                     // first lane of my segment
        unsigned long long a;
        for (;;) {                                                           // (wave-uniform: a round finds one break per walk)
            a = seg_and(word, lane, seg);
            const unsigned long long zero = __builtin_amdgcn_ballot_w64(active && a == 0ull);
            if (zero == 0ull) break;
            const unsigned long long mine = zero & rs_lanes(seg, 63) & walk; // (the lanes of my segment read non-zero below its first zero lane)
            if (active && mine) { const int b = __builtin_ctzll(mine); if (lane >= b) seg = b; }
        }
        const bool brk = active && seg != L.seg && lane == seg;              // the first step of a segment that is not the walk's first
        const unsigned long long brk_b = __builtin_amdgcn_ballot_w64(brk);
        const uint32_t k = 1u + (uint32_t)__popcll(brk_b & walk);
        const bool mosaic = active && k >= 2u;
        const bool seg_end = mosaic && (L.last || (lane < 63 && ((brk_b >> (lane + 1)) & 1ull) != 0ull));
        const unsigned long long end_b = __builtin_amdgcn_ballot_w64(seg_end);
        uint32_t e = MEMBER_NO_ENTRY;
        if (seg_end) { e = mos_assigned(a, L.st, bit_w, bit_entry); mos_add_segment(out, e, (uint32_t)(lane - seg) + 1u); }
        if (brk_b) {                                                         // (wave-uniform)
            const int my_end = brk ? __builtin_ctzll(end_b & rs_lanes(lane, 63)) : lane;
            const uint32_t e_left = (uint32_t)__shfl((int)e, (lane + 63) & 63), e_right = (uint32_t)__shfl((int)e, my_end);
            const uint32_t v_left = (uint32_t)__shfl((int)L.v, (lane + 63) & 63);
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(out.n_breaks, (unsigned long long)__popcll(brk_b));   // one returning atomic for the wave's break lanes
            base = lane_get(base, 0);
            if (brk) {
                mos_add_switch(out, mos[L.sr.x], e_left, e_right);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(brk_b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)brk_b, 0u));
                mos_file_junction(out, base + rank, L.sr.x, v_left - L.st.m.node_base, L.v - L.st.m.node_base);
            }
        }
        // the classes: counted and compatible per species of the wave, the rare ones per lane
        rs_species_rounds(decide, L.sr.x, [&](uint32_t s0, bool mine, unsigned long long mb) {
            unsigned long long *const so = out.sp + (uint64_t)s0 * (3u * MOS_N_CLASSES);
            rs_reduce_add(lane, mine, mb, steps, span, so + 3u * MOS_COUNTED);
            const bool comp = mine && active && k == 1u;
            const unsigned long long cb = __builtin_amdgcn_ballot_w64(comp);
            if (cb) rs_reduce_add(lane, comp, cb, steps, span, so + 3u * MOS_COMPATIBLE);
        });
        if (decide && (foreign || mosaic)) {
            unsigned long long *const so = out.sp + (uint64_t)L.sr.x * (3u * MOS_N_CLASSES);
            unsigned long long *const ex = out.extra + (uint64_t)L.sr.x * 3u;
            if (foreign) { rs_add3(so + 3u * MOS_FOREIGN, 1ull, steps, span); atomicAdd(ex + 2, (unsigned long long)__popcll(fz)); }
            else { rs_add3(so + 3u * mosaic_class_of(k), 1ull, steps, span); atomicAdd(ex, (unsigned long long)k); atomicAdd(ex + 1, (unsigned long long)(k - 1u)); }
        }
        // a walk of more than 64 steps begins in this group (at most one does: it fills the group's remaining lanes): this wave takes all of it
        const unsigned long long long_b = __builtin_amdgcn_ballot_w64(L.live && L.is_long && (uint32_t)((uint64_t)g * 64u + (uint64_t)lane) == L.rr.x);
        if (long_b) mos_long_walk(lane, __builtin_ctzll(long_b), L, g_node_id, tab, mos, node_haps, mask, bit_w, bit_entry, out);
    }
}

}  // namespace

// the candidates of every species in ascending haplotype order (cand_hap, cand_w), entry_of[c] = the caller's entry of sorted candidate c; pair_off [S+1]
// as the caller gets it; every array validated by the caller.  species_out [S][6][3], extra_out [S][3], hap_out [C][2] in the caller's order, pair_out
// [pair_off[S]]; junction_cap = 0: nothing is allocated for junctions.  More breaks than a non-zero junction_cap: E_LIMIT with only *n_breaks_total_out written
int mosaic_launch(Ctx *ctx, Db *db, Reads *rd, const uint64_t *cand_off, const uint32_t *cand_hap, const double *cand_w, const uint64_t *entry_of,
                  const uint64_t *pair_off, uint64_t *species_out, uint64_t *extra_out, uint64_t *hap_out, uint64_t *pair_out, uint64_t junction_cap,
                  uint32_t *junction_out, uint64_t *junction_count_out, uint64_t *n_junctions_out, uint64_t *n_breaks_total_out) {
    const uint32_t S = db->S;
    const uint64_t H = db->H, C = cand_off[S], P = pair_off[S];
    PTX_TRY(rs_check_bits(ctx, "strain_mosaic", H, C));
    std::vector<double> bit_w(H + C + 1, 0.0);
    std::vector<uint32_t> bit_entry(H + C + 1, MEMBER_NO_ENTRY);
    RsTable rt;
    rs_table_build(ctx, db, cand_off, cand_hap, rt, [&](uint64_t at, uint64_t c) { bit_w[at] = cand_w[c]; bit_entry[at] = (uint32_t)entry_of[c]; });
    std::vector<MosSpecies> mos(S ? S : 1, MosSpecies{0ull, 0u, 0u});
    for (uint32_t s = 0; s < S; ++s) mos[s] = MosSpecies{pair_off[s], (uint32_t)(cand_off[s + 1] - cand_off[s]), (uint32_t)cand_off[s]};
    const size_t n_sp = (size_t)S * 3 * MOS_N_CLASSES;
    RsCounters cnt;
    DevBuf<uint32_t> d_junction, d_bit_entry;
    DevBuf<RsSpecies> d_tab;
    DevBuf<MosSpecies> d_mos;
    DevBuf<double> d_bit_w;
    PTX_TRY(cnt.init(ctx, (size_t)C * 2 + n_sp + (size_t)S * 3 + (size_t)P + 1));
    const uint64_t rec_cap = std::min<uint64_t>(junction_cap, rd->T_pad);   // (a break is a step of the stream: there are fewer than T_pad)
    if (rec_cap) PTX_HIP(ctx, d_junction.alloc((size_t)rec_cap * 3));
    PTX_TRY(upload(ctx, d_tab, rt.tab.data(), rt.tab.size()));
    PTX_TRY(upload(ctx, d_mos, mos.data(), mos.size()));
    PTX_TRY(upload(ctx, d_bit_w, bit_w.data(), bit_w.size()));
    PTX_TRY(upload(ctx, d_bit_entry, bit_entry.data(), bit_entry.size()));
    PTX_TRY(rt.wm.build(ctx, db));
    const MosOut out{cnt.take((size_t)C * 2), cnt.take(n_sp), cnt.take((size_t)S * 3), cnt.take((size_t)P), cnt.take(1), rec_cap ? d_junction.p : nullptr, rec_cap};
    rs_launch_groups(ctx, rd, "mosaic_kernel", mosaic_kernel, d_tab.p, d_mos.p, rs_node_haps(rt, db), rt.wm.d_mask.p, d_bit_w.p, d_bit_entry.p, out);
    PTX_HIP(ctx, hipGetLastError());
    unsigned long long n_breaks = 0;
    PTX_TRY(download(ctx, &n_breaks, out.n_breaks, 1));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_breaks_total_out = n_breaks;
    if (junction_cap && n_breaks > junction_cap)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_mosaic: %llu breaks, the caller's junction arrays hold %llu", n_breaks, (unsigned long long)junction_cap);
    std::vector<MosaicBreak> recs(junction_cap ? (size_t)n_breaks : 0);
    static_assert(sizeof(MosaicBreak) == 3 * sizeof(uint32_t), "a break record is three u32");
    if (C) PTX_TRY(download(ctx, (unsigned long long *)hap_out, out.hap, (size_t)C * 2));
    if (S) PTX_TRY(download(ctx, (unsigned long long *)species_out, out.sp, n_sp));
    if (S) PTX_TRY(download(ctx, (unsigned long long *)extra_out, out.extra, (size_t)S * 3));
    if (P) PTX_TRY(download(ctx, (unsigned long long *)pair_out, out.pair, (size_t)P));
    if (!recs.empty()) PTX_TRY(download(ctx, reinterpret_cast<uint32_t *>(recs.data()), d_junction.p, recs.size() * 3));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    std::vector<MosaicBreak> distinct;
    std::vector<uint64_t> count;
    mosaic_junctions(recs, distinct, count);
    for (size_t i = 0; i < distinct.size(); ++i) {
        junction_out[3 * i] = distinct[i].species; junction_out[3 * i + 1] = distinct[i].node_a; junction_out[3 * i + 2] = distinct[i].node_b;
        junction_count_out[i] = count[i];
    }
    *n_junctions_out = distinct.size();
    return 0;
}

}  // namespace ptx
