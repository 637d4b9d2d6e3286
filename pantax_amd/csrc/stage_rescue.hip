// stage_rescue.hip -- read rescue (pantax_hip_strain_read_rescue, the --strain-rescue report): for every read that fits no reported strain, whether a
// single unreported candidate of the db walks all of its nodes, and which one.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Read rescue"): a counted read and Q(r) = (1, #steps, span) are those of the read support pass
// (stage_read_support.hip); Sel_s and Cand_s are those of the near-miss pass.  A species of K_s + J_s <= 64 is open: its row of the table is built over the
// LIST Sel ++ Cand (member_plan.hpp), so a node has ONE u64 on either route -- bit = haplotype index (route 1) or position in the list (route 2) -- and
// the species carries the two masks sel_bits and cand_bits that split it.  Integers only: no order matters.
//
// rescue_kernel walks the locus-grouped step stream as the other read passes do (read_pass_device.hpp: a wave per 64-step group, a lane per step):
//   the word    one seg_and of the step words gives C(r) = a & sel_bits and D(r) = a & cand_bits at the lane of the walk's last step;
//   foreign     one ballot of the lanes with word & sel_bits = 0, novel one of word & (sel_bits | cand_bits) = 0; a deciding lane ANDs each with the
//               lanes [first lane of its walk, its own];
//   steps       foreign_steps, claimed_steps, novel_steps and the candidates' steps are sums over steps, walks of any length alike: per species of the
//               wave's foreign lanes one ballot and popcount each, the candidates through one ballot per candidate bit present on those lanes;
//   counters    counted and compatible take nearly every read: per species of the wave one ballot, two DPP reductions and one 64-bit atomicAdd per
//               non-zero sum from lane 0 (rs_species_rounds, rs_reduce_add).  The rare classes add per lane.  The per-candidate sums go through one ballot per
//               candidate bit present in the D(r) of the species' rescued lanes.
// A walk of more than 64 steps ANDs its per-group partial into its slot's word (rs_long_partial, one word a slot) and ORs its two flags -- a step with
// M empty, a step with M and N empty -- into a per-slot u32; both arrays exist only when the reads hold such walks.  rescue_long_kernel takes a lane per
// slot and classifies and adds the same way.
//
// Algorithmic bytes of rescue_kernel (T' padded steps, R' slots), route 1: those of read_support_kernel in -- 4T' (node ids) + 1T' (step codes) + 8T' (mask
// words) + 16R' (read records) + 8R' (slot records); out: 80 J + 240 S bytes of counters.  Nothing R-sized is allocated but the long-walk partials.
#include <algorithm>
#include "common.hpp"
#include "read_pass_device.hpp"
#include "rescue_plan.hpp"

namespace ptx {

namespace {

constexpr uint32_t RES_LONG_FOREIGN = 1u, RES_LONG_NOVEL = 2u;   // the per-slot flags of a walk of more than 64 steps

struct ResSpecies {
    unsigned long long sel_bits;    // the bits of the species' word that stand for Sel
    unsigned long long cand_bits;   // ... and for Cand
    uint32_t open;                  // 1: K_s + J_s <= 64
    uint32_t pad;
};
struct ResOut {
    unsigned long long *cand;         // [J][3][3]  rescued, alone, from_foreign  x  n_reads, n_steps, span
    unsigned long long *cand_steps;   // [J]
    unsigned long long *sp;           // [S][9][3]
    unsigned long long *step;         // [S][3]     foreign_steps, claimed_steps, novel_steps
};

__device__ __forceinline__ unsigned long long res_wave_or(unsigned long long x) {
    return wave_reduce(x, [](unsigned long long p, unsigned long long q) { return p | q; });
}

// The deciding lanes of the wave -> the counters, species by species: a = the AND of the read's step words, has_f / has_n = the read has a step with M
// empty / with M and N empty.  All 64 lanes call it with everything but the per-lane values uniform.
__device__ __forceinline__ void res_wave_classes(int lane, bool decide, uint32_t sp, const ResSpecies &rs, unsigned long long a, bool has_f, bool has_n,
                                                 uint32_t steps, uint32_t span, const RsSpecies *__restrict__ tab, const uint32_t *__restrict__ bit_entry,
                                                 const ResOut &out) {
    const bool open = decide && rs.open != 0u;
    const unsigned long long c = a & rs.sel_bits, d = a & rs.cand_bits;
    const bool compatible = open && c != 0ull, foreign = open && has_f, mosaic = open && !has_f && c == 0ull;
    const bool rescued = (foreign || mosaic) && d != 0ull;
    rs_species_rounds(decide, sp, [&](uint32_t s0, bool mine, unsigned long long mb) {
        unsigned long long *const so = out.sp + (uint64_t)s0 * (3u * RES_N_CLASSES);
        rs_reduce_add(lane, mine, mb, steps, span, so + 3u * RES_COUNTED);
        const bool comp = mine && compatible;
        const unsigned long long cb = __builtin_amdgcn_ballot_w64(comp);
        if (cb) rs_reduce_add(lane, comp, cb, steps, span, so + 3u * RES_COMPATIBLE);
        // the candidates of the species' rescued lanes: one round per candidate bit present
        const unsigned long long dm = (mine && rescued) ? d : 0ull;
        if (__builtin_amdgcn_ballot_w64(dm != 0ull) == 0ull) return;
        const uint32_t bit_base = tab[s0].bit_base;
        for (unsigned long long q = res_wave_or(dm); q; q &= q - 1ull) {
            const int b = __builtin_ctzll(q);
            const bool has = (dm >> b) & 1ull;
            const unsigned long long hb = __builtin_amdgcn_ballot_w64(has);
            const uint32_t e = bit_entry[bit_base + (uint32_t)b];
            if (e == MEMBER_NO_ENTRY) continue;
            unsigned long long *const co = out.cand + (uint64_t)e * (3u * RES_N_CAND);
            rs_reduce_add(lane, has, hb, steps, span, co + 3u * RES_RESCUED);
            const bool al = has && (dm & (dm - 1ull)) == 0ull, ff = has && foreign;
            const unsigned long long b_al = __builtin_amdgcn_ballot_w64(al), b_ff = __builtin_amdgcn_ballot_w64(ff);
            if (b_al) rs_reduce_add(lane, al, b_al, steps, span, co + 3u * RES_ALONE);
            if (b_ff) rs_reduce_add(lane, ff, b_ff, steps, span, co + 3u * RES_FROM_FOREIGN);
        }
    });
    if (foreign || mosaic) {                                                // the rare classes, per lane
        unsigned long long *const so = out.sp + (uint64_t)sp * (3u * RES_N_CLASSES);
        if (foreign) {
            rs_add3(so + 3u * RES_FOREIGN, 1ull, steps, span);
            rs_add3(so + 3u * (rescued ? RES_FOREIGN_RESCUED : has_n ? RES_FOREIGN_NOVEL : RES_FOREIGN_PATCHWORK), 1ull, steps, span);
        } else {
            rs_add3(so + 3u * RES_MOSAIC, 1ull, steps, span);
            if (rescued) rs_add3(so + 3u * RES_MOSAIC_RESCUED, 1ull, steps, span);
        }
        if (rescued && (d & (d - 1ull)) != 0ull) rs_add3(so + 3u * RES_CONTESTED, 1ull, steps, span);
    }
}

__global__ void __launch_bounds__(256) rescue_kernel(uint32_t n_groups, uint32_t n_slots, const uint32_t *__restrict__ group_slot,
                                                     const uint8_t *__restrict__ step_code, const uint32_t *__restrict__ g_node_id,
                                                     const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec, const RsSpecies *__restrict__ tab,
                                                     const ResSpecies *__restrict__ res, const unsigned long long *__restrict__ node_haps,
                                                     const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ bit_entry,
                                                     unsigned long long *__restrict__ long_acc, uint32_t *__restrict__ long_flag, ResOut out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * 4) {
        const uint32_t gs = group_slot[g];                                   // (wave-uniform) NO_SLOT: a group of pads only
        if (gs == RS_NO_SLOT) continue;
        const RsLane L = rs_lane(g, gs, lane, n_slots, step_code, g_node_id, read_rec, slot_rec, tab);
        ResSpecies rs{0ull, 0ull, 0u, 0u};
        if (L.counted) rs = res[L.sr.x];
        const bool step = L.counted && rs.open != 0u;                        // a step of a counted read of an open species
        const unsigned long long m = step ? rs_word1(L.st, L.v, node_haps, mask) : ~0ull;
        const bool f0 = step && (m & rs.sel_bits) == 0ull, nv = step && (m & (rs.sel_bits | rs.cand_bits)) == 0ull;
        const unsigned long long f_b = __builtin_amdgcn_ballot_w64(f0), n_b = __builtin_amdgcn_ballot_w64(nv);
        const unsigned long long a = seg_and(m, lane, L.seg);
        const unsigned long long walk = rs_lanes(L.seg, lane);              // my walk's lanes in this wave up to mine
        const bool has_f = (f_b & walk) != 0ull, has_n = (n_b & walk) != 0ull;
        // the step counters: per species of the wave's foreign lanes
        rs_species_rounds(f0, L.sr.x, [&](uint32_t s0, bool mine, unsigned long long mb) {
            const unsigned long long nb = __builtin_amdgcn_ballot_w64(mine && nv);
            if (lane == 0) {
                unsigned long long *const xo = out.step + (uint64_t)s0 * 3u;
                const unsigned long long nf = (unsigned long long)__popcll(mb), nn = (unsigned long long)__popcll(nb);
                atomicAdd(xo, nf);
                if (nf - nn) atomicAdd(xo + 1, nf - nn);
                if (nn) atomicAdd(xo + 2, nn);
            }
            const unsigned long long cm = mine ? (m & rs.cand_bits) : 0ull;
            if (mb == nb) return;                                            // no candidate walks any of them
            const uint32_t bit_base = tab[s0].bit_base;
            for (unsigned long long q = res_wave_or(cm); q; q &= q - 1ull) {
                const int b = __builtin_ctzll(q);
                const unsigned long long hb = __builtin_amdgcn_ballot_w64(((cm >> b) & 1ull) != 0ull);
                const uint32_t e = bit_entry[bit_base + (uint32_t)b];
                if (lane == 0 && e != MEMBER_NO_ENTRY) atomicAdd(out.cand_steps + e, (unsigned long long)__popcll(hb));
            }
        });
        // a walk of more than 64 steps: this group's part of its word and of its flags
        if (L.tail && L.is_long && step) {
            rs_long_partial(long_acc, 1u, L.slot, 0u, a);
            const uint32_t fl = (has_f ? RES_LONG_FOREIGN : 0u) | (has_n ? RES_LONG_NOVEL : 0u);
            if (fl) atomicOr(&long_flag[L.slot], fl);
        }
        const bool decide = L.last && L.counted && !L.is_long;
        res_wave_classes(lane, decide, L.sr.x, rs, a, has_f, has_n, L.rr.y, rs_span(L.rr), tab, bit_entry, out);
    }
}

// walks of more than 64 steps: the AND of their per-group partials and the OR of their flags, a lane per slot, the same classes
__global__ void __launch_bounds__(256) rescue_long_kernel(uint32_t n_slots, const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                          const RsSpecies *__restrict__ tab, const ResSpecies *__restrict__ res,
                                                          const unsigned long long *__restrict__ long_acc, const uint32_t *__restrict__ long_flag,
                                                          const uint32_t *__restrict__ bit_entry, ResOut out) {
    const int lane = threadIdx.x & 63;
    for (uint64_t base = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64u; base < n_slots; base += (uint64_t)gridDim.x * 256u) {   // (wave-uniform)
        const RsLongSlot t = rs_long_slot(base, lane, n_slots, read_rec, slot_rec);
        ResSpecies rs{0ull, 0ull, 0u, 0u};
        if (t.decide) rs = res[t.sp];
        unsigned long long a = 0ull;
        uint32_t fl = 0u;
        if (t.decide && rs.open) { a = long_acc[t.s]; fl = long_flag[t.s]; }
        res_wave_classes(lane, t.decide, t.sp, rs, a, (fl & RES_LONG_FOREIGN) != 0u, (fl & RES_LONG_NOVEL) != 0u, t.rr.y, rs_span(t.rr), tab, bit_entry, out);
    }
}

}  // namespace

// both sets validated by the caller (in range, no repeats, disjoint).  species_out [S][9][3], step_out [S][3], cand_out [J][3][3] and cand_steps_out [J] in
// the caller's order of cand_hap
int rescue_launch(Ctx *ctx, Db *db, Reads *rd, const uint64_t *sel_off, const uint32_t *sel_hap, const uint64_t *cand_off, const uint32_t *cand_hap,
                  uint64_t *species_out, uint64_t *step_out, uint64_t *cand_out, uint64_t *cand_steps_out) {
    const uint32_t S = db->S;
    const uint64_t H = db->H, J = cand_off[S];
    // the list Sel ++ Cand of every open species; a skipped species gets an empty one: no masks are built for it
    std::vector<uint64_t> list_off(S + 1, 0), list_entry;
    std::vector<uint32_t> list;
    std::vector<ResSpecies> res(S ? S : 1, ResSpecies{0ull, 0ull, 0u, 0u});
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = sel_off[s + 1] - sel_off[s], Js = cand_off[s + 1] - cand_off[s];
        if (K + Js <= RESCUE_MAX_LIST) {
            res[s].open = 1u;
            list.insert(list.end(), sel_hap + sel_off[s], sel_hap + sel_off[s + 1]);
            list.insert(list.end(), cand_hap + cand_off[s], cand_hap + cand_off[s + 1]);
            list_entry.insert(list_entry.end(), K, (uint64_t)MEMBER_NO_ENTRY);
            for (uint64_t c = cand_off[s]; c < cand_off[s + 1]; ++c) list_entry.push_back(c);
        }
        list_off[s + 1] = list.size();
    }
    const uint64_t Ls = list.size();
    if (H + Ls >= 0xFFFFFFFFull || J >= 0xFFFFFFFFull)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_read_rescue: %llu haplotypes + entries exceed 32-bit positions", (unsigned long long)(H + Ls + J));
    std::vector<uint32_t> bit_entry(H + Ls + 1, MEMBER_NO_ENTRY);
    if (list.empty()) list.push_back(0u);   // (a pointer to hand on)
    RsTable rt;
    rs_table_build(ctx, db, list_off.data(), list.data(), rt, [&](uint64_t at, uint64_t c) { bit_entry[at] = (uint32_t)list_entry[c]; });
    for (uint32_t s = 0; s < S; ++s) {
        if (!res[s].open) continue;
        const uint64_t K = sel_off[s + 1] - sel_off[s], Js = cand_off[s + 1] - cand_off[s];
        const uint32_t route = rt.tab[s].m.route;
        if (route == 1u) { res[s].sel_bits = member_bits(sel_hap + sel_off[s], K); res[s].cand_bits = member_bits(cand_hap + cand_off[s], Js); }
        else if (route == 2u) {
            const unsigned long long all = K + Js >= 64 ? ~0ull : (1ull << (K + Js)) - 1ull;
            res[s].sel_bits = K >= 64 ? ~0ull : (1ull << K) - 1ull;
            res[s].cand_bits = all & ~res[s].sel_bits;
        }
    }
    const size_t n_sp = (size_t)S * 3 * RES_N_CLASSES, n_out = (size_t)J * 10 + n_sp + (size_t)S * 3;
    if (n_out == 0) return 0;
    RsCounters cnt;
    RsLongAcc lng;
    DevBuf<uint32_t> d_bit_entry;
    DevBuf<RsSpecies> d_tab;
    DevBuf<ResSpecies> d_res;
    PTX_TRY(cnt.init(ctx, n_out));
    const ResOut out{cnt.take((size_t)J * 9), cnt.take((size_t)J), cnt.take(n_sp), cnt.take((size_t)S * 3)};
    PTX_TRY(upload(ctx, d_tab, rt.tab.data(), rt.tab.size()));
    PTX_TRY(upload(ctx, d_res, res.data(), res.size()));
    PTX_TRY(upload(ctx, d_bit_entry, bit_entry.data(), bit_entry.size()));
    PTX_TRY(rt.wm.build(ctx, db));
    PTX_TRY(lng.init(ctx, rd, 1u, true));
    rs_launch_groups(ctx, rd, "rescue_kernel", rescue_kernel, d_tab.p, d_res.p, rs_node_haps(rt, db), rt.wm.d_mask.p, d_bit_entry.p, lng.d_acc.p, lng.d_flag.p, out);
    rs_launch_slots(ctx, rd, "rescue_long_kernel", rescue_long_kernel, d_tab.p, d_res.p, lng.d_acc.p, lng.d_flag.p, d_bit_entry.p, out);
    PTX_HIP(ctx, hipGetLastError());
    if (J) PTX_TRY(download(ctx, (unsigned long long *)cand_out, out.cand, (size_t)J * 9));
    if (J) PTX_TRY(download(ctx, (unsigned long long *)cand_steps_out, out.cand_steps, (size_t)J));
    if (S) PTX_TRY(download(ctx, (unsigned long long *)species_out, out.sp, n_sp));
    if (S) PTX_TRY(download(ctx, (unsigned long long *)step_out, out.step, (size_t)S * 3));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    return 0;
}

}  // namespace ptx
