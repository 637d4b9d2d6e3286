// read_strain_device.hpp -- what the two passes over the locus-grouped step stream that form the per-read candidate mask C(r) share
// (stage_read_strain.hip: the per-read assignment; stage_read_support.hip: the per-strain read support): the species table (member_plan.hpp), the
// slot lookup, the segmented AND over the lanes of a wave, a lane's view of its step, and the per-slot partials of walks of more than 64 steps.
// Device code and the host code that feeds it; include from .hip files only.
#pragma once
#include <algorithm>
#include <vector>
#include "common.hpp"
#include "member_device.hpp"

namespace ptx {

constexpr uint32_t RS_NO_SLOT = 0xFFFFFFFFu;
// step codes of the grouped stream (cov_device.hpp: STEP_PAD, STEP_START)
constexpr uint32_t RS_STEP_PAD = 0xFFu, RS_STEP_START = 0x40u;

struct RsSpecies { MemberRow m; uint32_t bit_base; };   // bit_base: first entry of the species in the per-bit arrays (bit_w / bit_hap, bit_w / bit_entry)

// slot of the step held by `lane` (all 64 lanes): group_first_slot owns the group's first step, every later walk start advances it
__device__ __forceinline__ uint32_t rs_slot_in_group(uint32_t group_first_slot, uint32_t code, int lane) {
    const unsigned long long starts = __builtin_amdgcn_ballot_w64((code != RS_STEP_PAD) & ((code & RS_STEP_START) != 0u)) & ~1ull;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(starts >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)starts, 0u));
    return group_first_slot + below + (uint32_t)((starts >> lane) & 1ull);
}

// DPP move whose invalid / masked-off lanes read all ones (the identity of AND)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_ones(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFF, (int)v, CTRL, ROW_MASK, 0xF, false); }

// inclusive AND over lanes [seg, lane] (seg <= lane: the first lane of my walk in this wave); all 64 lanes active.  The steps of
// wave_incl_scan_dpp: row_shr 1/2/4/8 inside the 16-lane rows, then the row results travel by row_bcast:15 and row_bcast:31; a lane
// takes a value only from a source lane of its own walk.
__device__ __forceinline__ unsigned long long seg_and(unsigned long long m, int lane, int seg) {
    uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
#define RS_STEP(CTRL, RM, SRC)                                                  \
    {                                                                           \
        const uint32_t tl = dpp_ones<CTRL, RM>(lo), th = dpp_ones<CTRL, RM>(hi); \
        if ((SRC) >= seg) { lo &= tl; hi &= th; }                               \
    }
    RS_STEP(0x111, 0xF, lane - 1)
    RS_STEP(0x112, 0xF, lane - 2)
    RS_STEP(0x114, 0xF, lane - 4)
    RS_STEP(0x118, 0xF, lane - 8)
    RS_STEP(0x142, 0xA, (lane & ~15) - 1)   // rows 1 and 3 <- lanes 15 and 47
    RS_STEP(0x143, 0xC, 31)                 // rows 2 and 3 <- lane 31
#undef RS_STEP
    return ((unsigned long long)hi << 32) | lo;
}

// a lane's step of a live 64-step group: its slot and the slot's records, its species' row of the table, where it stands in its walk
struct RsLane {
    uint4 rr;            // read record {walk's place in the stream, #steps, pstart, pend}
    uint2 sr;            // slot record {species (coded), node base - first node id of the species}
    RsSpecies st;        // the species' row (zeros unless counted)
    uint64_t mrow;       // route 2: first mask word of my node
    uint32_t slot, nw, v;   // nw: mask words of my species (0: not counted / no candidates); v: global node index
    int seg;             // first lane of my walk in this wave
    bool live, counted, last, is_long, tail;   // tail: last step of my walk in this wave
};
__device__ __forceinline__ RsLane rs_lane(uint32_t g, uint32_t gs, int lane, uint32_t n_slots, const uint8_t *__restrict__ step_code,
                                          const uint32_t *__restrict__ g_node_id, const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                          const RsSpecies *__restrict__ tab) {
    RsLane L;
    const uint64_t t = (uint64_t)g * 64u + (uint64_t)lane;
    const uint32_t code = step_code[t];
    L.slot = rs_slot_in_group(gs, code, lane);
    L.live = code != RS_STEP_PAD && L.slot < n_slots;
    L.rr = make_uint4(0u, 0u, 0u, 0u);
    L.sr = make_uint2(0xFFFFFFFFu, 0u);
    if (L.live) { L.rr = read_rec[L.slot]; L.sr = slot_rec[L.slot]; }
    L.counted = L.live && (int32_t)L.sr.x >= 0;
    L.st = RsSpecies{};
    if (L.counted) L.st = tab[L.sr.x];
    const uint32_t i = L.live ? (uint32_t)t - L.rr.x : 0u;                // position in the walk (T_pad < 2^32)
    L.last = L.live && i + 1u == L.rr.y;
    L.is_long = L.rr.y > 64u;
    L.seg = lane - (int)min(i, (uint32_t)lane);
    L.tail = L.live && (L.last || lane == 63);
    L.nw = L.st.m.route ? L.st.m.nw : 0u;
    L.v = L.counted ? g_node_id[t] + L.sr.y : 0u;
    L.mrow = member_mask_row(L.st.m, L.v);
    return L;
}
// word w of the AND over my walk's steps in this wave, up to and including mine (all 64 lanes call it: a wave-uniform trip count over w)
__device__ __forceinline__ unsigned long long rs_lane_word(const RsLane &L, uint32_t w, int lane, const unsigned long long *__restrict__ node_haps,
                                                           const unsigned long long *__restrict__ mask) {
    unsigned long long m = ~0ull;
    if (w < L.nw) m = L.st.m.route == 1u ? (node_haps[L.v] & L.st.m.bits) : mask[L.mrow + w];
    return seg_and(m, lane, L.seg);
}
// walks of more than 64 steps: long_nw words per slot, set to all ones before the pass; every group ANDs its partial in (the order does not matter)
__device__ __forceinline__ void rs_long_partial(unsigned long long *__restrict__ long_acc, uint32_t long_nw, uint32_t slot, uint32_t w, unsigned long long m) {
    atomicAnd(&long_acc[(uint64_t)slot * long_nw + w], m);
}

// ---- host: the species table of a candidate set, by member_plan.hpp; per_bit(position in the per-bit arrays of H + C + 1 entries, candidate entry) ----
struct RsTable {
    std::vector<RsSpecies> tab;
    WalkMasks wm;
    uint32_t long_nw = 1;    // words per slot of the long-walk partials: the widest species
    bool by_node = false;    // route 1 is open
};
template <class PerBit>
inline void rs_table_build(const Ctx *ctx, const Db *db, const uint64_t *cand_off, const uint32_t *cand_hap, RsTable &t, PerBit &&per_bit) {
    const uint32_t S = db->S;
    t.by_node = member_by_node(db->nh_built, ctx->cfg.read_strain_route);
    t.tab.assign(S ? S : 1, RsSpecies{});
    for (uint32_t s = 0; s < S; ++s) {
        RsSpecies &st = t.tab[s];
        st.m = t.wm.row(db, s, t.by_node, cand_hap + cand_off[s], cand_off[s + 1] - cand_off[s]);
        st.bit_base = member_bit_base(st.m.route, db->h_hap_off[s], db->H, cand_off[s]);
        member_file_bits(st.m.route, cand_hap + cand_off[s], st.m.K, 0, [&](uint64_t bit, uint64_t k) { per_bit(st.bit_base + bit, cand_off[s] + k); });
        t.long_nw = std::max(t.long_nw, st.m.nw);
    }
}

}  // namespace ptx
