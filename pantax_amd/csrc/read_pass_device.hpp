// read_pass_device.hpp -- what the eight passes over the locus-grouped step stream share: a wave per 64-step group, a lane per step.  Who takes what:
//   stage_read_strain.hip    (read_strains)         the species table, rs_lane / rs_lane_word / seg_and, the long-walk partials, the host skeleton;
//   stage_read_support.hip   (strain_read_support)  the same, and Q(r) with its wave sums, the species rounds, the lane-per-slot prologue, the counter block;
//   stage_read_em.hip        (strain_read_em)       as read support, less the counter block (its class tables grow between reruns and stay its own);
//   stage_mosaic.hip         (strain_mosaic)        rs_lane, seg_and, rs_word1, rs_lanes, Q(r), the species rounds, the counter block, the group launch;
//   stage_rescue.hip         (strain_read_rescue)   the same, and the long-walk partials with their flags and the lane-per-slot prologue;
//   stage_links.hip          (strain_links)         rs_lane, rs_word1, the species rounds, the table, the group launch -- its read pass, and the species
//                                                   rounds once more in links_count_kernel, a lane per distinct link: the loop is written in one place;
//   stage_rarefy.hip         (strain_rarefy)        the species rounds and the group launch (it has no species table and no candidate masks);
//   stage_fragments.hip      (strain_fragments)     rs_lane, rs_lane_word / seg_and, the long-walk partials, the table and the group launch in its mask pass;
//                                                   Q(r) with its wave sums, the species rounds and the counter block in its join, a lane per slot.
// The step codes and the slot lookup are those of the coverage pass (cov_device.hpp).  Device code and the host code that feeds it; include from .hip
// files only.  The kernels keep flat parameter lists with __restrict__ on every pointer: the helpers share code, not a kernarg layout.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>
#include "common.hpp"
#include "cov_device.hpp"
#include "member_device.hpp"
#include "primitives.hpp"

namespace ptx {

constexpr uint32_t RS_NO_SLOT = NO_SLOT;

struct RsSpecies { MemberRow m; uint32_t bit_base; };   // bit_base: first entry of the species in the per-bit arrays (bit_w / bit_hap, bit_w / bit_entry)

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
    L.slot = slot_in_group(gs, code, lane);
    L.live = code != STEP_PAD && L.slot < n_slots;
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
// The one-word membership of global node v over the species' chosen list: haplotype bits on route 1, list positions on route 2; a species without a
// list (route 0) is walked by nobody
__device__ __forceinline__ unsigned long long rs_word1(const RsSpecies &st, uint32_t v, const unsigned long long *__restrict__ node_haps,
                                                       const unsigned long long *__restrict__ mask) {
    if (st.m.route == 0u) return 0ull;
    return st.m.route == 1u ? (node_haps[v] & st.m.bits) : mask[member_mask_row(st.m, v)];
}
// word w of the AND over my walk's steps in this wave, up to and including mine (all 64 lanes call it: a wave-uniform trip count over w).  Its own
// membership line, not rs_word1: w < nw has ruled route 0 out and the row is at hand, and through rs_word1 read_strain_kernel measured 6 % slower
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
__device__ __forceinline__ unsigned long long rs_lanes(int a, int b) { return (~0ull << a) & (~0ull >> (63 - b)); }   // lanes a .. b

// ---- Q(r) = (1, #steps, span) of a read and its sums ----
struct RsQ { unsigned long long n, steps, span; };
__device__ __forceinline__ uint32_t rs_span(const uint4 &rr) { return rr.w >= rr.z ? rr.w - rr.z : 0u; }
__device__ __forceinline__ void rs_add3(unsigned long long *__restrict__ dst, unsigned long long n, unsigned long long steps, unsigned long long span) {
    if (n) atomicAdd(dst, n);
    if (steps) atomicAdd(dst + 1, steps);
    if (span) atomicAdd(dst + 2, span);
}
// sum of Q over the lanes of `on` (its ballot is `b`); all 64 lanes call it, the result is wave-uniform
__device__ __forceinline__ RsQ rs_reduce(bool on, unsigned long long b, uint32_t steps, uint32_t span) {
    const auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
    return RsQ{(unsigned long long)__popcll(b), wave_reduce(on ? (unsigned long long)steps : 0ull, add), wave_reduce(on ? (unsigned long long)span : 0ull, add)};
}
// ... -> dst, one 64-bit atomicAdd per non-zero sum from lane 0
__device__ __forceinline__ void rs_reduce_add(int lane, bool on, unsigned long long b, uint32_t steps, uint32_t span, unsigned long long *__restrict__ dst) {
    const RsQ q = rs_reduce(on, b, steps, span);
    if (lane == 0) rs_add3(dst, q.n, q.steps, q.span);
}

// The species rounds of a wave: body(s0, mine, mb) once per species present among the lanes of `on` -- s0 the species, mine = my lane is on and of s0,
// mb the ballot of mine.  The species of the first lane left goes first; the stream is grouped by locus, so one or two rounds as a rule.  All 64 lanes
// call it and the loop is wave-uniform: the body may ballot and reduce.
template <class Body>
__device__ __forceinline__ void rs_species_rounds(bool on, uint32_t sp, Body &&body) {
    for (unsigned long long rem = __builtin_amdgcn_ballot_w64(on); rem;) {
        const uint32_t s0 = lane_get(sp, __builtin_ctzll(rem));
        const bool mine = on && sp == s0;
        const unsigned long long mb = __builtin_amdgcn_ballot_w64(mine);
        rem &= ~mb;
        body(s0, mine, mb);
    }
}

// The prologue of the kernels that take a lane per slot behind the group pass (walks of more than 64 steps): slot base + lane, its records, and whether
// the lane decides a counted read.  base is wave-uniform.
struct RsLongSlot {
    uint64_t s;
    uint4 rr;
    uint32_t sp;
    bool in, decide;
};
__device__ __forceinline__ RsLongSlot rs_long_slot(uint64_t base, int lane, uint32_t n_slots, const uint4 *__restrict__ read_rec,
                                                   const uint2 *__restrict__ slot_rec) {
    RsLongSlot t;
    t.s = base + (uint64_t)lane;
    t.in = t.s < n_slots;
    t.rr = make_uint4(0u, 0u, 0u, 0u);
    t.sp = 0xFFFFFFFFu;
    if (t.in) { t.rr = read_rec[t.s]; t.sp = slot_rec[t.s].x; }
    t.decide = t.in && t.rr.y > 64u && (int32_t)t.sp >= 0;
    return t;
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
inline const unsigned long long *rs_node_haps(const RsTable &rt, const Db *db) { return rt.by_node ? (const unsigned long long *)db->d_node_haps.p : nullptr; }

// the per-bit arrays hold H + n + 1 entries at 32-bit positions
inline int rs_check_bits(Ctx *ctx, const char *call_name, uint64_t H, uint64_t n) {
    if (H + n >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: %llu haplotypes + candidates exceed 32-bit positions", call_name, (unsigned long long)(H + n));
    return 0;
}

// The per-slot words of the walks of more than 64 steps (all ones: the identity of the AND the groups form) and, for the rescue pass, the per-slot u32
// flags (zero).  Both exist only when the reads hold such walks: n_long counts slots, so n_long != 0 implies n_slots != 0, and this test and the guard of
// rs_launch_slots agree.
struct RsLongAcc {
    DevBuf<unsigned long long> d_acc;
    DevBuf<uint32_t> d_flag;
    int init(Ctx *ctx, const Reads *rd, uint32_t words_per_slot, bool with_flags = false) {
        const bool any_long = rd->n_long != 0;
        const size_t n = any_long ? (size_t)rd->n_slots * words_per_slot : 1;
        PTX_HIP(ctx, d_acc.alloc(n));
        if (any_long) PTX_HIP(ctx, hipMemsetAsync(d_acc.p, 0xFF, n * sizeof(unsigned long long), ctx->stream));
        if (!with_flags) return 0;
        PTX_HIP(ctx, d_flag.alloc(any_long ? (size_t)rd->n_slots : 1));
        if (any_long) PTX_HIP(ctx, hipMemsetAsync(d_flag.p, 0, (size_t)rd->n_slots * sizeof(uint32_t), ctx->stream));
        return 0;
    }
};

// The u64 counters of a call as one device block, zero-filled once; take(n) hands out the next sub-array, so the order of the takes is the layout
struct RsCounters {
    DevBuf<unsigned long long> d;
    size_t used = 0;
    int init(Ctx *ctx, size_t n) {
        PTX_HIP(ctx, d.alloc(n));
        return zero_fill(ctx, d.p, n * sizeof(unsigned long long));
    }
    unsigned long long *take(size_t n) { unsigned long long *const p = d.p + used; used += n; return p; }
};

// The two launches.  Groups: a wave per 64-step group, the kernel's parameters begin (n_groups, n_slots, group_slot, step_code, g_node_id, read_rec,
// slot_rec); slots: a lane (or a thread) per slot, only when the reads hold walks of more than 64 steps, the parameters begin (n_slots, read_rec,
// slot_rec).  rest... follows.  Nothing is launched for reads without slots.
template <class Kernel, class... Rest>
inline void rs_launch_groups(Ctx *ctx, const Reads *rd, const char *label, Kernel kernel, Rest &&...rest) {
    const uint32_t n_slots = rd->n_slots, n_groups = (uint32_t)(rd->T_pad / 64);
    if (!n_slots || !n_groups) return;
    KTimer tm(ctx, label);
    hipLaunchKernelGGL(kernel, dim3(grid_for(n_groups, 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, n_groups, n_slots, rd->d_g_group_slot.p,
                       rd->d_g_step_dup.p, rd->d_g_node_id.p, rd->d_g_read_rec.p, rd->d_g_slot_rec.p, std::forward<Rest>(rest)...);
}
template <class Kernel, class... Rest>
inline void rs_launch_slots(Ctx *ctx, const Reads *rd, const char *label, Kernel kernel, Rest &&...rest) {
    const uint32_t n_slots = rd->n_slots;
    if (!n_slots || !rd->n_long) return;
    KTimer tm(ctx, label);
    hipLaunchKernelGGL(kernel, dim3(grid_for(((uint64_t)n_slots + 63) / 64, 4, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, n_slots, rd->d_g_read_rec.p,
                       rd->d_g_slot_rec.p, std::forward<Rest>(rest)...);
}

}  // namespace ptx
