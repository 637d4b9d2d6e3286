// stage_cov.hip -- a8: the per-node coverage histogram (get_node_abundances, profile.rs:743-1026).
//
// Per read (semantics restated from the reference, line-cited below):
//   * local node = id - range_start (profile.rs:790 with start = range_start-1, :2886)
//   * one-node walk: target = pend-pstart; <0 => dropped (:821-827); bases += target (:828-829);
//     bitmap [pstart,pend) only if pstart<pend<=node_len (:832-841)
//   * otherwise: first node aligns node_len-pstart from pstart (:853-856; reference asserts
//     pstart<=node_len), interior nodes align fully (:860-862), the last aligns
//     max(target-seen,0) (:857-859); the bitmap is marked for every occurrence, clipped to the
//     node (:870-873); `seen` advances on every occurrence (:878) but bases are added once per
//     distinct node of the read (:879-882)
//   * every 3-window (a,b,c) is looked up in either orientation in the unique-trio table and adds
//     the read-local aligned lengths of its three nodes (:890-907)
// Outputs are integers and bit-exact: 64-bit atomic adds and 32-bit atomic ORs commute.
//
// Mapping: ONE THREAD PER WALK STEP.  A wave64 holds 64 consecutive steps (~8 neighbouring short
// reads); everything a step needs from its predecessors in the read comes from neighbouring lanes:
//   - `seen` (sum of aligned lengths before the last node): segmented wave scan over the lanes
//   - first-occurrence test of a node inside the read: shuffle compare against the earlier lanes
//   - (node, read_nodes_len) of steps i-1, i-2 for the 3-window: __shfl_up by 1 and 2
// Walks of <= 64 steps never straddle a wave (padded stream).  Longer walks (HiFi / ONT reads, hundreds of steps) get
// what lies in other waves from data prepared outside this kernel, all O(1) per step: a per-step "node occurred
// earlier in the walk" flag computed at upload (group_fill_long_kernel, LDS hash per walk), the sum of the node
// lengths before the last step from walk_sum_kernel, and plain loads for the two neighbours across a wave border.  The kernel
// is bound by the number of divergent (one cache line per lane) vector-memory instructions, so the
// tables it gathers from are packed into 16-byte records (one dwordx4 per lookup):
//   read_rec[r] = {first step, #steps, pstart, pend}      node_rec[v] = {bit_off (u64), len, -}
//   lookup head of node v (rides in node_rec) = {first row, #rows} of the unique windows whose MIDDLE is v;  trio_ent[j] = {smaller end, larger end} -- j IS the row (round 5: rows are numbered in filing order)
// A read that reaches this kernel was binned to its species, so every node id lies inside the
// species' id range (rcls.rs:253-257) and the index panic of profile.rs:849 cannot occur; an
// out-of-range id (inconsistent external binning) is counted as an abort per step instead.
//
// Algorithmic bytes per launch (the a8 row minus its popcount pass):
//   4T + 12R + 4V(node_len) + 8V(bases) + L/8 (bitmap) + 12*(T-2R) (trio probes)
// Layout: node arrays of all resident species are concatenated; a node's coverage bitmap starts
// at bit bit_off[v] of one global bit vector (1 bit per graph base instead of the reference's
// 1 byte, profile.rs:776-781).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "common.hpp"
#include "primitives.hpp"
#include "wave.hpp"
#include "cov_plan.hpp"
#include "cov_device.hpp"
// bools are combined with & and | on purpose in the coverage kernels (no short-circuit control flow: every operand is a plain comparison or a vote)
#pragma clang diagnostic ignored "-Wbitwise-instead-of-logical"

namespace ptx {

// ---------------------------------------------------------------------------------------------
// The short-read kernel: every 64-step group whose walks all have <= 64 steps (no STEP_LONG code: all of a short-read
// sample).  Such walks never straddle a group, so a wave holds whole reads and NOTHING of a step's read lives outside the
// wave: no border lanes, no walk sums, no per-step slot array.  Written for instruction count -- the kernel is bound by VALU /
// SALU issue at full occupancy, not by bytes (round 2: 337 VALU + 270 SALU wave-instructions per 64 steps, most of the SALU
// from exec-mask branches): loads are unconditional with a safe index on dead lanes, per-lane cases are selects, and only
// the LDS / memory updates sit under a mask.  Groups that hold a step of a longer walk are left to coverage_step_kernel.
// Levels: {code, node id} + group_slot (scalar) -> {read record 16 B, slot record 8 B} -> {node record 16 B, active byte}
// -> two unique-trio entries.  Off the chain: level 1 since round 5 and level 2 since round 6 (requested one / two rounds ahead), level 3 since round 25
// (the node record requested a round ahead at the delta of the item's species guess, checked against the lane's species when the slot record is
// there: PF3 in the body).  Level 4 is paid every round.
// Workgroup = one ITEM of the read layout (build_step_read): up to COV_ITEM_GROUPS consecutive groups whose reads all START inside one
// block of 2048 node ids.  (Round 3 gave every workgroup a fixed number of groups: where a species is thinly covered -- most species of a
// Dirichlet-distributed sample -- 4096 steps span more nodes than the LDS windows hold, and every update outside them is a memory-side
// atomic: 3.3 of the kernel's 10.6 ms at 1e4 strains.  By node block the windows cover the block whatever the depth, and a deeply
// covered block is simply cut into more items.)
//
// LONG (round 6): the same select-only body for the groups that hold steps of walks of MORE than 64 steps (HiFi / ONT reads; round 5 sent them through
// coverage_step_kernel, whose per-lane branches for wave-straddling walks -- dependent loads under an exec mask for the two neighbours across a wave
// border, for the first node of the walk, for the walk sums -- made it the kernel furthest from its roofline: 0.16 of peak with no wasted traffic).
// What a step of such a walk needs from OTHER waves is fetched unconditionally and wave-uniformly:
//   * the two steps in front of the wave (ids, step codes, node records): addresses that depend on the group alone -> scalar loads, issued with the
//     level they belong to (ids / codes with the stream, node records with the node gather), never a dependent load behind a per-lane test;
//   * per slot {length of the walk's first node, sum of the node lengths before the last step} (walk_sum_kernel) and the id of the walk's first
//     step: gathers with the read record / the node record, for every lane (the lanes of one walk share the address);
// and every per-lane case is a select.  only_long != 0: groups without a step of a longer walk are the plain instantiation's.
template <bool WITH_TRIO, int U, int PASSES, int WIN, bool LONG = false>
#if !defined(COV_NO_PF3) && !defined(COV_NO_PF2) && !defined(COV_NO_PREFETCH)
__attribute__((amdgpu_waves_per_eu((U <= 2 && !LONG) ? 6 : 1)))      // (the short-read shapes of two groups in flight: 80 vector registers, six waves -- no scratch, profiles/r25)
#endif
__global__ void __launch_bounds__(COV_BLOCK) coverage_fast_kernel(
    const uint2 *__restrict__ items, const uint32_t *__restrict__ group_slot, const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
    const uint32_t *__restrict__ node_id, const uint8_t *__restrict__ step_code, const uint8_t *__restrict__ active,
    const uint4 *__restrict__ node_rec, const uint64_t *__restrict__ bit_off, uint64_t V, unsigned long long *__restrict__ bases,
    uint32_t *__restrict__ bitmap, uint32_t *__restrict__ full, const uint2 *__restrict__ trio_ent, unsigned long long *__restrict__ trio_bases,
    unsigned long long *__restrict__ n_abort, uint32_t ablate, int blk_shift,
    const uint32_t *__restrict__ long_sum = nullptr, const uint32_t *__restrict__ long_len0 = nullptr, uint32_t only_long = 0u,
    uint32_t chunk_groups = 0u, uint32_t total_groups = 0u, uint32_t win_back = 0u, const uint32_t *__restrict__ item_sel = nullptr,
    uint32_t spec_miss = 0u) {
    constexpr int WAVES = COV_BLOCK / 64;
#if !defined(COV_NO_PF3) && !defined(COV_NO_PF2) && !defined(COV_NO_PREFETCH)
    const int lane = threadIdx.x & 63, wave = LONG ? (int)(threadIdx.x >> 6) : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (a scalar: group indices stay out of the vector registers)
#else
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#endif
    // this workgroup's groups [g0, n_groups): an item of the read layout -- or, LONG, a plain cut of the stream: a long walk begins anywhere in a group,
    // so hardly any group starts with the first step of a read and the layout's items are arbitrary cuts anyway; the windows then begin `win_back` nodes
    // in front of the first live step's node (a reverse-strand walk runs DOWN from its first node, the key the stream is ordered by)
    uint32_t g0, n_groups;
    if constexpr (LONG) { g0 = blockIdx.x * chunk_groups; n_groups = min(g0 + chunk_groups, total_groups); }
    else { const uint2 item = items[item_sel ? item_sel[blockIdx.x] : blockIdx.x]; g0 = item.x; n_groups = item.y; }   // (item_sel: the items a db of SOME of the species launches)
    for (int i = threadIdx.x; i < (int)(cov_lds_bytes(WIN) / 4); i += COV_BLOCK) s_cov[i] = 0;      // the three windows, one block
    // window base: the node of the first step of the first group that has a live one (workgroup-uniform scalar loads)
    uint32_t wlo = 0, win_n = 0, mark_n = 0, bit0_lo = 0, bwn = 0;
    uint64_t bw0 = 0;
    // ... and the item's guess (PF3 below): species and delta of that group's first slot -- an ACTIVE species, the loop requires it.  No live group: a
    // species no read has
    uint32_t s0 = 0xFFFFFFFFu, dlt0 = 0;
#pragma unroll 1
    for (uint32_t g = g0; g < n_groups && win_n == 0; ++g) {
        const uint32_t gs = group_slot[g];
        if (gs == NO_SLOT) continue;
        const uint2 sr0 = slot_rec[gs];
        if ((int)sr0.x < 0 || !active[sr0.x]) continue;
        s0 = sr0.x; dlt0 = sr0.y;
        // the window starts at the item's NODE BLOCK, not at its first read: the reads of a bucket of the layout (512 ids wide at 3e8 nodes)
        // are in no particular order, so later reads of the item may start hundreds of nodes in front of the first one -- every read of
        // the item starts inside the block (build_step_read), and ids and node indices run in step inside a species
        const uint32_t id0 = node_id[(uint64_t)g * 64], v0 = id0 + sr0.y, in_blk = id0 & ((1u << blk_shift) - 1u);
        const uint32_t back = LONG ? win_back : in_blk + 64u;
        wlo = (v0 > back ? v0 - back : 0u) & ~63u;
        win_n = WIN;
        const uint64_t b_lo = bit_off[wlo], b_hi = bit_off[min((uint64_t)wlo + WIN, V)];
        bw0 = b_lo >> 5;
        bit0_lo = (uint32_t)(bw0 << 5);
        bwn = COV_BWIN;
        // every node of the window has its bits inside the LDS bit window: a partial range is marked in 32-bit positions relative to it
        mark_n = (b_hi - (bw0 << 5) <= (uint64_t)COV_BWIN * 32) ? (uint32_t)min((uint64_t)WIN, V - wlo) : 0u;
    }
    if (spec_miss) s0 = 0xFFFFFFFFu;       // option cov_spec=miss (tests): no read matches the guess, every wave takes the fallback loads
    // the barrier orders the LDS zero-fill only (a workgroup fence on the local address space): the window probes above are
    // still in flight and are first needed by the updates of the first pass, behind that pass's own three levels of loads (PF3: `wlo`, the safe
    // index of the speculative node records, by the prologue's requests)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    // Level 1 of round r + 1 is requested at the top of round r (round 5): the stream loads are the one level that comes from HBM every time, and the
    // kernel waits for its four dependent levels two thirds of the time -- three more registers per group in flight (64 in all: still eight waves per
    // SIMD) take the first level off the chain: 5.70 -> 5.21 ms at 1e8 reads, 0.62 -> 0.57 at 1e7 (same box, alternating builds).  -DCOV_NO_PREFETCH:
    // the round-4 loop, for measurements.
#ifndef COV_NO_PREFETCH
    uint32_t n_code[U], n_id[U], n_gs[U];
    {
        const uint32_t gw0 = g0 + (uint32_t)(wave * U);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g = gw0 + (uint32_t)u < n_groups ? gw0 + (uint32_t)u : (gw0 < n_groups ? gw0 : g0);
            const uint64_t t = (uint64_t)g * 64 + lane;
            n_code[u] = step_code[t]; n_id[u] = node_id[t]; n_gs[u] = group_slot[g];
        }
    }
#endif
    // The plain instantiation takes TWO levels off the chain (round 6): the stream loads run two rounds ahead and the read / slot records of the coming
    // round are requested at the top of this one -- nine more registers per group in flight, 5.30 -> 5.13 ms at 1e8 reads (-DCOV_NO_PF2: one level)
#if !defined(COV_NO_PF2) && !defined(COV_NO_PREFETCH)
    constexpr bool PF2 = !LONG;
#else
    constexpr bool PF2 = false;
#endif
    // ... and takes level 3's NODE RECORD off the chain as well (round 25).  Level 3 waited for level 2 only because v = id + slot_rec.y; every read of an
    // item starts inside one block of 2048 ids and a species has hundreds of thousands, so the reads of an item are one species' in all but the item at a
    // species border -- and that species' delta is a scalar since the window probe (dlt0).  The record is requested from the id alone, with the
    // coming round's read / slot records; level 3 checks every ok lane's species against the guess (species, not delta: contiguous ranges give every
    // species the same delta, and a hit wave also skips the `active` gather -- s0 is active), and the rare wave with a lane of another species does
    // the old two loads instead (wave-uniform).  The exposed chain per round: trio entries alone.  -DCOV_NO_PF3: round 6's body.
    // Registers decide whether it pays: the plain way (four more per group in flight) is 86 VGPRs = FIVE waves per SIMD and 5.12 -> 5.47 ms, slower than
    // round 6's body.  Kept at 80 = six waves, without scratch: the slot record travels as its species alone (a hit wave's delta is dlt0; the
    // fallback loads the record again), `active` is folded into ok where it is loaded, the wave index is a scalar (group indices and the groups'
    // first slots live in SGPRs) and the two-group shapes ask for six waves: 5.12 -> 5.00 ms (profiles/r25_*; the kernel is no latency chain alone)
#if !defined(COV_NO_PF3)
    constexpr bool PF3 = PF2;
#else
    constexpr bool PF3 = false;
#endif
    // the speculative index: always inside the table -- dead lanes, pads and reads of no species request SOME record they never use
    const auto guess_v = [&](uint32_t id) { const uint32_t vg = id + dlt0; return vg < V ? vg : wlo; };
    uint32_t c_code[U], c_id[U], c_gs[U];      // PF2: this round's level 1 ...
    uint4 c_rr[U];                             // ... and level 2, requested a round ago
    uint2 c_sr[U];                             // (PF3: the species alone)
    uint4 c_nr[U];                             // PF3: ... and the node record at the item's delta
    bool c_run[U];                             // ... and whether the group is this kernel's at all (wave-uniform: decided once, when its records are requested)
#pragma unroll
    for (int u = 0; u < U; ++u) c_run[u] = false;
    if constexpr (PF2) {
        const uint32_t gw0 = g0 + (uint32_t)(wave * U), gw1 = gw0 + (uint32_t)(WAVES * U);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            c_code[u] = n_code[u]; c_id[u] = n_id[u]; c_gs[u] = n_gs[u];           // round 0 (requested above)
            const uint32_t g = gw1 + (uint32_t)u < n_groups ? gw1 + (uint32_t)u : (gw0 < n_groups ? gw0 : g0);
            const uint64_t t = (uint64_t)g * 64 + lane;
            n_code[u] = step_code[t]; n_id[u] = node_id[t]; n_gs[u] = group_slot[g];   // round 1
            const bool pad0 = c_code[u] == STEP_PAD;
            const bool run0 = (gw0 + (uint32_t)u < n_groups) & any1(!pad0) & none1(!pad0 & ((c_code[u] & STEP_LONG) != 0u));
            const uint32_t sl = slot_in_group(c_gs[u], c_code[u], lane);
            const uint32_t slot = (pad0 | !run0) ? (c_gs[u] == NO_SLOT ? 0u : c_gs[u]) : sl;
            c_rr[u] = read_rec[slot];
            if constexpr (PF3) c_sr[u] = make_uint2(slot_rec[slot].x, 0u); else c_sr[u] = slot_rec[slot];
            if constexpr (PF3) c_nr[u] = node_rec[guess_v(c_id[u])];
            c_run[u] = run0;
        }
        if constexpr (PF3) __builtin_amdgcn_sched_barrier(0);      // (the requests stay where they are written: in front of the first round)
    }
#pragma unroll 1
    for (int pass = 0;; ++pass) {
        const uint32_t gw = g0 + (uint32_t)((pass * WAVES + wave) * U);     // this wave's U consecutive groups
        if (gw >= n_groups) break;
        // ---- level 1
        uint32_t code[U], id[U], gs[U];
        bool run[U];                                                          // wave-uniform: the group is this kernel's
        uint4 rr[U];
        uint2 sr[U];
        uint4 nrg[U];                                                         // PF3: the node record at the item's delta
#ifndef COV_NO_PREFETCH
        if constexpr (PF2) {
            const uint32_t gn = gw + (uint32_t)(WAVES * U), g2 = gn + (uint32_t)(WAVES * U);   // the coming round's groups, and the one behind it
            uint32_t m_code[U], m_id[U], m_gs[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                run[u] = c_run[u];
                code[u] = c_code[u]; id[u] = c_id[u]; gs[u] = c_gs[u]; rr[u] = c_rr[u]; sr[u] = c_sr[u];
                if constexpr (PF3) nrg[u] = c_nr[u];
                const uint32_t g = g2 + (uint32_t)u < n_groups ? g2 + (uint32_t)u : gw;
                const uint64_t t = (uint64_t)g * 64 + lane;
                m_code[u] = step_code[t]; m_id[u] = node_id[t]; m_gs[u] = group_slot[g];
                // level 2 of the coming round (its level 1 was requested a round ago)
                const bool padn = n_code[u] == STEP_PAD;
                const bool runn = (gn + (uint32_t)u < n_groups) & any1(!padn) & none1(!padn & ((n_code[u] & STEP_LONG) != 0u));
                const uint32_t sl = slot_in_group(n_gs[u], n_code[u], lane);
                const uint32_t slot = (padn | !runn) ? (n_gs[u] == NO_SLOT ? 0u : n_gs[u]) : sl;
                c_rr[u] = read_rec[slot];
                if constexpr (PF3) c_sr[u] = make_uint2(slot_rec[slot].x, 0u); else c_sr[u] = slot_rec[slot];
                if constexpr (PF3) c_nr[u] = node_rec[guess_v(n_id[u])];       // level 3's node record of the coming round, from the id alone
                c_run[u] = runn;
                c_code[u] = n_code[u]; c_id[u] = n_id[u]; c_gs[u] = n_gs[u];
                n_code[u] = m_code[u]; n_id[u] = m_id[u]; n_gs[u] = m_gs[u];
            }
            if constexpr (PF3) __builtin_amdgcn_sched_barrier(0);             // (the requests leave here, with level 2's, not behind this round's waits)
        } else
        {
            const uint32_t gn = gw + (uint32_t)(WAVES * U);                    // the coming round's groups
#pragma unroll
            for (int u = 0; u < U; ++u) {
                run[u] = gw + (uint32_t)u < n_groups;
                code[u] = n_code[u]; id[u] = n_id[u]; gs[u] = n_gs[u];
                const uint32_t g = gn + (uint32_t)u < n_groups ? gn + (uint32_t)u : gw;
                const uint64_t t = (uint64_t)g * 64 + lane;
                n_code[u] = step_code[t]; n_id[u] = node_id[t]; n_gs[u] = group_slot[g];
            }
        }
#else
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g = gw + (uint32_t)u;
            run[u] = g < n_groups;
            const uint64_t t = (uint64_t)(run[u] ? g : gw) * 64 + lane;
            code[u] = step_code[t]; id[u] = node_id[t];
            gs[u] = group_slot[run[u] ? g : gw];
        }
#endif
        // ---- level 2 (dead lanes read the group's first record: in range, and on a line that is fetched anyway)
        bool pad[U];
        uint32_t slot_[U];
        uint32_t ll0[U], lsum[U];                                             // LONG: first node length / sum of the lengths before the last step, by slot
#pragma unroll
        for (int u = 0; u < U; ++u) {
            pad[u] = code[u] == STEP_PAD;
            if constexpr (!PF2) {
                const bool has_long = any1(!pad[u] & ((code[u] & STEP_LONG) != 0u));
                // nothing here / a group of the OTHER instantiation (steps of a longer walk: LONG's; none: the plain one's, unless LONG takes every group)
                run[u] = run[u] & any1(!pad[u]) & (LONG ? (has_long | (only_long == 0u)) : !has_long);
            }
            const uint32_t sl = slot_in_group(gs[u], code[u], lane);
            const uint32_t slot = (pad[u] | !run[u]) ? (gs[u] == NO_SLOT ? 0u : gs[u]) : sl;
            if constexpr (!PF2) { rr[u] = read_rec[slot]; sr[u] = slot_rec[slot]; }     // (PF2: requested a round ago)
            if constexpr (LONG) { ll0[u] = long_len0[slot]; lsum[u] = long_sum[slot]; }
            slot_[u] = slot;
        }
        // LONG: the two steps in front of the wave's group (wave-uniform addresses: position of the group - 1, - 2; the dword of step codes in front of it)
        uint32_t h_id1[U], h_id2[U], h_codes[U];
        if constexpr (LONG) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t gu = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gw + (uint32_t)u));
                const uint64_t t0 = (uint64_t)(run[u] && gu != 0u ? gu : 1u) * 64;     // (group 0 has nothing in front of it: any in-range address)
                h_id1[u] = node_id[t0 - 1]; h_id2[u] = node_id[t0 - 2];
                h_codes[u] = *reinterpret_cast<const uint32_t *>(step_code + t0 - 4);
            }
        }
        // ---- level 3
        uint4 nr[U];
        uint32_t v[U], act[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = run[u] & !pad[u] & ((int)sr[u].x >= 0);
            if constexpr (PF3) {
                // every ok lane is of the guessed species: its delta is dlt0, its record is the one requested a round ago (v < V for an id of its species)
                // and its species is active -- no `active` gather.  Lanes that are not ok hold SOME in-range record and never use it: `nl`, the marks and
                // the trio head shifted up from the lane below all sit under ok / live of the same read.
                // (each side waits for ITS record inside the branch -- the empty asm is a use: behind the join the compiler's one wait would be the
                // fallback's, for everything in flight with the coming round's requests among it, on the hit side too)
                if (none1(ok[u] & (sr[u].x != s0))) {
                    v[u] = ok[u] ? id[u] + dlt0 : wlo;
                    nr[u] = nrg[u];
                    asm volatile("" : "+v"(nr[u].x), "+v"(nr[u].y), "+v"(nr[u].z), "+v"(nr[u].w));
                } else {                                                      // a wave at a species border: the slot record's delta again, then round 6's two loads
                    v[u] = ok[u] ? id[u] + slot_rec[slot_[u]].y : wlo;
                    nr[u] = node_rec[v[u]];
                    const uint32_t a = active[ok[u] ? sr[u].x : 0u];
                    asm volatile("" : "+v"(nr[u].x), "+v"(nr[u].y), "+v"(nr[u].z), "+v"(nr[u].w));
                    ok[u] = ok[u] & (a != 0u);
                }
                act[u] = 1u;                                                  // (folded into ok where it was loaded)
            } else {
            v[u] = ok[u] ? id[u] + sr[u].y : wlo;
            nr[u] = node_rec[v[u]];
            act[u] = active[ok[u] ? sr[u].x : 0u];      // never null here (the launcher passes all-ones when no species is deselected): an unconditional load
                                                        // travels beside the node record; under a pointer test the compiler waited for it first
            }
        }
        // LONG: id of the walk's first step (one address per walk) and the node records of the two steps in front of the wave (wave-uniform: the
        // walk of lane 0, when it began one / two steps or more before this group)
        uint32_t idf[U], i0_[U], hv1[U], hv2[U];
        uint4 nrh1[U], nrh2[U];
        if constexpr (LONG) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                idf[u] = node_id[rr[u].x];
                const uint32_t gbase = (gw + (uint32_t)u) * 64u;
                const bool ok0 = __builtin_amdgcn_readfirstlane((int)ok[u]) != 0;
                i0_[u] = ok0 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(gbase - rr[u].x)) : 0u;      // lane 0's position in its walk
                const uint32_t delta0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)sr[u].y);
                hv1[u] = i0_[u] >= 1u ? h_id1[u] + delta0 : wlo;
                hv2[u] = i0_[u] >= 2u ? h_id2[u] + delta0 : wlo;
                nrh1[u] = node_rec[hv1[u]]; nrh2[u] = node_rec[hv2[u]];
            }
        }
        // ---- level 4: the unique-trio entries of the window (i-2, i-1, i), requested as soon as the head is known
        uint32_t i_[U], nl[U], len0[U], nh[U], hx[U], tlo[U], thi[U];
        uint2 e0[U], e1[U];
        bool live[U], single[U], dead_read[U], cross[U];
        int dist[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t gbase = (gw + (uint32_t)u) * 64u;
            i_[u] = gbase + (uint32_t)lane - rr[u].x;                         // position in the walk (T_pad < 2^32)
            ok[u] = ok[u] & (act[u] != 0u);
            nl[u] = ok[u] ? nr[u].z : 0u;
            if constexpr (LONG) {
                dist[u] = (int)min(ok[u] ? i_[u] : 0u, (uint32_t)lane);       // earlier steps of my walk held by lower lanes
                cross[u] = ok[u] & (i_[u] > (uint32_t)lane);                  // the walk began before this wave
                const uint32_t in_wave = __shfl(nl[u], lane - dist[u]);
                len0[u] = cross[u] ? ll0[u] : in_wave;
            } else
            len0[u] = __shfl(nl[u], lane - (int)i_[u]);                       // length of the walk's first node: the lane of step 0 (live lanes)
            uint32_t v2 = wave_shr1(wave_shr1(v[u]));
            uint32_t hw1 = wave_shr1(nr[u].w), hy1 = wave_shr1(nr[u].y);         // the lookup head of the window's MIDDLE node: the lane below
            if constexpr (LONG) {                                             // across the wave border: the records fetched for the steps in front of the group
                v2 = lane == 0 ? hv2[u] : lane == 1 ? hv1[u] : v2;
                hw1 = lane == 0 ? nrh1[u].w : hw1; hy1 = lane == 0 ? nrh1[u].y : hy1;
            }
            single[u] = rr[u].y == 1u;
            dead_read[u] = !single[u] & (rr[u].z > len0[u]);                  // assert :854 -> the whole read contributes nothing
            live[u] = ok[u] & !dead_read[u] & !(single[u] & (rr[u].w < rr[u].z));   // :821-827
            nh[u] = 0; hx[u] = 0; tlo[u] = 0; thi[u] = 0;
            e0[u] = make_uint2(0u, 0u); e1[u] = e0[u];
            if (WITH_TRIO && !ABL(4u)) {
                // canonical window (min end, middle, max end): the rows are filed under the MIDDLE node, keyed by the two ends
                hx[u] = hw1;
                tlo[u] = min(v[u], v2); thi[u] = max(v[u], v2);
                // the node's pair filter: a window whose bit is clear is not among its rows -- nothing is fetched for it
                nh[u] = (live[u] & (i_[u] >= 2u) & ((nr_filter(hy1) & nr_pair_bit(tlo[u], thi[u])) != 0u)) ? nr_rows(hy1) : 0u;
                // the head's first TWO entries in one 16-byte load (entries are 8 bytes since round 5; the pair is dword-aligned, and the array has one
                // entry of slack behind its last row)
                const EntPair ep = *reinterpret_cast<const EntPair *>(trio_ent + (nh[u] ? hx[u] : 0u));
                e0[u] = make_uint2(ep.a, ep.b); e1[u] = make_uint2(ep.c, ep.d);
            }
        }
        // ---- per group: aligned lengths and the updates
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t k = rr[u].y, ps = rr[u].z, pe = rr[u].w, i = i_[u];
            if (any1(ok[u] & dead_read[u] & (i == 0u))) { if (ok[u] & dead_read[u] & (i == 0u)) atomicAdd(n_abort, 1ull); }
            // `seen` before this step = wave prefix sum of the walk's aligned lengths minus its value at the walk's first lane
            const uint32_t contrib = (live[u] & !single[u]) ? (i == 0u ? nl[u] - ps : nl[u]) : 0u;
            const uint32_t pexcl = wave_incl_scan_dpp(contrib) - contrib;
            uint32_t seen = pexcl - __shfl(pexcl, lane - (LONG ? dist[u] : (int)i));
            if constexpr (LONG) seen = cross[u] ? lsum[u] - ps : seen;        // (used by a walk's last step only) all steps but the last: walk_sum_kernel
            const uint32_t tgt = pe - ps;                                     // target (profile.rs:800) where it is not negative
            uint32_t aln = nl[u];                                             // :860-862
            if (i + 1u == k) aln = ((pe >= ps) & (tgt > seen)) ? tgt - seen : 0u;   // :857-859 max(target - seen, 0)
            if (i == 0u) aln = single[u] ? tgt : nl[u] - ps;                  // :853-856, :828
            const uint32_t sidx = i == 0u ? ps : 0u;
            uint32_t hi = sidx + aln;
            if (hi > nl[u]) hi = nl[u];                                       // :871
            const bool markable = live[u] & (hi > sidx) & !(single[u] & !((ps < pe) & (pe <= nl[u])));   // :832
            const uint32_t dupd = code[u] & STEP_DIST;                        // distance back to the node's first occurrence in the walk (0: this is it)
            bool earlier = dupd != 0u, at_step0 = dupd == i;                  // the node occurred earlier in the walk / its first occurrence is step 0
            if constexpr (LONG) {                                             // a longer walk's code: STEP_LONG | occurred earlier
                const bool lc = (code[u] & STEP_LONG) != 0u;
                const uint32_t id_first = cross[u] ? idf[u] : __shfl(id[u], lane - dist[u]);
                earlier = lc ? (code[u] & 1u) != 0u : earlier;
                at_step0 = lc ? id[u] == id_first : at_step0;
            }
            const uint32_t rl = !live[u] ? 0u : !earlier ? aln : (at_step0 ? len0[u] - ps : nl[u]);   // read_nodes_len :879-882
            const uint32_t off = v[u] - wlo;                                  // unsigned wrap: nodes below the window are out of range too
            const bool inw = off < win_n;
            if (live[u] & !earlier & (aln != 0u) && !ABL(2u)) {               // :881 / :828
                // (the 32-bit LDS sum of a work item: build_step_read cuts items of at most 256 groups, 16384 steps x (2^18 - 1) < 2^32; LONG's cuts
                // of the stream are covl_shape's chunk_groups, which nothing bounds this way)
                if (inw & (aln < (1u << 18))) atomicAdd(&S_WIN(off), aln);
                else atomicAdd(&bases[v[u]], (unsigned long long)aln);
            }
            const bool whole = markable & (sidx == 0u) & (hi == nl[u]);       // the whole node: one flag
            if constexpr (LONG) { if (!ABL(1u) && !ABL(8u)) mark_full_out_wave<WIN>(full, whole & !inw, v[u]); }
            if (markable && !ABL(1u)) {
                if (whole) {
                    if (inw) S_FULL(WIN, off) = 1; else if (!LONG && !ABL(8u)) atomicOr(&full[v[u] >> 5], 1u << (v[u] & 31));
                } else if (off < mark_n) {
                    const uint32_t rel = nr[u].x - bit0_lo;
                    mark_window(WIN, rel + sidx, rel + hi);
                } else if (!ABL(8u)) {
                    const uint64_t bo = nr_bit_off(nr[u]);
                    mark_range(bitmap, WIN, bw0, bwn, bo + sidx, bo + hi);
                }
            }
            if (WITH_TRIO && !ABL(4u)) {                                      // :890-907
                uint32_t rl1 = wave_shr1(rl), rl2 = wave_shr1(rl1);
                if constexpr (LONG) {
                    // read_nodes_len of the two steps in front of the wave (never a walk's last step): the length aligned at the node's FIRST occurrence
                    // in the read -- wave-uniform values of lane 0's walk (lane 1 uses them only when it continues that walk)
                    const uint32_t idf0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)idf[u]), l0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)len0[u]),
                                   ps0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ps);
                    const uint32_t c1 = h_codes[u] >> 24, c2 = (h_codes[u] >> 16) & 0xFFu;
                    const uint32_t rlh1 = ((i0_[u] == 1u) | (((c1 & 1u) != 0u) & (h_id1[u] == idf0))) ? l0 - ps0 : nrh1[u].z;
                    const uint32_t rlh2 = ((i0_[u] == 2u) | (((c2 & 1u) != 0u) & (h_id2[u] == idf0))) ? l0 - ps0 : nrh2[u].z;
                    rl2 = lane == 0 ? rlh2 : lane == 1 ? rlh1 : rl2;
                    rl1 = lane == 0 ? rlh1 : rl1;
                }
                // a row IS its lookup entry (round 5): the index of the entry that matches (rows are 32-bit; NO_ROW: none)
                constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
                const bool m0 = (nh[u] != 0u) & (e0[u].x == tlo[u]) & (e0[u].y == thi[u]);
                const bool m1 = (nh[u] > 1u) & (e1[u].x == tlo[u]) & (e1[u].y == thi[u]);
                uint32_t row = m0 ? hx[u] : m1 ? hx[u] + 1u : NO_ROW;
                if (any1(!(m0 | m1) & (nh[u] > 2u))) {
                    if (!(m0 | m1) & (nh[u] > 2u))
                        for (uint32_t j = 2; j < nh[u]; ++j) {
                            const uint2 e = trio_ent[hx[u] + j];
                            if (e.x == tlo[u] && e.y == thi[u]) { row = hx[u] + j; break; }
                        }
                }
                const uint32_t sum = rl2 + rl1 + rl;                             // three node lengths: far below 2^32
                if ((row != NO_ROW) & (sum != 0u)) atomicAdd(&trio_bases[row], (unsigned long long)sum);
            }
        }
    }
    __syncthreads();
    if (win_n) {
        for (int i = threadIdx.x; i < WIN; i += COV_BLOCK) {
            const uint32_t c = S_WIN(i);
            if (c) atomicAdd(&bases[wlo + i], (unsigned long long)c);
            const unsigned long long fb = __ballot(S_FULL(WIN, i) != 0);
            if (fb && (lane & 31) == 0 && !ABL(32u)) {
                const uint32_t m = (uint32_t)(fb >> (lane & 32));
                if (m) atomicOr(&full[(wlo + i) >> 5], m);
            }
        }
        if (!ABL(16u))
        for (uint32_t i = threadIdx.x; i < bwn; i += COV_BLOCK) {
            const uint32_t m = S_BM(WIN, i);
            if (m) atomicOr(&bitmap[bw0 + i], m);
        }
    }
}

// Walks of more than 64 steps: the last step needs `seen` = everything aligned before it (:857-859), which lives in
// other waves.  One cheap pass over the steps of long walks adds the node lengths of all steps but the last into
// long_sum[slot] (one atomic per wave and walk); launched only when the upload saw such walks.
template <int WS_U, bool EAGER = false>   // EAGER (most walks are long): the node ids and group slots are requested WITH the step codes, not behind the test for a long step
__global__ void __launch_bounds__(256) walk_sum_kernel(uint64_t T, const uint32_t *__restrict__ group_slot, const uint8_t *__restrict__ step_dup,
                                                       const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                       const uint32_t *__restrict__ node_id, const uint32_t *__restrict__ node_len,
                                                       uint32_t *__restrict__ long_sum, uint32_t *__restrict__ long_len0) {
    // WS_U groups of 64 steps per wave and round, the loads of a level issued for all of them before the first is used (the
    // pass is a chain of three dependent levels: {code, slot, id} -> {slot record, read record} -> node length, a 4-byte
    // gather from the plain length array, not the 16-byte node record)
    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256 * WS_U;
    for (uint64_t base = ((uint64_t)blockIdx.x * 256 + (threadIdx.x - lane)) * WS_U; base < T; base += stride) {
        uint32_t code[WS_U], slot[WS_U], id[WS_U], nl[WS_U], gs_e[WS_U], id_e[WS_U];
        uint64_t t[WS_U];
        bool any = false;
#pragma unroll
        for (int u = 0; u < WS_U; ++u) {
            t[u] = base + (uint64_t)u * 64 + lane;
            code[u] = t[u] < T ? step_dup[t[u]] : STEP_PAD;
            if constexpr (EAGER) { gs_e[u] = t[u] < T ? group_slot[t[u] >> 6] : NO_SLOT; id_e[u] = t[u] < T ? node_id[t[u]] : 0u; }
        }
#pragma unroll
        for (int u = 0; u < WS_U; ++u) any = any || (code[u] != STEP_PAD && (code[u] & STEP_LONG));
        if (!__any(any)) continue;
#pragma unroll
        for (int u = 0; u < WS_U; ++u) {
            slot[u] = NO_SLOT; id[u] = 0;
            uint32_t gs;
            if constexpr (EAGER) gs = gs_e[u]; else gs = t[u] < T ? group_slot[t[u] >> 6] : NO_SLOT;
            const uint32_t sl = slot_in_group(gs, code[u], lane);
            if (code[u] != STEP_PAD && (code[u] & STEP_LONG)) { slot[u] = sl; if constexpr (EAGER) id[u] = id_e[u]; else id[u] = node_id[t[u]]; }
        }
        uint2 sr[WS_U];
        uint4 rr[WS_U];
#pragma unroll
        for (int u = 0; u < WS_U; ++u) {
            sr[u] = make_uint2(0xFFFFFFFFu, 0u); rr[u] = make_uint4(0u, 0u, 0u, 0u);
            if (slot[u] != NO_SLOT) { sr[u] = slot_rec[slot[u]]; rr[u] = read_rec[slot[u]]; }
        }
#pragma unroll
        for (int u = 0; u < WS_U; ++u) {
            nl[u] = 0;
            const bool counted = slot[u] != NO_SLOT && (int)sr[u].x >= 0 && (uint32_t)(t[u] - rr[u].x) + 1 < rr[u].y;   // not the last step
            if (counted) nl[u] = node_len[id[u] + sr[u].y];
        }
#pragma unroll
        for (int u = 0; u < WS_U; ++u) {
            if (!__any(slot[u] != NO_SLOT)) continue;
            if (slot[u] != NO_SLOT && (int)sr[u].x >= 0 && (uint32_t)(t[u] - rr[u].x) + 1 < rr[u].y && t[u] == rr[u].x)
                long_len0[slot[u]] = nl[u];                          // length of the walk's first node, for the lanes of later waves
            // segmented sum over runs of equal slot (a walk's steps are contiguous), one atomic per run
            const uint32_t prev = __shfl_up(slot[u], 1);
            const bool head = lane == 0 || prev != slot[u];
            const unsigned long long heads = __ballot(head);
            const int start = 63 - __builtin_clzll(heads & ((2ull << lane) - 1ull));   // lane of my run's head
            // (one DPP prefix sum of the wave minus its value in front of the run's head -- 64 lengths stay far below 2^32 --; a segmented shuffle scan of six
            // bpermutes stood here until round 6)
            const uint32_t sc = wave_incl_scan_dpp(nl[u]);
            const uint32_t front = __shfl(sc, start > 0 ? start - 1 : 0);
            const uint32_t incl = sc - (start > 0 ? front : 0u);
            const unsigned long long after = heads & ~((2ull << lane) - 1ull);
            const bool tail = after ? (lane + 1 == __builtin_ctzll(after)) : lane == 63;
            if (tail && slot[u] != NO_SLOT && incl) atomicAdd(&long_sum[slot[u]], incl);
        }
    }
}

// node_base_cov[v] = number of covered bases (profile.rs:844/874, :1018-1023)
// a node some step covered whole carries a flag instead of marked bits (coverage_step_kernel): its count is its length
__global__ void __launch_bounds__(256) popcount_kernel(uint64_t V, const uint64_t *__restrict__ bit_off, const uint32_t *__restrict__ full,
                                                       const uint32_t *__restrict__ bitmap, uint32_t *__restrict__ cov) {
    for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (uint64_t)gridDim.x * 256) {
        uint64_t g0 = bit_off[v], g1 = bit_off[v + 1];
        uint32_t c = 0;
        if ((full[v >> 5] >> (uint32_t)(v & 31)) & 1u) c = (uint32_t)(g1 - g0);
        else if (g1 > g0) {
            uint64_t w0 = g0 >> 5, w1 = (g1 - 1) >> 5;
            uint32_t m0 = 0xFFFFFFFFu << (g0 & 31);
            uint32_t m1 = 0xFFFFFFFFu >> (31 - (uint32_t)((g1 - 1) & 31));
            if (w0 == w1) c = __popc(bitmap[w0] & m0 & m1);
            else {
                c = __popc(bitmap[w0] & m0);
                for (uint64_t w = w0 + 1; w < w1; ++w) c += __popc(bitmap[w]);
                c += __popc(bitmap[w1] & m1);
            }
        }
        cov[v] = c;
    }
}

// The same counts for graphs of LONG nodes (a single-genome species is a chain of 1024-bp chunks, build_eq1.rs:26-36: 32 words of the bit vector per
// node): the per-thread loop above walks 64 different cache lines per iteration (11 ms at the reference-DB shape).  Here a wave takes 64 consecutive nodes,
// reads the words of the whole stretch coalesced, keeps the number of set bits in front of every word in LDS (a DPP prefix sum per 64 words) and takes a
// node's count as the difference of that prefix at its two ends -- node_cov_stats_kernel<.., LONGN>'s scheme (stage_node_stats.hip) for the stage call.
constexpr uint32_t PCL_WORDS = 2304;   // words of one stretch the prefix holds; a longer stretch takes the per-lane loop
__global__ void __launch_bounds__(256) popcount_long_kernel(uint64_t V, const uint64_t *__restrict__ bit_off, const uint32_t *__restrict__ full,
                                                            const uint32_t *__restrict__ bitmap, uint32_t *__restrict__ cov) {
    __shared__ __attribute__((aligned(16))) uint32_t s_prefix[4 * PCL_WORDS];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *pw = s_prefix + wave * PCL_WORDS;
    const uint64_t n_str = (V + 63) / 64;
    for (uint64_t st = (uint64_t)blockIdx.x * 4 + wave; st < n_str; st += (uint64_t)gridDim.x * 4) {
        const uint64_t v = st * 64 + lane;
        const bool in = v < V;
        const uint64_t g0 = in ? bit_off[v] : 0ull, g1 = in ? bit_off[v + 1] : 0ull;
        const uint64_t b0 = __shfl(g0, 0);                                             // (lane 0 is always inside)
        const uint32_t last = (uint32_t)min((uint64_t)63, V - 1 - st * 64);
        const uint64_t b1 = __shfl(g1, (int)last);
        // (from the 16-byte boundary at or below the stretch's first word: four words per lane and load; what the last load reads beyond the stretch is
        // inside the arena -- the flags follow the bit vector -- and never looked up)
        const uint64_t wa = (b0 >> 5) & ~3ull, nw = b1 > b0 ? ((b1 - 1) >> 5) - wa + 1 : 0;
        const bool coop = nw <= (uint64_t)PCL_WORDS && __builtin_amdgcn_ballot_w64(in && g1 - g0 > 64ull) != 0ull;   // (wave-uniform)
        if (coop) {
            uint32_t carry = 0;
            for (uint32_t k = 0; k < (uint32_t)nw; k += 256) {
                const uint32_t i = k + 4u * lane;
                const uint4 x = i < (uint32_t)nw ? *reinterpret_cast<const uint4 *>(bitmap + wa + i) : make_uint4(0u, 0u, 0u, 0u);
                const uint32_t p0 = (uint32_t)__popc(x.x), p1 = p0 + (uint32_t)__popc(x.y), p2 = p1 + (uint32_t)__popc(x.z), p3 = p2 + (uint32_t)__popc(x.w);
                const uint32_t incl = wave_incl_scan_dpp(p3);
                const uint32_t base = carry + incl - p3;                                 // set bits in front of this lane's four words
                if (i < (uint32_t)nw) *reinterpret_cast<uint4 *>(pw + i) = make_uint4(base, base + p0, base + p1, base + p2);
                carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        }
        uint32_t c = 0;
        if (in && g1 > g0) {
            const uint64_t w0 = g0 >> 5, w1 = (g1 - 1) >> 5;
            const uint32_t m0 = 0xFFFFFFFFu << (g0 & 31), m1 = 0xFFFFFFFFu >> (31 - (uint32_t)((g1 - 1) & 31));
            if ((full[v >> 5] >> (uint32_t)(v & 31)) & 1u) c = (uint32_t)(g1 - g0);
            else if (coop) c = (pw[w1 - wa] + (uint32_t)__popc(bitmap[w1] & m1)) - (pw[w0 - wa] + (uint32_t)__popc(bitmap[w0] & ~m0));
            else if (w0 == w1) c = __popc(bitmap[w0] & m0 & m1);
            else {
                c = __popc(bitmap[w0] & m0);
                for (uint64_t w = w0 + 1; w < w1; ++w) c += __popc(bitmap[w]);
                c += __popc(bitmap[w1] & m1);
            }
        }
        if (coop) __builtin_amdgcn_wave_barrier();                                      // (the prefix is rewritten by the next stretch)
        if (in) cov[v] = c;
    }
}

__global__ void __launch_bounds__(256) count_nonzero_words_kernel(const uint32_t *__restrict__ p, uint64_t n, unsigned long long *__restrict__ out) {
    unsigned long long c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) c += p[i] != 0u;
    if (c) atomicAdd(out, c);
}

// The part of the coverage pass that depends on the binning only -- zero-filling the result arena and the walk sums of
// long reads: the resident step issues it while the trio index is still being built on the side stream.
int coverage_prepare(Ctx *ctx, Db *db, Reads *rd, bool with_trio) {
    // one arena, one memset: [bases V u64][trio_bases U u64][abort u64][bitmap words u32][full-node flags: 1 bit per node, padded by a window]
    const CovArenaLayout a = cov_arena_layout(db->V, with_trio ? db->U : 0, db->L);
    const size_t off_trio = a.off_trio, off_bm = a.off_bm, off_full = a.off_full, total = a.total;
    PTX_HIP(ctx, db->d_cov_arena.alloc(total));
    uint8_t *base = db->d_cov_arena.p;
    db->d_bases.view(base, db->V);
    db->d_trio_bases.view(base + off_trio, a.n_trio);
    db->d_abort = reinterpret_cast<unsigned long long *>(base + a.off_abort);
    db->d_bitmap.view(base + off_bm, a.words);
    db->d_full.view(base + off_full, a.fwords);
    // (d_cov is allocated by the pass that writes it -- popcount_kernel below, node_stats_launch: a resident step on the fused node pass has none)
    // the resident step's last readers, or its fill on the side stream, left the arena zeroed unless its layout or place changed since (the signature):
    // only the abort counter is reset
    const uint64_t sig = (uint64_t)(uintptr_t)base ^ ((uint64_t)total * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)off_bm << 1) ^ ((uint64_t)off_full << 2) ^ (uint64_t)off_trio;
    const CovPrepare todo = db->cov.prepare_begun(sig, total);
    if (todo.wait_side_fill) PTX_HIP(ctx, hipStreamWaitEvent(ctx->stream, db->ev_cov_clean, 0));   // (coverage_arena_clean_async): over before anything here touches the arena
    if (todo.skip_fill) {
        if (ctx->cfg.cov_arena_verify) {
            DevBuf<unsigned long long> d_nz;
            PTX_HIP(ctx, d_nz.alloc(1));
            PTX_HIP(ctx, hipMemsetAsync(d_nz.p, 0, 8, ctx->stream));
            PTX_HIP(ctx, hipMemsetAsync(db->d_abort, 0, 8, ctx->stream));
            hipLaunchKernelGGL(count_nonzero_words_kernel, dim3(grid_for(total / 4, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, reinterpret_cast<const uint32_t *>(base), (uint64_t)(total / 4), d_nz.p);
            unsigned long long nz = 0;
            PTX_TRY(download(ctx, &nz, d_nz.p, 1));
            PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (nz) return fail(ctx, PANTAX_HIP_E_STATE, "coverage_prepare: %llu non-zero words in an arena its last readers should have left clean", nz);
        }
        PTX_HIP(ctx, hipMemsetAsync(db->d_abort, 0, 8, ctx->stream));
    } else {
        KTimer t(ctx, "zero_fill_kernel");   // (the arena's fill is a kernel of the step like any other: timed with them)
        PTX_TRY(zero_fill(ctx, base, total));
    }
    if (rd->R && rd->T_pad && rd->n_long && rd->state.long_sums_from(db->uid)) {
        // the binning pass of these reads against THIS db took the walk sums on its way (bin_slots_kernel, round 6)
    } else if (rd->R && rd->T_pad && rd->n_long) {
        PTX_HIP(ctx, hipMemsetAsync(rd->d_long_sum.p, 0, rd->R * sizeof(uint32_t), ctx->stream));
        KTimer t(ctx, "walk_sum_kernel");
        const bool eager = (uint64_t)rd->n_long * 2 > rd->n_slots;      // most walks are long: one dependent level less (0.363 -> 0.333 ms at the cfg5 share)
        hipLaunchKernelGGL((eager ? walk_sum_kernel<4, true> : walk_sum_kernel<4, false>), dim3(grid_for(rd->T_pad / 4 + 1, 256, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, rd->T_pad, rd->d_g_group_slot.p,
                           rd->d_g_step_dup.p, rd->d_g_read_rec.p, rd->d_g_slot_rec.p, rd->d_g_node_id.p, db->d_node_len.p, rd->d_long_sum.p,
                           rd->d_long_len0.p);
    }
    PTX_HIP(ctx, hipGetLastError());
    db->cov.prepare_finished();
    return 0;
}

// The resident step's zero fill of the coverage arena, taken off the main stream (round 6): enqueued on the side stream behind everything the main stream
// holds so far (the arena's last readers among it), it runs beside what the main stream gets next -- strain_enqueue calls it in front of the LPs, one
// workgroup per species, which leave most of the memory system idle (behind the node statistics, i.e. beside the row sort's bandwidth-bound passes: no
// gain; in two bursts, one beside the sort's sampling kernels: less gain; behind the LPs: a third of the gain; at the start of the NEXT step beside its binning
// pass, which waits for gathers at 0.3 of the HBM rate: the same 0.3 ms as here -- a streaming fill slows a latency-bound neighbour by what it takes).  The next coverage_prepare waits for
// ev_cov_clean.
int coverage_arena_clean_async(Ctx *ctx, Db *db) {
    if (!db->d_cov_arena.p || !db->cov.arena_bytes() || !ctx->stream2) return 0;
    uint8_t *f_ptr = db->d_cov_arena.p;
    const size_t f_n = db->cov.arena_bytes();
    if (!db->ev_cov_read) PTX_HIP(ctx, hipEventCreateWithFlags(&db->ev_cov_read, hipEventDisableTiming));
    if (!db->ev_cov_clean) PTX_HIP(ctx, hipEventCreateWithFlags(&db->ev_cov_clean, hipEventDisableTiming));
    PTX_HIP(ctx, hipEventRecord(db->ev_cov_read, ctx->stream));
    PTX_HIP(ctx, hipStreamWaitEvent(ctx->stream2, db->ev_cov_read, 0));
    int rc;
    hipError_t e;
    {
        SideStream side(ctx);
        if (!side) return fail(ctx, PANTAX_HIP_E_STATE, "coverage arena fill: the ctx is already on its side stream");
        rc = zero_fill(ctx, f_ptr, f_n);
        e = hipEventRecord(db->ev_cov_clean, ctx->stream2);
    }
    db->cov.invalidated();          // the arena no longer holds a coverage result, whether the fill went out whole or not
    if (rc != 0) return rc;
    PTX_HIP(ctx, e);
    db->cov.side_fill_enqueued();
    return 0;
}

// ---- coverage_launch: its stopwatch and its phases, in the order it calls them
// (the stage call of the file seam under hip_trace: where its milliseconds go)
struct CovLap {
    Ctx *ctx;
    bool on;
    std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!on) return;
        (void)hipStreamSynchronize(ctx->stream);
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[node_coverage]        %-28s %9.3f ms\n", what, std::chrono::duration<double, std::milli>(now - prev).count());
        prev = now;
    }
};

// the `active` table of the select-only kernels, which load the flag unconditionally: all ones when no species is deselected
static int active_flags(Ctx *ctx, Db *db, const uint8_t *d_active, const uint8_t **out) {
    if (!d_active) {
        if (db->d_ones.n < db->S) { PTX_HIP(ctx, db->d_ones.alloc(db->S)); PTX_HIP(ctx, hipMemsetAsync(db->d_ones.p, 1, db->S, ctx->stream)); }
        d_active = db->d_ones.p;
    }
    *out = d_active;
    return 0;
}

// Only the items whose node block meets the id range of one of the db's species hold reads of its species (round 6: the file seam runs a selection
// group by group over the same resident reads -- a read that starts outside every range is "U" for this db, and streaming its steps only to
// find that out cost a group of a quarter of the species 6 ms where the whole selection as one db took 8).  Every read of an item starts inside
// the item's block.  The groups of the seam are contiguous in the order of the species TABLE (by abundance), not of the ids: the items are
// picked species by species into a list (a few hundred KB), not as one range (cov_item_select).  The list is made once per db and reads layout.
struct ItemList { uint32_t n; const uint32_t *d; };   // d null: items 0 .. n - 1
static int item_selection(Ctx *ctx, Db *db, const Reads *rd, ItemList *out) {
    *out = {rd->n_items, nullptr};
    if (db->item_sel_layout == rd->layout_id && rd->layout_id != 0) {        // the list made for these reads' layout by an earlier pass of this db
        *out = {db->item_sel_n, db->item_sel_on ? db->d_item_sel.p : nullptr};
    } else if (rd->h_item_block.size() == rd->n_items && rd->item_blk_shift > 0 && db->S && !db->h_range_start.empty()) {
        const CovItemSel s = cov_item_select(rd->h_item_block, rd->item_blk_shift, db->h_range_start, db->h_range_end);
        if (s.on && s.n_sel) PTX_TRY(upload(ctx, db->d_item_sel, s.sel.data(), s.sel.size()));
        *out = {s.n_sel, s.on && s.n_sel ? db->d_item_sel.p : nullptr};
        db->item_sel_layout = rd->layout_id; db->item_sel_n = s.n_sel; db->item_sel_on = s.on;
    }
    return 0;
}

// what the two uses of coverage_fast_kernel pass differently: the short-read one its work items, LONG the walk sums and its cuts of the stream
struct CovFastTail {
    const uint2 *items; int blk_shift; const uint32_t *long_sum, *long_len0; uint32_t only_long, chunk_groups, total_groups, win_back; const uint32_t *item_sel;
};
template <int U, int PASSES, int WIN, bool LONG>
static void fast_launch_as(Ctx *ctx, Db *db, Reads *rd, const uint8_t *d_act, bool trio, int grid, const CovFastTail &t) {
    if (grid <= 0) return;
    const auto kernel = trio ? coverage_fast_kernel<true, U, PASSES, WIN, LONG> : coverage_fast_kernel<false, U, PASSES, WIN, LONG>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(COV_BLOCK), cov_lds_bytes(WIN), ctx->stream, t.items, rd->d_g_group_slot.p, rd->d_g_read_rec.p,
                       rd->d_g_slot_rec.p, rd->d_g_node_id.p, rd->d_g_step_dup.p, d_act, db->d_node_rec.p, db->d_bit_off.p, db->V, db->d_bases.p,
                       db->d_bitmap.p, db->d_full.p, db->d_trio_ent.p, db->d_trio_bases.p, db->d_abort, ctx->cfg.cov_ablate /* -DCOV_ABLATE builds only */,
                       t.blk_shift, t.long_sum, t.long_len0, t.only_long, t.chunk_groups, t.total_groups, t.win_back, t.item_sel,
                       ctx->cfg.cov_spec == "miss" ? 1u : 0u /* tests: every wave of the short-read kernel takes the fallback loads */);
}

// Walks of <= 64 steps: the short-read kernel, one wave per 64-step group, PASSES groups per wave and workgroup (the LDS windows are zeroed and flushed
// once per workgroup).  Groups in flight per wave, rounds per workgroup, nodes in the LDS window: 2 x 4 groups (2048 steps); 2 x 8 (4096 steps) on
// streams of 2^28 steps and more, where a workgroup's start-up chain costs more (measured: 0.711 vs 0.768 ms at 8e7 steps, 11.7 vs 9.8 ms at 8e8).  The
// window: 2304 nodes since round 5 -- an item's reads start inside one block of 2048 ids and the window begins 64..127 nodes in front of it, so 2304
// hold every short read; the 3072 of rounds 3-4 cost 23.5 KB of LDS per workgroup = SIX waves per SIMD where the registers allow eight (19.7 KB:
// eight).  The kernel waits for its gathers two thirds of the time: 6.46 -> 5.77 ms at 1e8 reads, 0.708 -> 0.639 at 1e7 (2048 nodes: 7.3 / 0.77,
// the reads at a block's end fall off the window)
static int fast_launch(Ctx *ctx, Db *db, Reads *rd, const uint8_t *d_act, bool trio, const CovFastShape &f, const ItemList &list) {
    const CovFastTail t{rd->d_g_items.p, rd->item_blk_shift, nullptr, nullptr, 0u, 0u, 0u, 0u, list.d};
    const int grid = (int)list.n;
    const auto is = [&](int u, int passes, int win) { return f.u == u && f.passes == passes && f.win == win; };
    if (is(1, 8, 2048)) fast_launch_as<1, 8, 2048, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(2, 4, 2048)) fast_launch_as<2, 4, 2048, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(2, 8, 2048)) fast_launch_as<2, 8, 2048, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(2, 8, 3072)) fast_launch_as<2, 8, 3072, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(2, 8, 4096)) fast_launch_as<2, 8, 4096, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(2, 4, 3072)) fast_launch_as<2, 4, 3072, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(2, 8, 2304)) fast_launch_as<2, 8, 2304, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(2, 8, 2560)) fast_launch_as<2, 8, 2560, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(2, 4, 2304)) fast_launch_as<2, 4, 2304, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(2, 4, 2560)) fast_launch_as<2, 4, 2560, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(1, 8, 2304)) fast_launch_as<1, 8, 2304, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(4, 4, 2304)) fast_launch_as<4, 4, 2304, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(4, 4, 2048)) fast_launch_as<4, 4, 2048, false>(ctx, db, rd, d_act, trio, grid, t);
    else if (is(4, 4, 3072)) fast_launch_as<4, 4, 3072, false>(ctx, db, rd, d_act, trio, grid, t);
    else return fail(ctx, PANTAX_HIP_E_STATE, "coverage_launch: no short-read kernel of shape U = %d, PASSES = %d, WIN = %d", f.u, f.passes, f.win);
    return 0;
}

// Groups that hold steps of longer walks (HiFi / ONT reads; cov_general: every group -- measurements, and the tests force it): round 6's select-only body
// (coverage_fast_kernel<.., LONG>) over plain cuts of the stream.  Default shape: 2 groups in flight per wave, 64 groups (4096 steps) per workgroup, a
// 3072-node window that begins 1024 nodes in front of the first live step (reverse-strand walks run down from their first node)
static int long_launch(Ctx *ctx, Db *db, Reads *rd, const uint8_t *d_act, bool trio, const CovPlan &plan) {
    if (!rd->d_long_sum.p) { PTX_HIP(ctx, rd->d_long_sum.alloc(rd->R)); PTX_HIP(ctx, rd->d_long_len0.alloc(rd->R)); }   // (cov_general over short reads: never read)
    const CovLongShape &l = plan.lng;
    const uint32_t total_groups = (uint32_t)(rd->T_pad / 64);
    const int grid = (int)((total_groups + l.chunk_groups - 1) / l.chunk_groups);
    const CovFastTail t{nullptr, 0, rd->d_long_sum.p, rd->d_long_len0.p, plan.only_long ? 1u : 0u, l.chunk_groups, total_groups, l.win_back, nullptr};
    if (l.u == 1 && l.win == 2048) fast_launch_as<1, 1, 2048, true>(ctx, db, rd, d_act, trio, grid, t);
    else if (l.u == 1 && l.win == 3072) fast_launch_as<1, 1, 3072, true>(ctx, db, rd, d_act, trio, grid, t);
    else if (l.u == 1 && l.win == 4096) fast_launch_as<1, 1, 4096, true>(ctx, db, rd, d_act, trio, grid, t);
    else if (l.u == 2 && l.win == 2048) fast_launch_as<2, 1, 2048, true>(ctx, db, rd, d_act, trio, grid, t);
    else if (l.u == 2 && l.win == 4096) fast_launch_as<2, 1, 4096, true>(ctx, db, rd, d_act, trio, grid, t);
    else if (l.u == 2 && l.win == 3072) fast_launch_as<2, 1, 3072, true>(ctx, db, rd, d_act, trio, grid, t);
    else return fail(ctx, PANTAX_HIP_E_STATE, "coverage_launch: no long-walk kernel of shape U = %d, WIN = %d", l.u, l.win);
    return 0;
}

// node_base_cov of the stage call (the resident step leaves it to the node statistics pass: defer_count)
static int count_launch(Ctx *ctx, Db *db) {
    PTX_HIP(ctx, db->d_cov.alloc(db->V));
    db->node_cov = Db::NodeCov::replaced;                        // (no longer the counts of a resident step: pantax_hip_strain_node_cov)
    KTimer t(ctx, "popcount_kernel");
    if (long_node_shape(db->L, db->V, ctx->cfg.ncs_prefix_min, ctx->cfg.ncs_no_prefix))
        hipLaunchKernelGGL(popcount_long_kernel, dim3(grid_for((db->V + 63) / 64, 4, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, db->V,
                           db->d_bit_off.p, db->d_full.p, db->d_bitmap.p, db->d_cov.p);
    else
        hipLaunchKernelGGL(popcount_kernel, dim3(grid_for(db->V, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, db->V,
                           db->d_bit_off.p, db->d_full.p, db->d_bitmap.p, db->d_cov.p);
    return 0;
}

int coverage_launch(Ctx *ctx, Db *db, Reads *rd, const uint8_t *d_active, bool with_trio, bool defer_count) {
    if (!rd->state.grouped()) return fail(ctx, PANTAX_HIP_E_STATE, "node_coverage: these reads are a slice kept as plain columns (to be routed to their owner), not resident reads");
    const bool trace = ctx->cfg.trace && !defer_count;
    CovLap lap{ctx, trace};
    if (db->cov.launch_needs_prepare()) PTX_TRY(coverage_prepare(ctx, db, rd, with_trio));
    lap("arena + zero fill");
    db->cov.launch_begun();
    db->trio.free_event_void();    // a reader of the unique-trio tables goes onto the stream: the event of an earlier strain step no longer covers them
    const bool trio = with_trio && db->U;
    const uint8_t *d_act_fast = d_active;
    if (rd->R && rd->T_pad) PTX_TRY(active_flags(ctx, db, d_active, &d_act_fast));
    const CtxConfig &cfg = ctx->cfg;
    const CovPlan plan = cov_plan(rd->T_pad, rd->n_long, rd->n_slots, rd->n_items, rd->R, cfg.cov_general, cfg.cov_long, cfg.covf_shape, cfg.covl_shape,
                                  cfg.cov_shape, cfg.cov_xcd);
    if (plan.run_fast) {
        KTimer t(ctx, "coverage_fast_kernel");
        ItemList list;
        PTX_TRY(item_selection(ctx, db, rd, &list));
        if (trace) std::fprintf(stderr, "[node_coverage]        %u of %u items launched\n", list.n, rd->n_items);
        PTX_TRY(fast_launch(ctx, db, rd, d_act_fast, trio, plan.fast, list));
    }
    if (plan.run_long) {
        KTimer t(ctx, "coverage_long_kernel");
        PTX_TRY(long_launch(ctx, db, rd, d_act_fast, trio, plan));
    }
    if (plan.run_step) {   // round 5's kernel for the groups of longer walks (measurements, and the tests compare the two); it tests d_active for null itself
        KTimer t(ctx, "coverage_step_kernel");
        PTX_TRY(coverage_step_launch(ctx, db, rd, d_active, trio, plan));
    }
    PTX_HIP(ctx, hipGetLastError());
    lap("coverage kernels");
    if (db->V && !defer_count) PTX_TRY(count_launch(ctx, db));
    PTX_HIP(ctx, hipGetLastError());
    lap("popcount");
    db->cov.launch_finished(defer_count && db->V != 0);   // (deferred, the resident step: node_stats_launch counts the covered bases in its own pass, or the fused node pass)
    return 0;
}

}  // namespace ptx
