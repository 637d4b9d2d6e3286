// stage_cov_step.hip -- round 5's coverage kernel for the groups that hold steps of walks of more than 64 steps (option cov_long=step; kept for
// measurements, and the tests compare it with coverage_fast_kernel<.., LONG>).  Semantics: the header of stage_cov.hip.
#include "common.hpp"
#include "cov_plan.hpp"
#include "cov_device.hpp"
#include "wave.hpp"

namespace ptx {

// Steps arrive grouped by the locus of their read's first node (build_step_read below), so a workgroup's
// chunk of consecutive steps lands in a narrow node window: `bases` is accumulated in an LDS
// window of COV_WIN nodes (32-bit LDS atomics) and flushed with one 64-bit global atomic per touched
// node -- the LDS-staged segmented reduction of the scatter.  Nodes outside the window (or oversized
// lengths) fall back to the global atomic; the result is identical either way.
//
// The kernel is bound by instruction issue and by the latency of its chain of dependent gathers, so
//   * the chain is three levels: {slot, node id, step code} (stream) -> {read record (16 B), slot record (8 B)} -> {node record}
//     (-> a unique-trio entry where the node has any).  The slot record {species, node base - first id} is written by the
//     binning pass; a binned walk lies inside its species' range and db_upload makes the range span exactly the graph, so a
//     step places its node with ONE add and no range test; the node record carries the lookup head of the unique-trio index (first row, #rows)
//     next to bit offset and length, and a 3-window takes the head of its middle node from the lane below:
//     ONE divergent 16-byte gather per step.  Everything is in global node indices (the lookup entries too).
//   * a step that covers its whole node (every interior step of a read: profile.rs:860-862 with :870-873) sets ONE flag for
//     the node instead of marking its bits word by word (popcount_kernel then takes the node's length); only the partial
//     ranges -- first and last step of a read -- are marked in the bit window, in 32-bit positions relative to the window.
//   * every wave works on U groups of 64 steps at once: the loads of one level are issued for all U groups before the
//     first of them is waited for (U x the memory-level parallelism per wave; registers permitting).
// PASSES such rounds share one set of LDS windows (zeroing and flushing them is per workgroup).  Workgroups are handed to
// the XCDs round-robin by the dispatcher; XCD_MAP makes every XCD walk ONE contiguous eighth of the stream, so neighbouring
// chunks -- which share the node records and bitmap lines at their seam -- meet in the same L2.
template <bool WITH_TRIO, int U, int PASSES>
__global__ void __launch_bounds__(COV_BLOCK) coverage_step_kernel(
    uint64_t T, const uint32_t *__restrict__ group_slot, const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
    const uint32_t *__restrict__ node_id, const uint8_t *__restrict__ step_dup, const uint8_t *__restrict__ active,
    const uint4 *__restrict__ node_rec, unsigned long long *__restrict__ bases, uint32_t *__restrict__ bitmap, uint32_t *__restrict__ full,
    const uint2 *__restrict__ trio_ent, unsigned long long *__restrict__ trio_bases, unsigned long long *__restrict__ n_abort,
    const uint32_t *__restrict__ long_sum, const uint32_t *__restrict__ long_len0, uint32_t n_chunks, uint32_t xcd_map, uint32_t ablate,
    uint32_t only_long /* 1: groups without a step of a longer walk belong to coverage_fast_kernel */) {
    constexpr int CHUNK = COV_BLOCK * U * PASSES;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t chunk = blockIdx.x;
    if (xcd_map) {   // blockIdx -> XCD is round-robin over 8: XCD x takes chunks [x * per, (x + 1) * per)
        const uint32_t per = (n_chunks + 7) / 8;
        chunk = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
        if ((blockIdx.x >> 3) >= per || chunk >= n_chunks) return;
    }
    const uint64_t chunk_b = (uint64_t)chunk * CHUNK;
    uint64_t chunk_e = chunk_b + CHUNK;
    if (chunk_e > T) chunk_e = T;
    for (int i = threadIdx.x; i < (int)(cov_lds_bytes(COV_WIN) / 4); i += COV_BLOCK) s_cov[i] = 0;
    // window base: the node of the first live step among a few probes of the chunk.  Every thread computes it
    // (workgroup-uniform addresses), so nobody waits on a broadcast and the probes overlap the first gathers.
    uint32_t wlo = 0, win_n = 0;
    uint64_t bw0 = 0, bit0 = 0;
    uint32_t bwn = 0;
#pragma unroll
    for (int c = 0; c < CHUNK / COV_BLOCK; ++c) {
        const uint64_t tc = chunk_b + (uint64_t)c * COV_BLOCK;
        if (win_n == 0 && tc < chunk_e) {
            const uint32_t slot = group_slot[tc >> 6];          // tc is a multiple of 64: the read that owns the group's first step
            if (slot != NO_SLOT) {
                const uint2 sr0 = slot_rec[slot];
                if ((int)sr0.x >= 0 && !(active && !active[sr0.x])) {
                    const uint32_t v0 = node_id[tc] + sr0.y;
                    wlo = (v0 > (uint32_t)COV_WIN_BACK ? v0 - COV_WIN_BACK : 0u) & ~63u;
                    win_n = COV_WIN;
                    bw0 = nr_bit_off(node_rec[wlo]) >> 5;        // bit window starts at the window's first node
                    bit0 = bw0 << 5;
                    bwn = COV_BWIN;
                }
            }
        }
    }
    __syncthreads();
    // the stream loads of round r + 1 are requested at the top of round r, as in the short-read kernel (-DCOV_NO_PREFETCH: the round-4 loop)
#ifndef COV_NO_PREFETCH
    uint32_t n_id[U], n_dupc[U], n_gs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t t = chunk_b + (uint64_t)(wave * U + u) * 64 + lane;
        const uint64_t tc = t < chunk_e ? t : chunk_b;              // (in range; dead lanes of a round are masked by `ok`)
        n_id[u] = node_id[tc]; n_dupc[u] = step_dup[tc]; n_gs[u] = group_slot[tc >> 6];
    }
#endif
#pragma unroll 1
    for (int pass = 0; pass < PASSES; ++pass) {
        const uint64_t wbase = chunk_b + (uint64_t)((pass * (COV_BLOCK / 64) + wave) * U) * 64;   // this wave's U x 64 consecutive steps
        if (wbase >= chunk_e) break;
        // ---- level 1: the stream
        uint32_t slot[U], id[U], dupc[U], ti[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t t = wbase + (uint64_t)u * 64 + lane;
            ok[u] = t < chunk_e;                                     // whole groups: T_pad and the chunk size are multiples of 64
            slot[u] = NO_SLOT; id[u] = 0; dupc[u] = STEP_PAD;
            ti[u] = (uint32_t)t;                                     // T_pad < 2^32 (build_step_read)
#ifndef COV_NO_PREFETCH
            uint32_t gs_now = NO_SLOT;
            if (ok[u]) { id[u] = n_id[u]; dupc[u] = n_dupc[u]; gs_now = n_gs[u]; }
            {
                const uint64_t tn = t + (uint64_t)COV_BLOCK * U;    // the same lane's step in the coming round
                const uint64_t tc = (pass + 1 < PASSES && tn < chunk_e) ? tn : chunk_b;
                n_id[u] = node_id[tc]; n_dupc[u] = step_dup[tc]; n_gs[u] = group_slot[tc >> 6];
            }
            const uint32_t gs = gs_now;
#else
            if (ok[u]) { id[u] = node_id[t]; dupc[u] = step_dup[t]; }
            const uint32_t gs = ok[u] ? group_slot[t >> 6] : NO_SLOT;
#endif
            const uint32_t sl = slot_in_group(gs, dupc[u], lane);
            ok[u] = ok[u] && dupc[u] != STEP_PAD;
            if (only_long && !__any(ok[u] && (dupc[u] & STEP_LONG))) ok[u] = false;   // a short-read group: the other kernel's
            if (ok[u]) slot[u] = sl;
        }
        // ---- level 2: per-read records
        uint4 rr[U];
        uint2 sr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            rr[u] = make_uint4(0u, 0u, 0u, 0u); sr[u] = make_uint2(0xFFFFFFFFu, 0u);
            if (ok[u]) { rr[u] = read_rec[slot[u]]; sr[u] = slot_rec[slot[u]]; }
        }
        // ---- level 3: the node record (issued before the species' `active` flag is known: a wasted gather at worst)
        uint4 nr[U];
        uint32_t v[U], act[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = ok[u] && (int)sr[u].x >= 0;                       // "U" / dropped rows
            nr[u] = make_uint4(0u, 0u, 0u, 0u); v[u] = 0; act[u] = 1u;
            if (ok[u]) {
                v[u] = id[u] + sr[u].y;
                nr[u] = node_rec[v[u]];
                if (active) act[u] = active[sr[u].x];
            }
        }
        // ---- shuffles, the trio lookup head and the first trio entry (level 4), for all groups
        uint32_t v1[U], v2[U], len0[U], tlo[U], thi[U];
        uint2 th[U];
        uint2 e0[U], e1[U];   // the first TWO lookup entries of the head: with one, 95 % of the waves held a lane whose window was
                              // the node's second entry (8 % of the visits meet a head of two or more) and paid another dependent gather
        int dist[U];
        bool cross[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (ok[u] && !act[u]) ok[u] = false;                      // unselected species
            if (!ok[u]) { v[u] = 0; nr[u] = make_uint4(0u, 0u, 0u, 0u); }
            const uint32_t b = rr[u].x;
            const uint32_t i = ok[u] ? ti[u] - b : 0u;
            dist[u] = ok[u] ? (int)min(i, (uint32_t)lane) : 0;        // earlier steps of my read held by lower lanes
            cross[u] = ok[u] && (int)i > lane;                        // the walk began before this wave (more than 64 steps)
            // neighbours one and two lanes down: DPP wave shifts (VALU), not LDS-crossbar shuffles
            v1[u] = wave_shr1(v[u]); v2[u] = wave_shr1(v1[u]);
            const uint32_t tf1 = wave_shr1(nr[u].w), ty1 = wave_shr1(nr[u].y);
            th[u] = make_uint2(0u, 0u); tlo[u] = 0; thi[u] = 0; e0[u] = make_uint2(0u, 0u); e1[u] = make_uint2(0u, 0u);
            if (WITH_TRIO && !ABL(4u) && ok[u] && i >= 2) {
                if (lane < 1) v1[u] = node_id[b + i - 1] + sr[u].y;
                if (lane < 2) v2[u] = node_id[b + i - 2] + sr[u].y;
                // canonical window (min end, middle, max end); the lookup rows are filed under the MIDDLE node (the lane below), keyed by the two ends
                tlo[u] = min(v[u], v2[u]); thi[u] = max(v[u], v2[u]);
                uint32_t hy = ty1;
                if (lane >= 1) th[u].x = tf1;
                else { const uint4 r1 = node_rec[v1[u]]; th[u].x = r1.w; hy = r1.y; }   // wave border of a long walk
                th[u].y = (nr_filter(hy) & nr_pair_bit(tlo[u], thi[u])) ? nr_rows(hy) : 0u;   // the pair filter: nothing is fetched for a window whose bit is clear
                if (th[u].y) {
                    const EntPair ep = *reinterpret_cast<const EntPair *>(trio_ent + th[u].x);   // two entries, one load (one entry of slack behind the last row)
                    e0[u] = make_uint2(ep.a, ep.b); e1[u] = make_uint2(ep.c, ep.d);
                }
            }
            // first node length: from the lane that holds step b, else (long walk) noted by walk_sum_kernel
            const uint32_t nl_src = __shfl(nr[u].z, lane - dist[u]);
            len0[u] = nr[u].z;
            if (ok[u] && i > 0) len0[u] = !cross[u] ? nl_src : long_len0[slot[u]];
        }
        // ---- per group: aligned lengths, bitmap, bases, trio bases
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t b = rr[u].x, k = rr[u].y, ps = rr[u].z, pe = rr[u].w;
            // positions, node lengths and aligned lengths are 32-bit quantities (the packed layout carries u32 columns and a
            // walk cannot align 4 Gbp): only `target` needs a sign.
            const uint32_t i = ok[u] ? ti[u] - b : 0u;
            const uint64_t bo = nr_bit_off(nr[u]);
            const uint32_t nl = nr[u].z;
            const uint64_t rel = bo - bit0;                           // the node inside the LDS bit window: 32-bit relative positions
            const bool in_win = rel < (uint64_t)bwn * 32 && nl <= (uint64_t)bwn * 32 - rel;   // (a node that starts below the window wraps to a huge rel)
            bool live = ok[u];
            uint32_t mfull = NO_FULL;                                 // the node this step covers whole (its flag is set below, by the whole wave)
            const long long target = (long long)pe - (long long)ps;   // profile.rs:800
            if (live && k == 1) {                                     // :811
                if (target >= 0) {                                    // :821-827
                    if (target && !ABL(2u)) add_bases(bases, wlo, win_n, v[u], (uint32_t)target);
                    if (ps < pe && pe <= nl && !ABL(1u)) {            // :832
                        if (ps == 0 && pe == nl) { if (!ABL(8u)) mfull = v[u]; }
                        else if (ABL(16u)) {}
                        else if (in_win) mark_window(COV_WIN, (uint32_t)rel + ps, (uint32_t)rel + pe);
                        else mark_range(bitmap, COV_WIN, bw0, bwn, bo + ps, bo + pe);
                    }
                }
                live = false;
            }
            if (live && ps > len0[u]) {                               // assert :854 -> whole read contributes nothing
                if (i == 0) atomicAdd(n_abort, 1ull);
                live = false;
            }
            // ---- `seen` before this step = sum of the aligned lengths of steps 0..i-1 of MY read: a plain wave prefix sum (DPP)
            // minus its value at the lane that holds step 0 -- the steps of a read sit in consecutive lanes (mod 2^32 like the adds)
            const uint32_t contrib = live ? (i == 0 ? nl - ps : nl) : 0u;
            const int dst = dist[u];
            const uint32_t pexcl = wave_incl_scan_dpp(contrib) - contrib;
            const uint32_t seen_in_wave = pexcl - __shfl(pexcl, lane - dst);
            // ---- first occurrence of this node in the read (:879): decided at upload time (step codes above)
            const uint32_t id0 = __shfl(id[u], lane - dst);           // id of step 0 when the walk starts in this wave
            uint32_t rl = 0;
            if (live) {
                int jf = -1;                                          // -1: first occurrence; 0: the node of step 0; 1: another earlier step
                if (dupc[u] & STEP_LONG) { if (dupc[u] & 1u) jf = (id[u] == (cross[u] ? node_id[b] : id0)) ? 0 : 1; }
                else if (dupc[u] & STEP_DIST) jf = (int)i - (int)(dupc[u] & STEP_DIST);
                uint32_t aln, sidx;
                if (i == 0) { aln = nl - ps; sidx = ps; }             // :853-856
                else if (i == k - 1) {                                // :857-859
                    uint32_t seen = seen_in_wave;
                    if (cross[u]) seen = long_sum[slot[u]] - ps;      // all steps but the last, from walk_sum_kernel
                    aln = target > (long long)seen ? (uint32_t)(target - (long long)seen) : 0u;   // max(target - seen, 0)
                    sidx = 0;
                } else { aln = nl; sidx = 0; }                        // :860-862
                uint32_t hi = sidx + aln;
                if (hi > nl) hi = nl;                                 // :871
                if (ABL(1u)) {}
                else if (sidx == 0 && hi == nl) { if (nl && !ABL(8u)) mfull = v[u]; }
                else if (ABL(16u)) {}
                else if (in_win) mark_window(COV_WIN, (uint32_t)rel + sidx, (uint32_t)rel + hi);
                else mark_range(bitmap, COV_WIN, bw0, bwn, bo + sidx, bo + hi);
                if (jf < 0) {
                    rl = aln;
                    if (aln && !ABL(2u)) add_bases(bases, wlo, win_n, v[u], aln);     // :881
                } else rl = (jf == 0) ? (len0[u] - ps) : nl;
            }
            mark_full_wave(full, wlo, win_n, mfull);
            if (WITH_TRIO) {                                          // :890-907
                uint32_t rl1 = wave_shr1(rl), rl2 = wave_shr1(wave_shr1(rl));
                if (live && i >= 2 && !ABL(4u)) {
                    if (lane < 1) rl1 = rl_from_memory(i - 1, b, node_id, step_dup, sr[u].y, node_rec, len0[u], ps);
                    if (lane < 2) rl2 = rl_from_memory(i - 2, b, node_id, step_dup, sr[u].y, node_rec, len0[u], ps);
                    long long row = -1;                                      // a row IS its lookup entry: the index of the entry that matches
                    if (th[u].y) {
                        if (e0[u].x == tlo[u] && e0[u].y == thi[u]) row = (long long)th[u].x;
                        else if (th[u].y > 1 && e1[u].x == tlo[u] && e1[u].y == thi[u]) row = (long long)th[u].x + 1;
                        else
                            for (uint32_t j = 2; j < th[u].y; ++j) {
                                const uint2 e = trio_ent[th[u].x + j];
                                if (e.x == tlo[u] && e.y == thi[u]) { row = (long long)th[u].x + j; break; }
                            }
                    }
                    if (row >= 0) {
                        const unsigned long long sum = (unsigned long long)rl2 + rl1 + rl;
                        if (sum) atomicAdd(&trio_bases[row], sum);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (win_n) {
        for (int i = threadIdx.x; i < COV_WIN; i += COV_BLOCK) {
            const uint32_t c = S_WIN(i);
            if (c) atomicAdd(&bases[wlo + i], (unsigned long long)c);
            // full-node flags: the window starts at a multiple of 64 nodes, so a wave's ballot is two whole words of the flag vector
            const unsigned long long fb = __ballot(S_FULL(COV_WIN, i) != 0);
            if (fb && (lane & 31) == 0) {
                const uint32_t m = (uint32_t)(fb >> (lane & 32));
                if (m) atomicOr(&full[(wlo + i) >> 5], m);
            }
        }
    }
    for (uint32_t i = threadIdx.x; i < bwn; i += COV_BLOCK) {
        const uint32_t m = S_BM(COV_WIN, i);
        if (m) atomicOr(&bitmap[bw0 + i], m);     // nothing waits for these (a probe first would be a dependent round trip per word)
    }
}

template <int U, int PASSES>
static void step_launch_as(Ctx *ctx, Db *db, Reads *rd, const uint8_t *d_active, bool trio, const CovPlan &plan) {
    const uint32_t n_chunks = (uint32_t)((rd->T_pad + (uint64_t)COV_BLOCK * U * PASSES - 1) / ((uint64_t)COV_BLOCK * U * PASSES));
    const int grid = plan.xcd_map ? (int)(((n_chunks + 7) / 8) * 8) : (int)n_chunks;
    const auto kernel = trio ? coverage_step_kernel<true, U, PASSES> : coverage_step_kernel<false, U, PASSES>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(COV_BLOCK), cov_lds_bytes(COV_WIN), ctx->stream, rd->T_pad, rd->d_g_group_slot.p, rd->d_g_read_rec.p,
                       rd->d_g_slot_rec.p, rd->d_g_node_id.p, rd->d_g_step_dup.p, d_active, db->d_node_rec.p, db->d_bases.p, db->d_bitmap.p, db->d_full.p,
                       db->d_trio_ent.p, db->d_trio_bases.p, db->d_abort, rd->d_long_sum.p, rd->d_long_len0.p, n_chunks, plan.xcd_map, ctx->cfg.cov_ablate,
                       plan.only_long ? 1u : 0u);
}

// the groups of longer walks (plan.only_long) or every group through coverage_step_kernel<.., U, PASSES> of plan.step.  d_active: device [S] or null
int coverage_step_launch(Ctx *ctx, Db *db, Reads *rd, const uint8_t *d_active, bool trio, const CovPlan &plan) {
    const int u = plan.step.u, p = plan.step.passes;
    if (u == 2 && p == 2) step_launch_as<2, 2>(ctx, db, rd, d_active, trio, plan);
    else if (u == 2 && p == 1) step_launch_as<2, 1>(ctx, db, rd, d_active, trio, plan);
    else if (u == 4 && p == 1) step_launch_as<4, 1>(ctx, db, rd, d_active, trio, plan);
    else if (u == 4 && p == 2) step_launch_as<4, 2>(ctx, db, rd, d_active, trio, plan);
    else if (u == 1 && p == 8) step_launch_as<1, 8>(ctx, db, rd, d_active, trio, plan);
    else if (u == 1 && p == 4) step_launch_as<1, 4>(ctx, db, rd, d_active, trio, plan);
    else return fail(ctx, PANTAX_HIP_E_STATE, "coverage_step_launch: no kernel of shape U = %d, PASSES = %d", u, p);
    return 0;
}

}  // namespace ptx
