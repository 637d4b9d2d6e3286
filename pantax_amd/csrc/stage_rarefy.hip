// stage_rarefy.hip -- rarefaction of the strain fit (pantax_hip_strain_rarefy, the --strain-rarefy report): the L1 fit again on nested subsamples of the
// READS.  Not a stage of the reference.
//
// Contract (include/pantax_hip.h, DESIGN.md "Rarefaction of the strain fit"): read r belongs to level l of replicate b iff rarefy_depth(seed, b, r) >= l
// (rarefy_depth.hpp); bases_l[v] = the bases_per_node of the coverage pass over the reads of the level; every (replicate, level) is refitted as the
// bootstrap's replicate 0 on bases_l.
//
// Per replicate:
//   rarefy_depth_kernel   over the reads: min(depth, 255) as one byte per slot of the locus-grouped copy (d_slot_of) -- the main pass runs in slot order and
//                         never sees a read index.  5 bytes per read (4 read, 1 written at a scattered place);
// per pass (rarefy_plan.hpp: the levels [l0, l1) whose arrays of V u64 the device holds at once):
//   rarefy_bases_kernel   over the locus-grouped stream, a wave per 64-step group as the read passes of read_pass_device.hpp: the per-step aligned length
//                         of the coverage pass (coverage_fast_kernel, stage_cov.hip: the first-occurrence codes of d_g_step_dup, the wave's segmented
//                         prefix of node lengths, d_long_sum / d_long_len0 for walks of more than 64 steps) -- `bases` alone: no bit vector, no trio sums,
//                         no arena.  A step with aln > 0 adds it to bases[l][v] for l0 <= l < l1, l <= depth(slot): u64 atomics, the same bits in every
//                         order.  Level-major arrays: the refit's row source reads one level as a plain array of V.  A group none of whose slots
//                         reaches level l0 ends behind its slot records (half the groups' node gathers at l0 = 1).  Per (level, species) the counted reads
//                         and the added bases, reduced over the wave before the atomic.  Per step 5 bytes of stream, per slot 25 bytes of records, per
//                         live step 4 bytes of node length; expected atomics per step over the levels 1 .. : below one (sum of 2^-l).  (The levels of
//                         a node side by side, so that a step's adds share a line, took 1.8 times the time on cfg4: DESIGN.md);
// per entry:
//   the bootstrap's replicate 0 on the level's array (bootstrap_launch_on, boot_front.hpp: rows, radix sort, base patterns, lad_solve_kernel through
//   lad_args_launch, boot_objective_launch) and
//   rarefy_member_kernel  over the base patterns: per selected strain the rows with its bit (n_member) and the rows with its bit alone (n_only).
#include <algorithm>
#include <vector>
#include "common.hpp"
#include "boot_front.hpp"
#include "rarefy_depth.hpp"
#include "rarefy_plan.hpp"
#include "read_pass_device.hpp"

namespace ptx {

namespace {

__global__ void __launch_bounds__(256) rarefy_depth_kernel(uint64_t R, uint32_t n_slots, const uint32_t *__restrict__ slot_of, uint64_t replicate_hash,
                                                           uint8_t *__restrict__ depth_of_slot) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 256) {
        const uint32_t slot = slot_of[r];
        if (slot >= n_slots) continue;   // (~0: a read without a walk)
        depth_of_slot[slot] = (uint8_t)min(rarefy_depth_hashed(replicate_hash, r), 255u);
    }
}

struct RfyPass {
    uint32_t lb0, lb1;            // the levels with an array in `bases`: array l - lb0 holds level l
    uint32_t lc0;                 // the lowest level whose species counters this pass adds (lc0 <= lb0; the levels [lc0, lb1))
    uint32_t S;
    uint64_t V;
    unsigned long long *bases;    // [lb1 - lb0][V]
    unsigned long long *sp;       // [levels][S][2] = {counted reads, bases added}, indexed by the absolute level
    const uint8_t *serve;         // [S] the species the pass thins
};

__global__ void __launch_bounds__(256) rarefy_bases_kernel(uint32_t n_groups, uint32_t n_slots, const uint32_t *__restrict__ group_slot,
                                                           const uint8_t *__restrict__ step_code, const uint32_t *__restrict__ g_node_id,
                                                           const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                           const uint32_t *__restrict__ node_len, const uint32_t *__restrict__ long_sum,
                                                           const uint32_t *__restrict__ long_len0, const uint8_t *__restrict__ depth_of_slot, RfyPass P) {
    const int lane = threadIdx.x & 63;
    const uint32_t l_min = min(P.lb0, P.lc0);
    const auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * 4) {
        const uint32_t gs = group_slot[g];                                   // (wave-uniform) NO_SLOT: a group of pads only
        if (gs == RS_NO_SLOT) continue;
        const uint64_t t = (uint64_t)g * 64u + (uint64_t)lane;
        const uint32_t code = step_code[t];
        const uint32_t slot = slot_in_group(gs, code, lane);
        const bool live = code != STEP_PAD && slot < n_slots;
        uint4 rr = make_uint4(0u, 0u, 0u, 0u);
        uint2 sr = make_uint2(0xFFFFFFFFu, 0u);
        uint32_t depth = 0u;
        if (live) { rr = read_rec[slot]; sr = slot_rec[slot]; depth = depth_of_slot[slot]; }
        bool counted = live && (int32_t)sr.x >= 0;                           // drop flags and "U" reads stay out, as in the coverage pass
        if (counted) counted = P.serve[sr.x] != 0;
        if (__builtin_amdgcn_ballot_w64(counted && depth >= l_min) == 0ull) continue;   // (wave-uniform) no read of the group reaches the pass's levels
        const uint32_t v = counted ? g_node_id[t] + sr.y : 0u;
        const uint32_t nl = counted ? node_len[v] : 0u;
        const uint32_t i = live ? (uint32_t)t - rr.x : 0u;                   // position in the walk
        const uint32_t k = rr.y, ps = rr.z, pe = rr.w;
        const int dist = (int)min(i, (uint32_t)lane);                        // earlier steps of my walk held by lower lanes
        const bool cross = counted && i > (uint32_t)lane;                    // the walk began before this wave: more than 64 steps
        const uint32_t in_wave = __shfl(nl, lane - dist);
        uint32_t len0 = in_wave, lsum = 0u;
        if (cross) { len0 = long_len0[slot]; lsum = long_sum[slot]; }
        const bool single = k == 1u;
        const bool dead_read = !single && ps > len0;                         // the reference's assert: the whole read adds nothing
        const bool on = counted && !dead_read && !(single && pe < ps);
        // `seen` before this step = wave prefix sum of the walk's aligned lengths minus its value at the walk's first lane
        const uint32_t contrib = (on && !single) ? (i == 0u ? nl - ps : nl) : 0u;
        const uint32_t pexcl = wave_incl_scan_dpp(contrib) - contrib;
        uint32_t seen = pexcl - __shfl(pexcl, lane - dist);
        if (cross) seen = lsum - ps;                                         // (used by a walk's last step only) all steps but the last: walk_sum_kernel
        const uint32_t tgt = pe - ps;
        uint32_t aln = nl;
        if (i + 1u == k) aln = (pe >= ps && tgt > seen) ? tgt - seen : 0u;   // max(target - seen, 0)
        if (i == 0u) aln = single ? tgt : nl - ps;
        const bool earlier = (code & STEP_LONG) ? (code & 1u) != 0u : (code & STEP_DIST) != 0u;   // only the first occurrence of a node in a read adds
        const bool adds = on && !earlier && aln != 0u;
        if (adds)
            for (uint32_t l = P.lb0; l < P.lb1 && l <= depth; ++l) atomicAdd(&P.bases[(uint64_t)(l - P.lb0) * P.V + v], (unsigned long long)aln);
        // per (level, species): the counted reads (their first steps) and the bases added, species by species of the wave
        rs_species_rounds(counted, sr.x, [&](uint32_t s0, bool mine, unsigned long long) {
            for (uint32_t l = P.lc0; l < P.lb1; ++l) {                       // (wave-uniform)
                const bool in = mine && depth >= l;
                if (__builtin_amdgcn_ballot_w64(in) == 0ull) break;          // nested: nothing at the levels above either
                const unsigned long long nb = __builtin_amdgcn_ballot_w64(in && i == 0u);
                const unsigned long long sum = wave_reduce((in && adds) ? (unsigned long long)aln : 0ull, add);
                if (lane == 0) {
                    unsigned long long *const o = P.sp + ((uint64_t)l * P.S + s0) * 2u;
                    if (nb) atomicAdd(o, (unsigned long long)__popcll(nb));
                    if (sum) atomicAdd(o + 1, sum);
                }
            }
        });
    }
}

// per base pattern: its rows to n_member of every column of its mask, and to n_only of the column of a single-bit mask
__global__ void __launch_bounds__(256) rarefy_member_kernel(uint32_t n_pat, const uint64_t *__restrict__ pat_mask, const uint32_t *__restrict__ pat_start,
                                                            const uint32_t *__restrict__ pat_species, const uint64_t *__restrict__ sel_off,
                                                            unsigned long long *__restrict__ member /*[C][2]*/) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pat) return;
    const unsigned long long m = pat_mask[p], n = pat_start[p + 1] - pat_start[p];
    unsigned long long *const o = member + sel_off[pat_species[p]] * 2ull;
    const bool only = (m & (m - 1ull)) == 0ull;
    for (unsigned long long x = m; x; x &= x - 1ull) {
        const int k = __builtin_ctzll(x);
        atomicAdd(o + 2 * k, n);
        if (only) atomicAdd(o + 2 * k + 1, n);
    }
}

// the passes over the reads of one replicate: the depth bytes once, then a bases pass per range of levels
struct RfyReads {
    Ctx *ctx; Db *db; Reads *rd;
    DevBuf<uint8_t> d_depth, d_serve;
    int prepare(const std::vector<uint8_t> &serve) {
        PTX_TRY(upload(ctx, d_serve, serve.data(), serve.size()));
        PTX_HIP(ctx, d_depth.alloc(rd->n_slots ? rd->n_slots : 1));
        return 0;
    }
    int depths(uint64_t seed, uint32_t replicate) {
        PTX_HIP(ctx, hipMemsetAsync(d_depth.p, 0, rd->n_slots ? rd->n_slots : 1, ctx->stream));
        if (!rd->R || !rd->n_slots) return 0;
        KTimer tm(ctx, "rarefy_depth_kernel");
        hipLaunchKernelGGL(rarefy_depth_kernel, dim3(grid_for(rd->R, 256, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, rd->R, rd->n_slots, rd->d_slot_of.p,
                           rarefy_replicate_hash(seed, replicate), d_depth.p);
        PTX_HIP(ctx, hipGetLastError());
        return 0;
    }
    // bases [lb1 - lb0][V] zero-filled here; sp is the caller's to zero
    int pass(uint32_t lb0, uint32_t lb1, uint32_t lc0, unsigned long long *bases, unsigned long long *sp) {
        if (!db->V) return 0;
        PTX_TRY(zero_fill(ctx, bases, (size_t)(lb1 - lb0) * db->V * sizeof(unsigned long long)));
        const RfyPass P{lb0, lb1, lc0, db->S, db->V, bases, sp, d_serve.p};
        rs_launch_groups(ctx, rd, "rarefy_bases_kernel", rarefy_bases_kernel, db->d_node_len.p, rd->d_long_sum.p, rd->d_long_len0.p, d_depth.p, P);
        PTX_HIP(ctx, hipGetLastError());
        return 0;
    }
};

}  // namespace

// the test seam: the two kernels for ONE level over every species
int rarefy_node_bases_launch(Ctx *ctx, Db *db, Reads *rd, uint64_t seed, uint32_t replicate, uint32_t level, uint64_t *bases_out) {
    const uint64_t V = db->V;
    if (V == 0) return 0;
    RfyReads rr{ctx, db, rd};
    PTX_TRY(rr.prepare(std::vector<uint8_t>(db->S ? db->S : 1, 1)));
    PTX_TRY(rr.depths(seed, replicate));
    DevBuf<unsigned long long> d_bases, d_sp;
    PTX_HIP(ctx, d_bases.alloc(V));
    PTX_HIP(ctx, d_sp.alloc(2));
    PTX_TRY(rr.pass(level, level + 1, level + 1 /* no counters */, d_bases.p, d_sp.p));
    std::vector<unsigned long long> h(V);
    PTX_TRY(download(ctx, h.data(), d_bases.p, V));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::copy(h.begin(), h.end(), bases_out);
    return 0;
}

// selection validated by the caller; E = 1 + n_replicates * n_levels entries
int rarefy_launch(Ctx *ctx, Db *db, Reads *rd, const uint64_t *sel_off, const uint32_t *sel_hap, uint64_t seed, uint32_t n_levels, uint32_t n_replicates,
                  double *x_out, double *obj_out, uint64_t *rows_out, int32_t *status_out, uint64_t *reads_out, uint64_t *member_out) {
    const uint32_t S = db->S;
    if (S == 0) return 0;
    const uint64_t C = sel_off[S], V = db->V, E = 1ull + (uint64_t)n_replicates * n_levels;
    if (E * std::max<uint64_t>(C, S) >= 0xFFFFFFFFull)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_rarefy: %llu entries of %llu selection entries and %u species exceed 32-bit positions", (unsigned long long)E, (unsigned long long)C, S);
    // ---- the plan of the passes
    uint64_t fit = RAREFY_MAX_LEVELS;
    if (ctx->cfg.rarefy_levels_max == 0) {
        size_t free_b = 0, total_b = 0;
        PTX_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        fit = rarefy_default_arrays(free_b, V);
    }
    RarefyPlan plan;
    std::string why;
    if (!rarefy_plan(n_levels, fit, ctx->cfg.rarefy_levels_max, plan, why)) return fail(ctx, PANTAX_HIP_E_LIMIT, "%s", why.c_str());
    // ---- the species the stage thins: 1 <= K_s <= 64
    std::vector<uint8_t> serve(S, 0);
    for (uint32_t s = 0; s < S; ++s) { const uint64_t K = sel_off[s + 1] - sel_off[s]; serve[s] = (K >= 1 && K <= 64) ? 1 : 0; }
    RfyReads rr{ctx, db, rd};
    PTX_TRY(rr.prepare(serve));
    const size_t n_sp = (size_t)(n_levels + 1) * S * 2, n_mem = (size_t)std::max<uint64_t>(C, 1) * 2;
    DevBuf<unsigned long long> d_lev, d_sp, d_member;
    DevBuf<uint64_t> d_sel_off;
    if (V) PTX_HIP(ctx, d_lev.alloc((size_t)plan.per_pass * V));
    PTX_HIP(ctx, d_sp.alloc(n_sp));
    PTX_HIP(ctx, d_member.alloc(n_mem));
    PTX_TRY(upload(ctx, d_sel_off, sel_off, (size_t)S + 1));
    // results on the host; the caller's arrays are written at the very end
    std::vector<double> hx((size_t)(E * C), 0.0), hobj((size_t)(E * S), 0.0);
    std::vector<uint64_t> hrows((size_t)(E * S), 0), hreads((size_t)(E * S) * 2, 0), hmember((size_t)(E * C) * 2, 0);
    std::vector<int32_t> hstatus((size_t)(E * S), 1);
    std::vector<unsigned long long> c_sp(n_sp), c_member(n_mem);
    double dummy_x = 0.0;
    // the refit of one entry: the bootstrap's replicate 0 on `bases`, and the member counts from its base patterns
    const auto refit = [&](uint64_t e, const unsigned long long *bases) -> int {
        PTX_HIP(ctx, hipMemsetAsync(d_member.p, 0, n_mem * sizeof(unsigned long long), ctx->stream));
        const std::function<int(const BootFront &)> members = [&](const BootFront &F) -> int {
            KTimer tm(ctx, "rarefy_member_kernel");
            hipLaunchKernelGGL(rarefy_member_kernel, dim3((F.P + 255) / 256), dim3(256), 0, ctx->stream, F.P, F.d_bpat_mask.p, F.d_bpat_start.p, F.d_bpat_species.p,
                               d_sel_off.p, d_member.p);
            PTX_HIP(ctx, hipGetLastError());
            return 0;
        };
        PTX_TRY(bootstrap_launch_on(ctx, db, bases, sel_off, sel_hap, nullptr, 0, 0, ctx->cfg.rarefy_route, "strain_rarefy", &members, C ? hx.data() + e * C : &dummy_x,
                                    hobj.data() + e * S, hrows.data() + e * S, hstatus.data() + e * S));
        PTX_TRY(download(ctx, c_member.data(), d_member.p, n_mem));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint64_t c = 0; c < 2 * C; ++c) hmember[e * C * 2 + c] = c_member[c];
        return 0;
    };
    PTX_TRY(refit(0, (const unsigned long long *)db->d_bases.p));
    for (uint32_t b = 1; b <= n_replicates; ++b) {
        PTX_TRY(rr.depths(seed, b));
        PTX_HIP(ctx, hipMemsetAsync(d_sp.p, 0, n_sp * sizeof(unsigned long long), ctx->stream));
        for (uint32_t i = 0; i < plan.n_passes; ++i) {
            uint32_t l0, l1;
            rarefy_pass_levels(plan, n_levels, i, l0, l1);
            PTX_TRY(rr.pass(l0, l1, (b == 1 && i == 0) ? 0u : l0, d_lev.p, d_sp.p));   // entry 0's reads and bases: the first pass of all
            for (uint32_t l = l0; l < l1; ++l) PTX_TRY(refit(rarefy_entry(n_levels, b, l), d_lev.p + (size_t)(l - l0) * V));
        }
        PTX_TRY(download(ctx, c_sp.data(), d_sp.p, n_sp));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t l = (b == 1 ? 0u : 1u); l <= n_levels; ++l) {
            const uint64_t e = l == 0 ? 0 : rarefy_entry(n_levels, b, l);
            for (size_t j = 0; j < (size_t)S * 2; ++j) hreads[e * S * 2 + j] = c_sp[(size_t)l * S * 2 + j];
        }
    }
    if (C) { std::copy(hx.begin(), hx.end(), x_out); std::copy(hmember.begin(), hmember.end(), member_out); }
    std::copy(hobj.begin(), hobj.end(), obj_out); std::copy(hrows.begin(), hrows.end(), rows_out);
    std::copy(hstatus.begin(), hstatus.end(), status_out); std::copy(hreads.begin(), hreads.end(), reads_out);
    return 0;
}

}  // namespace ptx
