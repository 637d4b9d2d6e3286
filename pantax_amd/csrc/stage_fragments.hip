// stage_fragments.hip -- fragment support (pantax_hip_fragment_mates, pantax_hip_strain_fragments; the --strain-fragments report): read pairs as the unit
// of strain compatibility.  Not a stage of the reference.
//
// Contract: include/pantax_hip.h, DESIGN.md "Fragment support".  Integers only: no result depends on any order.
//
// Mates.  Keys and tags go up; radix_sort orders (key, read index) over the bits the keys use; frag_pair_kernel takes a lane per sorted position, finds
// the run of equal keys it stands in from its neighbours (two before, two behind) and writes its own verdict at its read index: every read is written
// by exactly one lane.  The four counters are ballots, added once per wave.
// Fragment pass, on the read-pass skeleton (read_pass_device.hpp):
//   frag_mask_kernel       a wave per 64-step group: C(r) of every counted read of a served species (1 <= K_s <= 64) as ONE u64 per slot, formed exactly as
//                          read_support_kernel forms it.  Its bits are those of the species' row of the table (route 1: haplotype index; route 2:
//                          position in the ascending list): the per-bit arrays name the weight and the caller's entry either way.  The tail lane of a
//                          walk of <= 64 steps stores plainly; longer walks AND their per-group partials into the word, which starts as all ones.
//   frag_mate_slot_kernel  mate[] (file order) -> slot space through Reads::d_slot_of, and the validation of mate[] on the way (one counter word).
//   frag_join_kernel       a lane per slot, in slot order (grouped by locus: a wave sees one or two species).  The mate with the smaller slot owns the
//                          fragment and gathers the other's slot record, read record and mask word (32 bytes of random access per fragment).  The wave
//                          reduces: species classes through rs_species_rounds, candidate classes by one ballot per set bit of the union of the
//                          round's F = C(r) & C(m), lane 0 one 64-bit atomicAdd per non-zero sum.  A discordant fragment adds its two entries of the
//                          pair block itself (rare, and spread over K_s^2 words).
//   frag_gather_kernel     |F| per slot -> file order (only when the caller asks for frag_n_out).
//
// Algorithmic bytes (T' padded steps, R' slots, R reads, F paired fragments): frag_mask_kernel those of read_support_kernel in (4T' + 1T' + 8T' + 16R' + 8R')
// and 8R' out; frag_join_kernel 16R' + 8R' + 4R' + 8R' in order and 32F gathered.
#include <algorithm>
#include <cmath>
#include "common.hpp"
#include "fragments_plan.hpp"
#include "read_pass_device.hpp"

namespace ptx {

namespace {

constexpr uint32_t FR_NONE = PANTAX_HIP_MATE_NONE, FR_AMBIGUOUS = PANTAX_HIP_MATE_AMBIGUOUS;
constexpr uint32_t FR_ELSEWHERE = 0xFFFFFFFDu;   // slot space only: the mate is a read without a walk
static_assert(FR_NONE == RS_NO_SLOT, "a mate without a slot is told from 'no mate' in frag_mate_slot_kernel");

// ---- mates from keys ----
__global__ void __launch_bounds__(256) frag_iota_kernel(uint64_t n, uint32_t *__restrict__ v) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) v[i] = (uint32_t)i;
}

// key [n] sorted, idx [n] the read of every sorted position (a permutation of 0 .. n - 1), tag [n] by read; counts [4] = pairs, none, ambiguous reads,
// keys seen three times or more
__global__ void __launch_bounds__(256) frag_pair_kernel(uint64_t n, const unsigned long long *__restrict__ key, const uint32_t *__restrict__ idx,
                                                        const uint8_t *__restrict__ tag, uint32_t *__restrict__ mate_out,
                                                        unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    for (uint64_t base = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64u; base < n; base += (uint64_t)gridDim.x * 256u) {   // (wave-uniform)
        const uint64_t i = base + (uint64_t)lane;
        const bool in = i < n;
        const unsigned long long k = in ? key[i] : 0ull;
        const bool p1 = in && i >= 1 && key[i - 1] == k, p2 = p1 && i >= 2 && key[i - 2] == k;
        const bool n1 = in && i + 1 < n && key[i + 1] == k, n2 = n1 && i + 2 < n && key[i + 2] == k;
        const bool crowd = (p1 && n1) || p2 || n2;      // my run holds three positions or more
        uint32_t verdict = FR_NONE;
        bool first_of_pair = false;
        if (in) {
            const uint32_t me = idx[i];
            if (crowd) verdict = FR_AMBIGUOUS;
            else if (p1 || n1) {
                const uint32_t other = idx[n1 ? i + 1 : i - 1];
                const uint32_t ta = tag[me], tb = tag[other];
                const bool ok = (ta | tb) == 0u || ta + tb == 3u;   // tags are 0, 1, 2: both 0, or {1, 2}
                verdict = ok ? other : FR_AMBIGUOUS;
                first_of_pair = ok && n1;
            }
            mate_out[me] = verdict;
        }
        const unsigned long long b_pair = __builtin_amdgcn_ballot_w64(first_of_pair), b_none = __builtin_amdgcn_ballot_w64(in && verdict == FR_NONE),
                                 b_amb = __builtin_amdgcn_ballot_w64(in && verdict == FR_AMBIGUOUS), b_k3 = __builtin_amdgcn_ballot_w64(in && !p1 && n2);
        if (lane == 0) {
            if (b_pair) atomicAdd(counts, (unsigned long long)__popcll(b_pair));
            if (b_none) atomicAdd(counts + 1, (unsigned long long)__popcll(b_none));
            if (b_amb) atomicAdd(counts + 2, (unsigned long long)__popcll(b_amb));
            if (b_k3) atomicAdd(counts + 3, (unsigned long long)__popcll(b_k3));
        }
    }
}

// ---- the fragment pass ----
struct FragSpecies {
    uint64_t pair_base;   // first entry of the species' K x K block (served)
    uint32_t K;           // candidates
    uint32_t ent0;        // first candidate entry of the species
    uint32_t served;      // 1: 1 <= K <= 64
    uint32_t pad;
};
struct FragOut {
    unsigned long long *hap;    // [C][4][3]  compatible, unique, unique_by_pair, assigned  x  n_fragments, n_steps, span
    unsigned long long *sp;     // [S][9][3]  the classes of fragments_plan.hpp
    unsigned long long *pair;   // [P]
};

__global__ void __launch_bounds__(256) frag_mask_kernel(uint32_t n_groups, uint32_t n_slots, const uint32_t *__restrict__ group_slot,
                                                        const uint8_t *__restrict__ step_code, const uint32_t *__restrict__ g_node_id,
                                                        const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                        const RsSpecies *__restrict__ tab, const unsigned long long *__restrict__ node_haps,
                                                        const unsigned long long *__restrict__ mask, unsigned long long *__restrict__ slot_mask) {
    const int lane = threadIdx.x & 63;
    for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += gridDim.x * 4) {
        const uint32_t gs = group_slot[g];                                   // (wave-uniform) NO_SLOT: a group of pads only
        if (gs == RS_NO_SLOT) continue;
        const RsLane L = rs_lane(g, gs, lane, n_slots, step_code, g_node_id, read_rec, slot_rec, tab);
        const unsigned long long m = rs_lane_word(L, 0u, lane, node_haps, mask);   // (every lane: seg_and)
        if (L.tail && L.counted) {
            const bool served = L.nw == 1u;                                  // one word: 1 <= K_s <= 64 on either route
            if (!served) { if (L.last) slot_mask[L.slot] = 0ull; }
            else if (L.is_long) rs_long_partial(slot_mask, 1u, L.slot, 0u, m);
            else if (L.last) slot_mask[L.slot] = m;
        }
    }
}

// mate [R] in file order -> mate_slot [R'] by slot: the codes as they are, the slot of the mate, FR_ELSEWHERE for a mate without a walk.  *bad counts the
// entries that are neither a code nor the index of another read that names this one back.
__global__ void __launch_bounds__(256) frag_mate_slot_kernel(uint64_t R, const uint32_t *__restrict__ mate, const uint32_t *__restrict__ slot_of,
                                                             uint32_t *__restrict__ mate_slot, uint32_t *__restrict__ bad) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 256) {
        const uint32_t m = mate[r];
        uint32_t ms = m;
        if (m < FR_AMBIGUOUS) {
            const bool ok = m < R && m != r && mate[m] == (uint32_t)r;
            if (!ok) atomicAdd(bad, 1u);
            ms = ok ? slot_of[m] : FR_ELSEWHERE;
            if (ms == RS_NO_SLOT) ms = FR_ELSEWHERE;
        }
        const uint32_t s = slot_of[r];
        if (s != RS_NO_SLOT) mate_slot[s] = ms;
    }
}

// argmax of the weight over the set bits of m != 0, ascending: the first of equal weights; a set whose weights are all NaN or -inf keeps its lowest bit
// (the rule of sup_take, stage_read_support.hip)
__device__ __forceinline__ uint32_t frag_argmax(unsigned long long m, const double *__restrict__ w) {
    uint32_t besti = (uint32_t)__builtin_ctzll(m);
    double best = -INFINITY;
    while (m) {
        const uint32_t idx = (uint32_t)__builtin_ctzll(m);
        m &= m - 1ull;
        const double x = w[idx];
        if (x > best) { best = x; besti = idx; }
    }
    return besti;
}
// the numbers of a fragment are sums of two reads': 64-bit lanes
__device__ __forceinline__ void frag_reduce_add(int lane, bool on, unsigned long long b, unsigned long long steps, unsigned long long span,
                                                unsigned long long *__restrict__ dst) {
    const auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
    const unsigned long long ss = wave_reduce(on ? steps : 0ull, add), sn = wave_reduce(on ? span : 0ull, add);
    if (lane == 0) rs_add3(dst, (unsigned long long)__popcll(b), ss, sn);
}

__global__ void __launch_bounds__(256) frag_join_kernel(uint32_t n_slots, const uint4 *__restrict__ read_rec, const uint2 *__restrict__ slot_rec,
                                                        const RsSpecies *__restrict__ tab, const FragSpecies *__restrict__ fsp,
                                                        const unsigned long long *__restrict__ slot_mask, const uint32_t *__restrict__ mate_slot,
                                                        const double *__restrict__ bit_w, const uint32_t *__restrict__ bit_entry,
                                                        int32_t *__restrict__ frag_n, FragOut out) {
    const int lane = threadIdx.x & 63;
    for (uint64_t base = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64u; base < n_slots; base += (uint64_t)gridDim.x * 256u) {   // (wave-uniform)
        const uint64_t s = base + (uint64_t)lane;
        const bool in = s < n_slots;
        uint4 rr = make_uint4(0u, 0u, 0u, 0u);
        uint32_t sp = 0xFFFFFFFFu;
        if (in) { rr = read_rec[s]; sp = slot_rec[s].x; }
        const bool counted = in && (int32_t)sp >= 0;
        uint32_t ms = FR_NONE;
        if (counted) ms = mate_slot[s];
        bool paired = false;
        if (counted && ms < n_slots) paired = slot_rec[ms].x == sp;           // a slot (the codes lie above every slot): the mate is counted and of my species
        const bool single = counted && ms == FR_NONE, multi = counted && ms == FR_AMBIGUOUS, elsewhere = counted && !single && !multi && !paired;
        const bool owner = paired && s < (uint64_t)ms;
        unsigned long long cm_raw = 0ull, mm_raw = 0ull;
        uint4 mrr = make_uint4(0u, 0u, 0u, 0u);
        if (paired && (owner || frag_n)) { cm_raw = slot_mask[s]; mm_raw = slot_mask[ms]; }
        if (owner) mrr = read_rec[ms];
        const uint32_t steps = rr.y, span = rs_span(rr);
        const unsigned long long fsteps = (unsigned long long)rr.y + mrr.y, fspan = (unsigned long long)span + rs_span(mrr);
        rs_species_rounds(counted, sp, [&](uint32_t s0, bool mine, unsigned long long mb) {
            const RsSpecies st = tab[s0];
            const FragSpecies fs = fsp[s0];
            unsigned long long *const so = out.sp + (uint64_t)s0 * (3u * FRG_N_CLASSES);
            rs_reduce_add(lane, mine, mb, steps, span, so + 3 * FRG_COUNTED);
            {
                const bool si = mine && single, mu = mine && multi, el = mine && elsewhere;
                const unsigned long long b_si = __builtin_amdgcn_ballot_w64(si), b_mu = __builtin_amdgcn_ballot_w64(mu), b_el = __builtin_amdgcn_ballot_w64(el);
                if (b_si) rs_reduce_add(lane, si, b_si, steps, span, so + 3 * FRG_SINGLE);
                if (b_mu) rs_reduce_add(lane, mu, b_mu, steps, span, so + 3 * FRG_MULTI);
                if (b_el) rs_reduce_add(lane, el, b_el, steps, span, so + 3 * FRG_ELSEWHERE);
            }
            // the bits of the species' row and no other: whatever a mask word holds, no position behind the per-bit arrays is ever read
            const unsigned long long row_bits = !fs.served ? 0ull : st.m.route == 1u ? st.m.bits : (fs.K >= 64u ? ~0ull : (1ull << fs.K) - 1ull);
            const unsigned long long cm = cm_raw & row_bits, mm = mm_raw & row_bits;
            if (frag_n && fs.served && mine && paired) frag_n[s] = (int32_t)__popcll(cm & mm);
            const bool own = mine && owner;
            const unsigned long long b_own = __builtin_amdgcn_ballot_w64(own);
            if (b_own == 0ull) return;
            frag_reduce_add(lane, own, b_own, fsteps, fspan, so + 3 * FRG_PAIRED);
            if (!fs.served) return;
            const unsigned long long F = cm & mm;
            const bool conc = own && F != 0ull, disc = own && F == 0ull && cm != 0ull && mm != 0ull, unex = own && cm == 0ull && mm == 0ull;
            const bool half = own && !conc && !disc && !unex;
            const unsigned long long b_co = __builtin_amdgcn_ballot_w64(conc), b_di = __builtin_amdgcn_ballot_w64(disc), b_ha = __builtin_amdgcn_ballot_w64(half),
                                     b_un = __builtin_amdgcn_ballot_w64(unex);
            if (b_co) frag_reduce_add(lane, conc, b_co, fsteps, fspan, so + 3 * FRG_CONCORDANT);
            if (b_di) frag_reduce_add(lane, disc, b_di, fsteps, fspan, so + 3 * FRG_DISCORDANT);
            if (b_ha) frag_reduce_add(lane, half, b_ha, fsteps, fspan, so + 3 * FRG_HALF);
            if (b_un) frag_reduce_add(lane, unex, b_un, fsteps, fspan, so + 3 * FRG_UNEXPLAINED);
            const double *const w = bit_w + st.bit_base;
            const uint32_t *const ent = bit_entry + st.bit_base;
            if (disc) {   // filed by the assigned strains of the two mates; they differ: the sets are disjoint
                const uint64_t pa = ent[frag_argmax(cm, w)] - fs.ent0, pb = ent[frag_argmax(mm, w)] - fs.ent0;
                if (pa < fs.K && pb < fs.K) {
                    atomicAdd(out.pair + fs.pair_base + pa * fs.K + pb, 1ull);
                    atomicAdd(out.pair + fs.pair_base + pb * fs.K + pa, 1ull);
                }
            }
            if (b_co == 0ull) return;
            const unsigned long long Fm = conc ? F : 0ull;
            const uint32_t besti = conc ? frag_argmax(F, w) : 64u;
            const bool by_pair = __popcll(cm) != 1 && __popcll(mm) != 1;
            const unsigned long long present = wave_reduce(Fm, [](unsigned long long x, unsigned long long y) { return x | y; });
            for (unsigned long long q = present; q; q &= q - 1ull) {           // (wave-uniform)
                const int b = __builtin_ctzll(q);
                const bool has = (Fm >> b) & 1ull;
                const unsigned long long cb = __builtin_amdgcn_ballot_w64(has);
                const uint32_t e = ent[b];
                if (e == MEMBER_NO_ENTRY) continue;
                unsigned long long *const ho = out.hap + (uint64_t)e * (3u * FRG_N_HAP);
                frag_reduce_add(lane, has, cb, fsteps, fspan, ho + 3 * FRG_COMPATIBLE);
                const bool uq = has && Fm == (1ull << b), up = uq && by_pair, as = has && besti == (uint32_t)b;
                const unsigned long long b_uq = __builtin_amdgcn_ballot_w64(uq), b_up = __builtin_amdgcn_ballot_w64(up), b_as = __builtin_amdgcn_ballot_w64(as);
                if (b_uq) frag_reduce_add(lane, uq, b_uq, fsteps, fspan, ho + 3 * FRG_UNIQUE);
                if (b_up) frag_reduce_add(lane, up, b_up, fsteps, fspan, ho + 3 * FRG_UNIQUE_BY_PAIR);
                if (b_as) frag_reduce_add(lane, as, b_as, fsteps, fspan, ho + 3 * FRG_ASSIGNED);
            }
        });
    }
}

// file order: only the entries of reads binned to a species of the db
__global__ void __launch_bounds__(256) frag_gather_kernel(uint64_t R, const uint32_t *__restrict__ slot_of, const uint2 *__restrict__ slot_rec,
                                                          const int32_t *__restrict__ frag_n, int32_t *__restrict__ n_out) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 256) {
        const uint32_t s = slot_of[r];
        if (s == RS_NO_SLOT) continue;
        if ((int32_t)slot_rec[s].x == -1) continue;                           // "U" against this db
        n_out[r] = frag_n[s];
    }
}

}  // namespace

// key / tag / mate_out [n] host arrays, 0 < n < 2^32 - 2, tags <= 2 (validated by the caller); counts_out [4]
int fragment_mates_launch(Ctx *ctx, uint64_t n, const uint64_t *key, const uint8_t *tag, uint32_t *mate_out, uint64_t *counts_out) {
    uint64_t used = 0;
    for (uint64_t i = 0; i < n; ++i) used |= key[i];
    DevBuf<uint64_t> d_ka, d_kb;
    DevBuf<uint32_t> d_va, d_vb, d_table, d_tmp, d_mate;
    DevBuf<uint8_t> d_tag;
    RsCounters cnt;
    PTX_TRY(upload(ctx, d_ka, key, n));
    PTX_TRY(upload(ctx, d_tag, tag, n));
    PTX_HIP(ctx, d_kb.alloc(n)); PTX_HIP(ctx, d_va.alloc(n)); PTX_HIP(ctx, d_vb.alloc(n)); PTX_HIP(ctx, d_mate.alloc(n));
    PTX_HIP(ctx, d_table.alloc(sort_table_elems(n))); PTX_HIP(ctx, d_tmp.alloc(scan_tmp_elems(n)));
    PTX_TRY(cnt.init(ctx, 4));
    unsigned long long *const d_counts = cnt.take(4);
    {
        KTimer tm(ctx, "frag_iota_kernel");
        hipLaunchKernelGGL(frag_iota_kernel, dim3(grid_for(n, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, n, d_va.p);
    }
    SortBufs A, B;
    A.nw = B.nw = 1; A.k[0] = d_ka.p; B.k[0] = d_kb.p; A.v = d_va.p; B.v = d_vb.p;
    std::vector<SortPass> passes;
    add_passes(passes, 0, 0, bits_for(used));
    bool in_b = false;
    PTX_TRY(radix_sort(ctx, A, B, n, passes.data(), (int)passes.size(), d_table.p, d_tmp.p, &in_b));
    {
        KTimer tm(ctx, "frag_pair_kernel");
        hipLaunchKernelGGL(frag_pair_kernel, dim3(grid_for((n + 63) / 64, 4, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, n,
                           reinterpret_cast<const unsigned long long *>(in_b ? d_kb.p : d_ka.p), in_b ? d_vb.p : d_va.p, d_tag.p, d_mate.p, d_counts);
    }
    PTX_HIP(ctx, hipGetLastError());
    PTX_TRY(download(ctx, mate_out, d_mate.p, n));
    PTX_TRY(download(ctx, (unsigned long long *)counts_out, d_counts, 4));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    return 0;
}

// the candidates of every species in ascending haplotype order (cand_hap, cand_w), entry_of[c] = the caller's entry of sorted candidate c; validated by the
// caller.  mate [R] is validated here, on the device, before anything is written; then pair_off_out [S+1] and the pair_cap rule of read support.
int fragments_launch(Ctx *ctx, Db *db, Reads *rd, const uint64_t *cand_off, const uint32_t *cand_hap, const double *cand_w, const uint64_t *entry_of,
                     const uint32_t *mate, uint64_t *hap_out, uint64_t *species_out, int32_t *status_out, uint64_t *pair_off_out, uint64_t pair_cap,
                     uint64_t *pair_out, int32_t *frag_n_out) {
    const uint32_t S = db->S, n_slots = rd->n_slots;
    const uint64_t H = db->H, C = cand_off[S], R = rd->R;
    PTX_TRY(rs_check_bits(ctx, "strain_fragments", H, C));
    if (R >= FR_ELSEWHERE) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_fragments: %llu reads exceed the 32-bit mate indices", (unsigned long long)R);
    DevBuf<uint32_t> d_mate, d_mate_slot, d_bad;
    if (R) {
        uint32_t bad = 0;
        PTX_TRY(upload(ctx, d_mate, mate, R));
        PTX_HIP(ctx, d_mate_slot.alloc(n_slots ? n_slots : 1));
        PTX_HIP(ctx, d_bad.alloc(1));
        PTX_HIP(ctx, hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), ctx->stream));
        {
            KTimer tm(ctx, "frag_mate_slot_kernel");
            hipLaunchKernelGGL(frag_mate_slot_kernel, dim3(grid_for(R, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, R, d_mate.p, rd->d_slot_of.p, d_mate_slot.p,
                               d_bad.p);
        }
        PTX_HIP(ctx, hipGetLastError());
        PTX_TRY(download(ctx, &bad, d_bad.p, 1));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (bad) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_fragments: %u entries of mate are neither a code nor the index of another read that names them back", bad);
    }
    std::vector<uint64_t> pair_off(S + 1, 0);
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = cand_off[s + 1] - cand_off[s];
        pair_off[s + 1] = pair_off[s] + (K <= FRAG_MAX_LIST ? K * K : 0);
    }
    std::copy(pair_off.begin(), pair_off.end(), pair_off_out);
    const uint64_t P = pair_off[S];
    if (P > pair_cap)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_fragments: %llu pair entries, the caller's array holds %llu", (unsigned long long)P, (unsigned long long)pair_cap);
    if ((C && !hap_out) || (S && (!species_out || !status_out)) || (P && !pair_out)) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_fragments: null output array");
    std::vector<double> bit_w(H + C + 1, 0.0);
    std::vector<uint32_t> bit_entry(H + C + 1, MEMBER_NO_ENTRY);
    RsTable rt;
    rs_table_build(ctx, db, cand_off, cand_hap, rt, [&](uint64_t at, uint64_t c) { bit_w[at] = cand_w[c]; bit_entry[at] = (uint32_t)entry_of[c]; });
    std::vector<FragSpecies> fsp(S ? S : 1, FragSpecies{0ull, 0u, 0u, 0u, 0u});
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = cand_off[s + 1] - cand_off[s];
        fsp[s] = FragSpecies{pair_off[s], (uint32_t)std::min<uint64_t>(K, 0xFFFFFFFFull), (uint32_t)cand_off[s], (K >= 1 && K <= FRAG_MAX_LIST) ? 1u : 0u, 0u};
    }
    const size_t n_hap = (size_t)C * 3 * FRG_N_HAP, n_sp = (size_t)S * 3 * FRG_N_CLASSES, n_out = n_hap + n_sp + (size_t)P;
    if (n_out == 0) return 0;
    RsCounters cnt;
    DevBuf<RsSpecies> d_tab;
    DevBuf<FragSpecies> d_fsp;
    DevBuf<double> d_bit_w;
    DevBuf<uint32_t> d_bit_entry;
    DevBuf<unsigned long long> d_slot_mask;
    DevBuf<int32_t> d_frag_n, d_n_out;
    PTX_TRY(cnt.init(ctx, n_out));
    const FragOut out{cnt.take(n_hap), cnt.take(n_sp), cnt.take((size_t)P)};
    PTX_TRY(upload(ctx, d_tab, rt.tab.data(), rt.tab.size()));
    PTX_TRY(upload(ctx, d_fsp, fsp.data(), fsp.size()));
    PTX_TRY(upload(ctx, d_bit_w, bit_w.data(), bit_w.size()));
    PTX_TRY(upload(ctx, d_bit_entry, bit_entry.data(), bit_entry.size()));
    PTX_TRY(rt.wm.build(ctx, db));
    PTX_HIP(ctx, d_slot_mask.alloc(n_slots ? n_slots : 1));
    if (n_slots) PTX_TRY(byte_fill(ctx, d_slot_mask.p, 0xFF, (size_t)n_slots * sizeof(unsigned long long)));   // the identity of the long walks' AND
    const bool want_n = frag_n_out != nullptr && R != 0;
    if (want_n) {
        PTX_HIP(ctx, d_frag_n.alloc(n_slots ? n_slots : 1));
        if (n_slots) PTX_TRY(byte_fill(ctx, d_frag_n.p, 0xFF, (size_t)n_slots * sizeof(int32_t)));   // -1 unless the join says otherwise
    }
    rs_launch_groups(ctx, rd, "frag_mask_kernel", frag_mask_kernel, d_tab.p, rs_node_haps(rt, db), rt.wm.d_mask.p, d_slot_mask.p);
    if (n_slots) {
        KTimer tm(ctx, "frag_join_kernel");
        hipLaunchKernelGGL(frag_join_kernel, dim3(grid_for(((uint64_t)n_slots + 63) / 64, 4, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, n_slots,
                           rd->d_g_read_rec.p, rd->d_g_slot_rec.p, d_tab.p, d_fsp.p, d_slot_mask.p, d_mate_slot.p, d_bit_w.p, d_bit_entry.p,
                           want_n ? d_frag_n.p : nullptr, out);
    }
    if (want_n) {
        // the caller's array travels up first: entries of reads outside this db's species keep what the caller put there
        PTX_TRY(upload(ctx, d_n_out, frag_n_out, R));
        if (n_slots) {
            KTimer tm(ctx, "frag_gather_kernel");
            hipLaunchKernelGGL(frag_gather_kernel, dim3(grid_for(R, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, R, rd->d_slot_of.p, rd->d_g_slot_rec.p,
                               d_frag_n.p, d_n_out.p);
        }
        PTX_TRY(download(ctx, frag_n_out, d_n_out.p, R));
    }
    PTX_HIP(ctx, hipGetLastError());
    if (C) PTX_TRY(download(ctx, (unsigned long long *)hap_out, out.hap, n_hap));
    if (S) PTX_TRY(download(ctx, (unsigned long long *)species_out, out.sp, n_sp));
    if (P) PTX_TRY(download(ctx, (unsigned long long *)pair_out, out.pair, (size_t)P));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the temporaries are released on return
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = cand_off[s + 1] - cand_off[s];
        status_out[s] = K == 0 ? 1 : K > FRAG_MAX_LIST ? PANTAX_HIP_E_LIMIT : 0;
    }
    return 0;
}

}  // namespace ptx
