// ssn_patterns.hip -- node-order row sort, the pattern heads: the runs of equal mask in every segment's sorted rows, found from the splitters.
#include "ssn_device.hpp"

namespace ptx {

namespace {
// ---------------------------------------------------------------------------------------------
// Patterns = runs of equal mask in a segment's sorted rows (the solver's groups, lad_prepare).  No pass over the rows: a run can only
// begin where the mask of the SPLITTERS changes -- between two splitters of one mask every row has that mask, and the row in front of
// them is a copy of the lower splitter or a row behind it -- so one wave per segment walks the 1023 splitters and reads the rows of the
// few bucket pairs at a change (and of the first and the last pair).  Heads are collected in order in the segment's part of the row
// scratch, which the local kernels have finished with.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ssn_heads_kernel(Sn sn, uint32_t *__restrict__ sub_k) {
    // wave w of a segment (four per workgroup): the bucket pairs [HP w, HP w + HP), its heads from slot start[2 HP w] of the scratch on
    // (a range holds no more heads than rows); sub_k[s][w] = how many
    constexpr int NW = SN_NWH, HP = SN_HP;
    const uint32_t s = blockIdx.y, o = sn.node_base[s], nn = sn.node_base[s + 1] - o, lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t n = nn ? sn.seg_n[s] : 0u;
    const uint32_t *w = sn.w(s);
    const uint32_t out = n ? sn.seg_out[s] : 0u;
    const bool small = n != 0 && w[SN_OFF_FLAGS] != 0;
    const uint32_t *start = w + SN_OFF_START;
    uint32_t cnt = 0;
    if (n != 0 && (!small || wave == 0)) {
        ulonglong2 *heads = sn.rows + o + (small ? 0u : start[2 * HP * wave]);   // {mask word as stored, first row of the run}
        // rows [r0, r1) of the output, in order.  Only key words that were STORED may be read (Sn::keys_all == 0: those of the small segments and of the even
        // buckets of mixed pairs), so the caller says what it knows from the splitters: pm0 = the mask word of row r0 - 1 (used when r0 > out), and row
        // `tie` (~0u: none) has the mask word tm.  Every other km read here is a row of [r0, r1) other than `tie`.
        auto scan_rows = [&](uint32_t r0, uint32_t r1, uint64_t pm0, uint32_t tie, uint64_t tm) {
            for (uint32_t base = r0; base < r1; base += 64) {
                const uint32_t i = base + lane;
                const bool in = i < r1;
                const uint64_t m = in ? (i == tie ? tm : sn.km[i]) : 0ull, pm = (in && i > out) ? (i == r0 ? pm0 : sn.km[i - 1]) : 0ull;
                const bool head = in && (i == out || m != pm);
                const uint64_t bal = __ballot(head);
                if (head) heads[cnt + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = make_ulonglong2(m, (uint64_t)i);
                cnt += (uint32_t)__popcll(bal);
            }
        };
        if (small) scan_rows(out, out + n, 0ull, ~0u, 0ull);  // a small segment has no splitters (and all its key words: r0 == out, no row in front)
        else {
            const ulonglong2 *tree = reinterpret_cast<const ulonglong2 *>(w + SN_OFF_TREE);
            const uint32_t j = HP * wave + (lane < (uint32_t)HP ? lane : 0u);
            const bool c = sn_pair_mixed(tree, j);            // the pairs whose even bucket the local sorts stored with key words
            uint64_t bal = __ballot(c && lane < (uint32_t)HP);
            while (bal) {
                const uint32_t jj = HP * wave + (uint32_t)__builtin_ctzll(bal);
                bal &= bal - 1;
                // the odd bucket of the pair holds copies of ONE key (splitter jj): a head can only be its first row -- the rest is not read (round 6:
                // with fifty strains nearly every splitter changes the mask, and a tie bucket of 1e5 rows kept one wave reading for the whole 0.43 ms)
                // -- and that row's mask is the splitter's, so it comes from the tree (the tie fill stores no key words where nothing else reads them).
                const uint32_t b0 = start[2 * jj], e0 = start[2 * jj + 1], e1 = start[2 * jj + 2];
                const bool tie = e1 > e0;                     // (then jj < SN_NSPLIT: the last odd bucket stays empty)
                if (!tie && e0 == b0) continue;
                const uint64_t tm = tie ? sn.key_word(s, tree[tree_node(jj)].x) : 0ull;
                // The row in front of the range, r0 - 1 (when the segment has one: b0 > 0).  It is the last row of the nearest non-empty bucket below 2 jj.
                // As a rule that is the tie bucket 2 jj - 1: splitter jj - 1 is a sampled row, and the node pass files that very node as equal to it.  The
                // bucket is empty only when splitter jj - 1 repeats an earlier splitter as a whole key -- the descent files the equal rows under ONE of the
                // copies, and the even buckets between copies hold nothing -- or is a pad behind the valid samples.  So walk down over the empty buckets to
                // the one that holds the row, whichever it is: a tie bucket q has the mask of splitter q / 2 (for a repeated splitter: the same mask, one
                // of its copies); an even bucket of a pair that is not mixed has the mask of its upper splitter; the even bucket of a mixed pair was stored
                // with its key words.  No case reads a word that was not written, and none depends on the rule above.
                uint64_t pm0 = 0ull;
                if (b0 > 0) {
                    uint32_t q = 2 * jj - 1;                  // (b0 > 0: jj > 0 and a non-empty bucket below 2 jj exists; the walk is the same in every lane)
                    while (start[q + 1] == start[q]) --q;
                    uint64_t mv = 0;
                    if ((q & 1u) != 0u) pm0 = sn.key_word(s, tree[tree_node(q >> 1)].x);
                    else if (sn_pair_mixed(tree, q >> 1, &mv)) pm0 = sn.km[out + b0 - 1];
                    else pm0 = sn.key_word(s, mv);
                }
                scan_rows(out + b0, out + e0 + (tie ? 1u : 0u), pm0, tie ? out + e0 : ~0u, tm);
            }
        }
    }
    if (lane == 0) sub_k[(size_t)s * NW + wave] = cnt;
}
// first pattern of every segment, the number of patterns, and the end of the last run
__global__ void __launch_bounds__(1024) ssn_patscan_kernel(uint32_t S, const uint32_t *__restrict__ sub_k, uint32_t *__restrict__ sp_pat_off, uint32_t *__restrict__ d_K,
                                                           const uint32_t *__restrict__ d_n, uint32_t *__restrict__ pat_start) {
    constexpr int NW = SN_NWH;
    __shared__ uint32_t s_wave[16];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < S; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        uint32_t v = 0;
        if (i < S) for (int q = 0; q < NW; ++q) v += sub_k[(size_t)i * NW + q];
        uint32_t tot;
        const uint32_t ex = block_excl_scan<1024>(v, s_wave, &tot);
        if (i < S) sp_pat_off[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) { sp_pat_off[S] = carry; *d_K = carry; pat_start[carry] = *d_n; }
}
__global__ void __launch_bounds__(256) ssn_patfill_kernel(Sn sn, const uint32_t *__restrict__ sub_k, const uint32_t *__restrict__ sp_pat_off, uint64_t *__restrict__ pat_mask,
                                                          uint32_t *__restrict__ pat_start, uint32_t *__restrict__ pat_species) {
    constexpr int NW = SN_NWH;
    const uint32_t s = blockIdx.x, k0 = sp_pat_off[s];
    const uint32_t *w = sn.w(s);
    const bool small = w[SN_OFF_FLAGS] != 0;
    uint32_t before = 0;
    for (int q = 0; q < NW; before += sub_k[(size_t)s * NW + q], ++q) {
        const uint32_t cnt = sub_k[(size_t)s * NW + q];
        if (cnt == 0) continue;
        const ulonglong2 *heads = sn.rows + sn.node_base[s] + (small ? 0u : w[SN_OFF_START + 2 * SN_HP * q]);
        for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
            const ulonglong2 h = heads[i];
            pat_mask[k0 + before + i] = sn.pack_shift >= 0 ? (h.x & ((1ull << sn.pack_shift) - 1ull)) : h.x;
            pat_start[k0 + before + i] = (uint32_t)h.y;
            pat_species[k0 + before + i] = s;
        }
    }
}
}  // namespace

void ssn_patterns_launch(Ctx *ctx, const Sn &sn, uint32_t S, uint32_t *sub_k, const RowPatterns &pat, const uint32_t *d_n) {
    hipLaunchKernelGGL(ssn_heads_kernel, dim3(SN_NWH / 4, S), dim3(256), 0, ctx->stream, sn, sub_k);
    hipLaunchKernelGGL(ssn_patscan_kernel, dim3(1), dim3(1024), 0, ctx->stream, S, (const uint32_t *)sub_k, pat.sp_pat_off, pat.d_K, d_n, pat.pat_start);
    hipLaunchKernelGGL(ssn_patfill_kernel, dim3(S), dim3(256), 0, ctx->stream, sn, (const uint32_t *)sub_k, (const uint32_t *)pat.sp_pat_off, pat.pat_mask, pat.pat_start,
                       pat.pat_species);
}

}  // namespace ptx
