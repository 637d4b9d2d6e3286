// stage_hap_stats.hip -- a9 on device: the per-haplotype unique-trio statistics by key (zscore_filter, profile.rs:1028-1051; :1114-1147)
// and the first filter that reads them (first_filter_paths, profile.rs:1080-1227).
#include <algorithm>
#include <cstdio>
#include <vector>
#include "lad.hpp"
#include "primitives.hpp"
#include "wave.hpp"

namespace ptx {

// ---------------------------------------------------------------------------------------------
// a9: per-hap unique-trio statistics, BY KEY (round 5).  The rows of the index are numbered in filing order -- node after node --, so
// the rows of one haplotype are scattered over its species' block; every row carries its owner (d_trio_hap).  The block of a species
// is cut into chunks of rows; ONE WAVE takes a chunk and keeps an accumulator per haplotype of the species (in LDS; in the chunk's own
// row of the partials for a species of more than HS_LDS_HAPS haplotypes): per 64 rows it walks the distinct owners among its lanes --
// neighbouring rows are windows around the same private allele, a handful of owners -- and adds each owner's lanes by a DPP reduction
// in fixed lane order.  A chunk's partials are then added in chunk order by one wave per species.  Every sum has a fixed order: same bits
// on every run (the reference's own order is that of a hash set).  Three passes like zscore_filter (profile.rs:1028-1051): (sum, count)
// of the non-zero abundances -> mean; squared deviations -> sd; (sum, count) of |z| < 3 -> the filtered mean.
// ALL NON-ZERO ABUNDANCES OF A HAPLOTYPE EQUAL (x, x, ... c times): the reference's mean is c SEQUENTIAL additions of x over c (data.iter().sum()) --
// whatever the order of the rows --, and whether that gives x back decides sd == 0 and with it the filtered mean (0.0 or x).  The sums here have
// another shape (lanes, a DPP tree, chunks) and land on the other side for many (c, x).  So pass 0 also carries, per haplotype, the OR of the
// values' bits and the OR of their complements (HapBits; exact, order-free, zero for "nothing"): no bit position is set in both exactly when all
// values are equal, and then hap_combine_kernel forms the mean the reference's way.  Passes 1 and 2 follow from that mean.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t HS_CHUNK_ROWS = 1024, HS_LDS_HAPS = 1024;
constexpr int HS_SLAB = 16;   // haplotypes whose accumulators a lane keeps in registers at a time
struct HapAcc { double a; uint32_t c, n; };   // sum, count of the pass, rows seen (pass 0)
struct HapBits { unsigned long long any1, any0; };   // pass 0: OR of the non-zero values' bits, OR of their complements

template <int PASS>
__global__ void __launch_bounds__(64) hap_rows_pass_kernel(const uint4 *__restrict__ chunks, const uint64_t *__restrict__ hap_off, const uint16_t *__restrict__ row_hap,
                                                           unsigned long long *tb /* read, and -- clean != 0, pass 0 -- zeroed behind the read */, const trio_len_t *__restrict__ tlen,
                                                           const double *__restrict__ mean0, const double *__restrict__ sd, HapAcc *__restrict__ part,
                                                           HapBits *__restrict__ pbits /* pass 0: beside the partials, same index */,
                                                           double *__restrict__ cx, uint16_t *__restrict__ chh, uint32_t *__restrict__ cn, uint32_t clean,
                                                           const uint8_t *__restrict__ active) {
    extern __shared__ HapAcc s_hap_acc[];
    __shared__ uint32_t s_qrow[128];
    __shared__ unsigned long long s_qtb[128];
    __shared__ unsigned long long s_any[PASS == 0 ? 128 : 1];   // pass 0, up to 64 haplotypes on the slab route: [h] OR of the value bits, [64 + h] OR of their complements
    const uint4 ch = chunks[blockIdx.x];                       // {species, first row, end row, first partial}
    const uint32_t h0 = (uint32_t)hap_off[ch.x], Hs = (uint32_t)hap_off[ch.x + 1] - h0;
    const int lane = threadIdx.x;
    // a species the species level dropped: the coverage pass skipped its reads, its rows' abundances are all zero -- the partials of an empty chunk, nothing read
    if (active != nullptr && active[ch.x] == 0) {              // (chunk-uniform)
        for (uint32_t h = (uint32_t)lane; h < Hs; h += 64) { part[ch.w + h] = HapAcc{0.0, 0u, 0u}; if (PASS == 0) pbits[ch.w + h] = HapBits{0ull, 0ull}; }
        if (PASS == 0 && lane == 0) cn[blockIdx.x] = 0u;
        return;
    }
    // Only rows with a NON-ZERO abundance count in any of the three statistics (profile.rs:1129-1133: `> 0.0`), and most rows are zero (the strains that
    // are not in the sample; a fifth of the rows at the BASELINE configurations).  Pass 0 reads the abundances of all rows (8 bytes each), QUEUES the
    // non-zero ones in LDS and handles them 64 at a time on dense lanes: length and owner are gathered, the f64 division is done, and {owner, value} go
    // to the chunk's stretch of a compacted copy -- passes 1 and 2 read that copy alone.  Before: three passes over {8, 4, 2} bytes of every row with a
    // division per row and pass, bound by VALU issue (184 wave-instructions per 64 rows: 0.8 ms a pass at 1e4 strains).
    // Up to 64 haplotypes per species (every species of the BASELINE configurations): every LANE keeps its own accumulators for a slab of
    // HS_SLAB haplotypes in registers and adds its rows to them by compare-and-select -- no cross-lane traffic and no scalar round trip inside
    // the loop over the rows; the lanes meet once per chunk and slab (DPP reductions, fixed order).  Version 1 of this kernel walked the distinct
    // owners of every 64 rows (readlane -> ballot -> DPP reduction -> owner's lane adds): ~150 cycles of scalar / vector ping-pong per owner,
    // 2.0 ms a pass at 1e4 strains whether the accumulators sat in LDS or in registers (round 4's kernel over contiguous rows: 0.85 ms for
    // all three).  A species of 17 .. 64 haplotypes reads its compacted rows once per slab.  Mean and sd of pass 0 / 1 ride in lane h and reach
    // a row's lane by one bpermute.
    const bool in_reg = Hs <= 64u;
    const bool in_lds = !in_reg && Hs <= HS_LDS_HAPS;
    HapAcc *acc = in_lds ? s_hap_acc : part + ch.w;            // (more than 64 haplotypes: LDS; beyond HS_LDS_HAPS the chunk's own, zero-filled row of partials)
    HapBits *accb = in_lds ? reinterpret_cast<HapBits *>(s_hap_acc + Hs) : pbits + ch.w;   // (pass 0; the LDS holds 32 bytes per haplotype)
    if (in_lds) for (uint32_t h = lane; h < Hs; h += 64) { acc[h] = HapAcc{0.0, 0u, 0u}; if (PASS == 0) accb[h] = HapBits{0ull, 0ull}; }
    if (PASS == 0 && in_reg) { s_any[lane] = 0ull; s_any[64 + lane] = 0ull; }
    __syncthreads();
    double my_mean = 0.0, my_sd = 0.0;
    if (in_reg && PASS >= 1 && (uint32_t)lane < Hs) { my_mean = mean0[h0 + lane]; if (PASS == 2) my_sd = sd[h0 + lane]; }
    uint32_t n_c = PASS == 0 ? 0u : cn[blockIdx.x];           // non-zero rows of the chunk = entries of its compacted stretch [ch.y, ch.y + n_c)
    // what a compacted entry {h, x > 0} adds in this pass (all lanes come here: the shuffles)
    auto pass_value = [&](uint32_t h, double x, bool valid, double &val, bool &flag) {
        val = 0.0; flag = false;
        if (PASS == 0) { if (valid) { val = x; flag = true; } return; }             // :1129-1133
        double m, s_ = 0.0;
        if (in_reg) { m = __shfl(my_mean, (int)(h & 63u)); if (PASS == 2) s_ = __shfl(my_sd, (int)(h & 63u)); }
        else { m = valid ? mean0[h0 + h] : 0.0; if (PASS == 2) s_ = valid ? sd[h0 + h] : 0.0; }
        if (valid) {
            if (PASS == 1) { val = (x - m) * (x - m); flag = true; }
            else if (s_ != 0.0 && fabs((x - m) / s_) < 3.0) { val = x; flag = true; }   // :1043-1050
        }
    };
    // pass 0: the chunk's rows -> its compacted stretch, every dense batch of up to 64 entries handed to `sink` on the way
    auto compact_rows = [&](auto &&sink) {
        uint32_t qh = 0, qn = 0, nw = 0;                       // queue head, entries queued, entries written (wave-uniform)
        auto drain = [&](uint32_t nb) {
            const bool v = (uint32_t)lane < nb;
            const uint32_t row = s_qrow[(qh + (uint32_t)lane) & 127u];
            const unsigned long long t = s_qtb[(qh + (uint32_t)lane) & 127u];
            uint32_t h = 0xFFFFFFFFu;
            double x = 0.0;
            if (v) {
#if TRIO_LH_PACK
                const uint2 lh = tlen[row];
                h = lh.y;
                x = (double)(long long)t / (double)lh.x;                       // profile.rs:1013-1014
#else
                h = row_hap[row];
                x = (double)(long long)t / (double)tlen[row];                  // profile.rs:1013-1014
#endif
                cx[ch.y + nw + (uint32_t)lane] = x; chh[ch.y + nw + (uint32_t)lane] = (uint16_t)h;
            }
            sink(h, x, v);
            qh = (qh + nb) & 127u; qn -= nb; nw += nb;
        };
#ifndef HS_TB_AHEAD
#define HS_TB_AHEAD 4
#endif
        constexpr int TA = HS_TB_AHEAD;                        // stretches of 64 rows whose abundances are requested together (one at a time: a round trip per stretch)
        for (uint32_t rb = ch.y; rb < ch.z; rb += 64u * TA) {
            unsigned long long tq[TA];
#pragma unroll
            for (int q = 0; q < TA; ++q) { const uint32_t row = rb + 64u * (uint32_t)q + (uint32_t)lane; tq[q] = row < ch.z ? tb[row] : 0ull; }
#pragma unroll
            for (int q = 0; q < TA; ++q) {
                const uint32_t r0 = rb + 64u * (uint32_t)q;
                if (r0 >= ch.z) break;                             // (chunk-uniform)
                const uint32_t row = r0 + (uint32_t)lane;
                const unsigned long long t = tq[q];
                const bool nz = (long long)t > 0;
                // the resident step: pass 0 is the only reader of the coverage pass's trio_bases -- it leaves them zeroed for the next step's pass (round 6)
                if (PASS == 0 && clean && t != 0ull) tb[row] = 0ull;
                const unsigned long long bal = __ballot(nz);
                if (nz) {
                    const uint32_t idx = (qh + qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))) & 127u;
                    s_qrow[idx] = row; s_qtb[idx] = t;
                }
                qn += (uint32_t)__popcll(bal);
                if (qn >= 64u) drain(64u);
            }
        }
        if (qn) drain(qn);
        n_c = nw;
    };
#ifndef HS_NO_TRANSPOSE
    if (in_reg && Hs > (uint32_t)HS_SLAB) {                   // (up to 16 haplotypes the one slab below is faster: 1.02 against 1.46 ms at ten)
        // 17 .. 64 haplotypes (round 6): LANE h owns haplotype h.  The entries that count are handed round one by one (two readlanes for the value, one for the
        // owner: scalar broadcasts) and the owner's lane adds -- in entry order, a fixed order of additions; no slabs that read the compacted rows again, no
        // reductions at the end.  (-DHS_NO_TRANSPOSE: the slabs of 16 below, as up to 16 haplotypes.)
        double acc_t = 0.0;
        uint32_t cnt_t = 0;
        unsigned long long any1_t = 0ull, any0_t = 0ull;
        auto sink_t = [&](uint32_t h, double val, bool flag) {
            unsigned long long todo = __ballot(flag);
            while (todo) {
                const int e = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
                todo &= todo - 1ull;
                const uint32_t he = (uint32_t)__builtin_amdgcn_readlane((int)h, e);
                const double ve = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(val), e), __builtin_amdgcn_readlane(__double2loint(val), e));
                if ((uint32_t)lane == he) { acc_t += ve; ++cnt_t; if (PASS == 0) { any1_t |= (unsigned long long)__double_as_longlong(ve); any0_t |= ~(unsigned long long)__double_as_longlong(ve); } }
            }
        };
        if (PASS == 0) compact_rows([&](uint32_t h, double x, bool v) { sink_t(h, v ? x : 0.0, v); });
        else
            for (uint32_t r0 = 0; r0 < n_c; r0 += 64) {
                const uint32_t i = r0 + (uint32_t)lane;
                const bool v = i < n_c;
                const uint32_t h = v ? (uint32_t)chh[ch.y + i] : 0xFFFFFFFFu;
                const double x = v ? cx[ch.y + i] : 0.0;
                double val; bool flag;
                pass_value(h, x, v, val, flag);
                sink_t(h, val, flag);
            }
        if ((uint32_t)lane < Hs) { part[ch.w + (uint32_t)lane] = HapAcc{acc_t, cnt_t, 0u}; if (PASS == 0) pbits[ch.w + (uint32_t)lane] = HapBits{any1_t, any0_t}; }
        if (PASS == 0 && lane == 0) cn[blockIdx.x] = n_c;
        return;
    }
#endif
    if (in_reg) {
        for (uint32_t slab = 0; slab * HS_SLAB < Hs; ++slab) {
            double a_[HS_SLAB];
            uint32_t c_[HS_SLAB];
#pragma unroll
            for (int k = 0; k < HS_SLAB; ++k) { a_[k] = 0.0; c_[k] = 0u; }
            auto sink_reg = [&](uint32_t h, double val, bool flag) {
                const uint32_t j = h - slab * HS_SLAB;                         // (a lane without an entry: no slab holds it)
#pragma unroll
                for (int k = 0; k < HS_SLAB; ++k) {
                    if (slab * HS_SLAB + (uint32_t)k >= Hs) break;                // (chunk-uniform) haplotypes the species does not have: 2.09 -> 1.62 ms at the reference-DB shape
                    const bool m_ = j == (uint32_t)k;
                    a_[k] += m_ ? val : 0.0;
                    c_[k] += (m_ && flag) ? 1u : 0u;
                }
            };
            // the value bits: an OR has no order, so the entries of a dense batch go straight to the haplotype's two LDS words (two LDS atomics per 64 entries --
            // carried through the compare-and-select above they cost 32 more 64-bit registers a lane and 0.2 ms over the three passes at 1e4 strains)
            if (PASS == 0 && slab == 0) compact_rows([&](uint32_t h, double x, bool v) {
                sink_reg(h, v ? x : 0.0, v);
                if (v) { const unsigned long long b_ = (unsigned long long)__double_as_longlong(x); atomicOr(&s_any[h], b_); atomicOr(&s_any[64u + h], ~b_); }
            });
            else {
                // the compacted stretch was written by this very wave, entry i by the lane that reads it back: ordering within the wave is all that is
                // needed.  (Until round 6 a __threadfence() stood here: agent scope = write-back + invalidate of the XCD's L2 on gfx950, by every chunk's
                // wave -- species of more than HS_SLAB haplotypes paid 0.84 ms for pass 0 at 125 x 50 strains where 1000 x 10 strains paid 0.53.)
                if (PASS == 0 && slab == 1) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                for (uint32_t r0 = 0; r0 < n_c; r0 += 64) {
                    const uint32_t i = r0 + (uint32_t)lane;
                    const bool v = i < n_c;
                    const uint32_t h = v ? (uint32_t)chh[ch.y + i] : 0xFFFFFFFFu;
                    const double x = v ? cx[ch.y + i] : 0.0;
                    double val; bool flag;
                    pass_value(h, x, v, val, flag);
                    sink_reg(h, val, flag);
                }
            }
#pragma unroll
            for (int k = 0; k < HS_SLAB; ++k) {
                if (slab * HS_SLAB + (uint32_t)k >= Hs) break;
                const double v = wave_reduce(a_[k], [](double x, double y) { return x + y; });
                const uint32_t c = wave_reduce(c_[k], [](uint32_t x, uint32_t y) { return x + y; });
                const uint32_t hh = slab * HS_SLAB + (uint32_t)k;
                if (lane == 0 && hh < Hs) part[ch.w + hh] = HapAcc{v, c, 0u};
            }
        }
        if (PASS == 0) {
            __syncthreads();                                       // (one wave: the LDS atomics of all lanes are done)
            if ((uint32_t)lane < Hs) pbits[ch.w + (uint32_t)lane] = HapBits{s_any[lane], s_any[64 + lane]};
            if (lane == 0) cn[blockIdx.x] = n_c;
        }
        return;
    }
    auto sink_gen = [&](uint32_t h, double val, bool flag, bool valid) {
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const uint32_t hh = (uint32_t)__builtin_amdgcn_readlane((int)h, __builtin_ctzll(todo));
            const bool mine = valid && h == hh;
            const unsigned long long sel = __ballot(mine);
            const double v = wave_reduce(mine ? val : 0.0, [](double a2, double b2) { return a2 + b2; });
            const uint32_t c = (uint32_t)__popcll(__ballot(mine && flag));
            if (lane == 0) { HapAcc t = acc[hh]; t.a += v; t.c += c; t.n += (uint32_t)__popcll(sel); acc[hh] = t; }
            if (PASS == 0) {
                const unsigned long long b_ = (unsigned long long)__double_as_longlong(val);
                const unsigned long long o1 = wave_reduce((mine && flag) ? b_ : 0ull, [](unsigned long long x, unsigned long long y) { return x | y; });
                const unsigned long long o0 = wave_reduce((mine && flag) ? ~b_ : 0ull, [](unsigned long long x, unsigned long long y) { return x | y; });
                if (lane == 0) { HapBits t = accb[hh]; t.any1 |= o1; t.any0 |= o0; accb[hh] = t; }
            }
            todo &= ~sel;
        }
    };
    if (PASS == 0) compact_rows([&](uint32_t h, double x, bool v) { sink_gen(h, v ? x : 0.0, v, v); });
    else
        for (uint32_t r0 = 0; r0 < n_c; r0 += 64) {
            const uint32_t i = r0 + (uint32_t)lane;
            const bool v = i < n_c;
            const uint32_t h = v ? (uint32_t)chh[ch.y + i] : 0xFFFFFFFFu;
            const double x = v ? cx[ch.y + i] : 0.0;
            double val; bool flag;
            pass_value(h, x, v, val, flag);
            sink_gen(h, val, flag, v);
        }
    __syncthreads();
    if (in_lds) for (uint32_t h = lane; h < Hs; h += 64) { part[ch.w + h] = acc[h]; if (PASS == 0) pbits[ch.w + h] = accb[h]; }
    if (PASS == 0 && lane == 0) cn[blockIdx.x] = n_c;
}
template <int PASS>
__global__ void __launch_bounds__(256) hap_combine_kernel(const uint32_t *__restrict__ sp_chunk_off, const uint4 *__restrict__ chunks, const uint64_t *__restrict__ hap_off,
                                                          const HapAcc *__restrict__ part, const HapBits *__restrict__ pbits, uint32_t *__restrict__ nnz, double *__restrict__ mean0, double *__restrict__ sd,
                                                          double *__restrict__ meanf) {
    // one workgroup per species; the chunks' partials of a haplotype are summed by `parts` threads (chunk c by thread c mod parts, in chunk order), the
    // parts then in part order: a fixed order of additions, whatever the launch (same bits every run)
    __shared__ double s_a[256];
    __shared__ unsigned long long s_c[256];
    __shared__ unsigned long long s_o1[PASS == 0 ? 256 : 1], s_o0[PASS == 0 ? 256 : 1];
    const uint32_t s = blockIdx.x, c0 = sp_chunk_off[s], c1 = sp_chunk_off[s + 1];
    const uint32_t h0 = (uint32_t)hap_off[s], Hs = (uint32_t)hap_off[s + 1] - h0;
    uint32_t width = 256;                                  // threads side by side over the haplotypes: the power of two >= Hs, at most 256
    if (Hs <= 128u) { width = 8; while (width < Hs) width <<= 1; }
    const uint32_t parts = 256u / width, hl = threadIdx.x % width, pt = threadIdx.x / width;
    for (uint32_t hb = 0; hb < Hs; hb += width) {
        const uint32_t h = hb + hl;
        double a = 0.0;
        unsigned long long c = 0, o1 = 0, o0 = 0;
        if (h < Hs) for (uint32_t k = c0 + pt; k < c1; k += parts) {
            const HapAcc p = part[chunks[k].w + h]; a += p.a; c += p.c;
            if (PASS == 0) { const HapBits b = pbits[chunks[k].w + h]; o1 |= b.any1; o0 |= b.any0; }
        }
        s_a[threadIdx.x] = a; s_c[threadIdx.x] = c;
        if (PASS == 0) { s_o1[threadIdx.x] = o1; s_o0[threadIdx.x] = o0; }
        __syncthreads();
        if (pt == 0 && h < Hs) {
            for (uint32_t q = 1; q < parts; ++q) { a += s_a[q * width + hl]; c += s_c[q * width + hl]; }
            if (PASS == 0) {
                for (uint32_t q = 1; q < parts; ++q) { o1 |= s_o1[q * width + hl]; o0 |= s_o0[q * width + hl]; }
                // c <= the unique-trio windows of this haplotype, and the loop runs only where every one of its non-zero windows has the same abundance: one thread,
                // c dependent additions (some 1e8 a second -- 1e5 equally covered windows hold the species' workgroup for a millisecond).  The order IS the result.
                if (c > 1 && (o1 & o0) == 0ull) {                          // all c values are the same x: the reference's sum, c sequential additions
                    const double x = __longlong_as_double((long long)o1);
                    a = 0.0;
                    for (unsigned long long i = 0; i < c; ++i) a += x;
                }
                nnz[h0 + h] = (uint32_t)c; mean0[h0 + h] = c ? a / (double)c : 0.0;                              // profile.rs:1037
            }
            else if (PASS == 1) { const double n = (double)nnz[h0 + h]; sd[h0 + h] = n > 0 ? sqrt(a / n) : 0.0; }   // :1038-1041
            else meanf[h0 + h] = c ? a / (double)c : 0.0;                 // sd == 0 -> empty -> 0.0 (:1043-1045, :1143-1147)
        }
        __syncthreads();
    }
}

// first build of a db (trio_index_build): the blocks of rows of the species -> chunks of rows, a row of partials per chunk
int hap_stats_layout(Ctx *ctx, Db *db, const uint64_t *sp_first_row, const uint64_t *sp_rows) {
    const uint32_t S = db->S;
    // rows per chunk (= per wave): 1024 where that gives a few thousand chunks; small dbs take shorter chunks, down to 128 rows, so that the pass has
    // waves for every CU (one species x 10 strains: 176 chunks of 1024 rows ran as 176 waves, 0.05 ms a pass)
    uint64_t total_rows = 0;
    for (uint32_t s = 0; s < S; ++s) total_rows += sp_rows[s];
    const uint64_t chunk_rows = std::min<uint64_t>(HS_CHUNK_ROWS, std::max<uint64_t>(128, ((total_rows / 4096 + 63) / 64) * 64));
    std::vector<uint4> chunks;
    std::vector<uint32_t> sp_off(S + 1, 0);
    uint64_t n_part = 0;
    uint32_t lds_haps = 1;
    bool global_rows = false;
    for (uint32_t s = 0; s < S; ++s) {
        sp_off[s] = (uint32_t)chunks.size();
        const uint64_t Hs = db->h_hap_off[s + 1] - db->h_hap_off[s];
        if (Hs > 64 && Hs <= HS_LDS_HAPS) lds_haps = std::max<uint32_t>(lds_haps, (uint32_t)Hs);
        if (Hs > HS_LDS_HAPS && sp_rows[s]) global_rows = true;
        // a chunk holds at least eight rows per haplotype of its species: the partials stay an eighth of the rows at most
        const uint64_t per = std::max<uint64_t>(chunk_rows, ((8 * Hs + 63) / 64) * 64);
        for (uint64_t r = 0; r < sp_rows[s]; r += per) {
            if (n_part + Hs >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "hap statistics: more than 2^32 chunk partials");
            chunks.push_back(make_uint4(s, (uint32_t)(sp_first_row[s] + r), (uint32_t)(sp_first_row[s] + std::min<uint64_t>(sp_rows[s], r + per)), (uint32_t)n_part));
            n_part += Hs;
        }
    }
    sp_off[S] = (uint32_t)chunks.size();
    db->n_stat_chunks = (uint32_t)chunks.size();
    db->n_stat_partials = n_part;
    db->stat_lds_haps = lds_haps;
    db->stat_global_rows = global_rows;
    if (chunks.empty()) chunks.push_back(make_uint4(0u, 0u, 0u, 0u));
    PTX_TRY(upload(ctx, db->d_stat_chunks, chunks.data(), chunks.size()));
    PTX_TRY(upload(ctx, db->d_sp_chunk_off, sp_off.data(), sp_off.size()));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the staging vectors go out of scope
    return 0;
}

int hap_trio_stats_launch(Ctx *ctx, Db *db, DevBuf<uint32_t> &d_nnz, DevBuf<double> &d_mean, const uint8_t *d_active, bool readers_clean) {
    if (ctx->cfg.no_absent_skip) d_active = nullptr;
    PTX_HIP(ctx, d_nnz.alloc(db->H));
    PTX_HIP(ctx, d_mean.alloc(db->H));
    if (db->H == 0) return 0;
    const uint32_t S = db->S, NC = db->n_stat_chunks;
    const uint64_t H = db->H;
    const size_t NP = (size_t)std::max<uint64_t>(db->n_stat_partials, 1);
    PTX_HIP(ctx, db->d_hap_part.alloc(4 * NP + 2 * H));   // the chunks' partials (16 B each), pass 0's value bits beside them (16 B each), then mean and sd of pass 0 / 1
    HapAcc *part = reinterpret_cast<HapAcc *>(db->d_hap_part.p);
    HapBits *pbits = reinterpret_cast<HapBits *>(db->d_hap_part.p + 2 * NP);
    double *mean0 = db->d_hap_part.p + 4 * NP, *sd = mean0 + H;
    const size_t lds_acc = (size_t)db->stat_lds_haps * sizeof(HapAcc), lds_bits = (size_t)db->stat_lds_haps * sizeof(HapBits);   // (the bits: pass 0 alone)
    // the compacted copy of the non-zero rows {value, owner}, chunk by chunk in place of the chunk's rows, and its length per chunk
    PTX_HIP(ctx, db->d_hs_x.alloc(std::max<uint64_t>(db->U, 1))); PTX_HIP(ctx, db->d_hs_h.alloc(std::max<uint64_t>(db->U, 1))); PTX_HIP(ctx, db->d_hs_n.alloc(std::max<uint32_t>(NC, 1)));
    KTimer t(ctx, "hap_rows_pass_kernel");
#define HS_PASS(PP)                                                                                                                                            \
    if (db->stat_global_rows) { KTimer tz(ctx, "hap_partials_zero_fill"); PTX_TRY(zero_fill(ctx, part, NP * (sizeof(HapAcc) + (PP == 0 ? sizeof(HapBits) : 0)))); }   /* (the bits lie behind the partials) */ \
    if (NC) hipLaunchKernelGGL(hap_rows_pass_kernel<PP>, dim3(NC), dim3(64), lds_acc + (PP == 0 ? lds_bits : 0), ctx->stream, (const uint4 *)db->d_stat_chunks.p, (const uint64_t *)db->d_hap_off.p, \
                               TRIO_HAP_PTR(db), (unsigned long long *)db->d_trio_bases.p, (const trio_len_t *)db->d_trio_len.p,          \
                               (const double *)mean0, (const double *)sd, part, pbits, db->d_hs_x.p, db->d_hs_h.p, db->d_hs_n.p, readers_clean ? 1u : 0u, d_active);  \
    hipLaunchKernelGGL(hap_combine_kernel<PP>, dim3(S), dim3(256), 0, ctx->stream, (const uint32_t *)db->d_sp_chunk_off.p, (const uint4 *)db->d_stat_chunks.p,  \
                       (const uint64_t *)db->d_hap_off.p, (const HapAcc *)part, (const HapBits *)pbits, d_nnz.p, mean0, sd, d_mean.p);
    HS_PASS(0) HS_PASS(1) HS_PASS(2)
#undef HS_PASS
    PTX_HIP(ctx, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// a9 / a13 decisions on the device, so that the strain step never waits for the host between its stages.
// Same arithmetic as the host reporting code in api_strain.cpp (IEEE f64, no contraction-sensitive forms).
// ---------------------------------------------------------------------------------------------

// first_filter_paths (profile.rs:1080-1227): which haplotypes become LP columns.  One thread per species.
__global__ void __launch_bounds__(64) first_filter_kernel(uint32_t S, const uint8_t *__restrict__ active, const uint64_t *__restrict__ hap_off,
                                                          const uint64_t *__restrict__ hto, const uint32_t *__restrict__ nnz,
                                                          const double *__restrict__ meanf, const uint8_t *__restrict__ all_same, double fr,
                                                          int shift, int32_t *__restrict__ hap_bit, int32_t *__restrict__ sp_p,
                                                          uint32_t *__restrict__ hap_nt, uint8_t *__restrict__ sp_trio) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const uint64_t h0 = hap_off[s], h1 = hap_off[s + 1];
    for (uint64_t h = h0; h < h1; ++h) { hap_bit[h] = -1; hap_nt[h] = (uint32_t)(hto[h + 1] - hto[h]); }
    sp_trio[s] = hto[h1] != hto[h0];
    int p = 0;
    if (h1 > h0 && !(active && !active[s])) {
        const uint64_t Hs = h1 - h0, Us = hto[h1] - hto[h0];
        if (Hs != 1 && Us != 0) {                                          // :1098
            for (uint64_t h = h0; h < h1; ++h) {
                const uint64_t nt = hto[h + 1] - hto[h];
                if (nt == 0) continue;                                     // :1119
                const double frac = (double)nnz[h] / (double)nt;           // :1135
                const double fm = meanf[h];
                if (shift) {                                               // :1140-1165
                    double sh;
                    if (fm >= 1.0) { sh = fr + (0.8 - fr) * fm / 100.0; if (sh > 0.8) sh = 0.8; } else sh = fr * fm;
                    if (frac < sh) continue;
                } else if (frac < fr) continue;                            // :1168
                hap_bit[h] = p++;
            }
        } else if (Hs == 1 || all_same[s]) { hap_bit[h0] = 0; p = 1; }     // :1191-1205, :1211-1224
        else { for (uint64_t h = h0; h < h1; ++h) hap_bit[h] = p++; }      // :1208 (any number of columns: see lad_prepare)
    }
    sp_p[s] = p;
}
int first_filter_launch(Ctx *ctx, const Db *db, LadBatch *lb, const uint8_t *d_active, const FilterCfg &fc) {
    const uint32_t S = db->S;
    PTX_HIP(ctx, lb->d_hap_bit.alloc(db->H)); PTX_HIP(ctx, lb->d_p.alloc(S));
    PTX_HIP(ctx, lb->d_hap_nt.alloc(db->H ? db->H : 1)); PTX_HIP(ctx, lb->d_sp_trio.alloc(S));
    hipLaunchKernelGGL(first_filter_kernel, dim3((S + 63) / 64), dim3(64), 0, ctx->stream, S, d_active, db->d_hap_off.p, db->d_hap_trio_off.p,
                       db->d_hap_nnz.p, db->d_hap_mean.p, db->d_all_same.p, fc.fr, fc.shift, lb->d_hap_bit.p, lb->d_p.p, lb->d_hap_nt.p, lb->d_sp_trio.p);
    PTX_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace ptx
