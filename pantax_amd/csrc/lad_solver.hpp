// lad_solver.hpp -- device side of a12, the batched exact LAD solver (the kernels and host launchers are in stage_lad.hip): the row searches, the LDS
// shapes, the LDS of a solver workgroup (LadLds), one view of a species' solver state (LadView) whose members are the phases of a pivot, and the
// driver lad_solve_body, which reads top to bottom as the algorithm ("The LAD solver by phase").
#pragma once
#include "lad_args.hpp"
#include "lad_device.hpp"
#include "wave.hpp"

namespace ptx {


// ---------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lower_bound_a(const double *__restrict__ a, uint32_t lo, uint32_t hi, double v) {
    while (lo < hi) { uint32_t m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; }
    return lo;
}
__device__ __forceinline__ uint32_t upper_bound_a(const double *__restrict__ a, uint32_t lo, uint32_t hi, double v) {
    while (lo < hi) { uint32_t m = (lo + hi) >> 1; if (a[m] <= v) lo = m + 1; else hi = m; }
    return lo;
}
// 64-ary searches by a whole wave64 (all lanes pass the same arguments, all get the result): each
// round probes 64 evenly spaced elements with one gather and narrows the range ~65x by a ballot, so a
// search over 10^5 rows costs 3 dependent memory round trips instead of 17.
__device__ __forceinline__ uint32_t wave_bound(const double *__restrict__ a, uint32_t lo, uint32_t hi, double v, bool upper) {
    const uint32_t lane = threadIdx.x & 63;
    while (hi - lo > 64) {
        const uint32_t m = hi - lo;
        const uint32_t pj = lo + (uint32_t)(((uint64_t)(lane + 1) * m) / 65);
        const double x = a[pj];
        const bool before = upper ? (x <= v) : (x < v);
        const int c = __popcll(__ballot(before));
        const uint32_t nlo = c > 0 ? lo + (uint32_t)(((uint64_t)c * m) / 65) + 1 : lo;
        const uint32_t nhi = c < 64 ? lo + (uint32_t)(((uint64_t)(c + 1) * m) / 65) : hi;
        lo = nlo; hi = nhi;
    }
    bool before = false;
    if (lo + lane < hi) { const double x = a[lo + lane]; before = upper ? (x <= v) : (x < v); }
    return lo + (uint32_t)__popcll(__ballot(before));
}
// Two-level search: the solver keeps every (1 << shift)-th row of its species in LDS (sample j = row
// row0 + (j << shift)); the samples narrow [lo,hi) to less than one stride without touching memory, the
// remainder is one more (usually single) round in global memory.  Same result as the plain search.
struct RowIdx {
    const double *a;      // all rows (global)
    const double *idx;    // samples (LDS)
    uint32_t row0, shift, n_idx;
    // optional LDS copy of rows [c_row0, c_row0 + c_n) (the line search caches each pattern's remaining candidates)
    const double *cache;
    uint32_t c_row0, c_n;
};
__device__ __forceinline__ double row_val(const RowIdx &r, uint32_t row) {
    const uint32_t off = row - r.c_row0;
    return off < r.c_n ? r.cache[off] : r.a[row];
}
// samples only, no memory access: rmin <= (first row of [lo,hi) that is not "before" v) <= rmax
__device__ __forceinline__ void bound_idx_range(bool coop, const RowIdx &r, uint32_t lo, uint32_t hi, double v, bool upper, uint32_t &rmin,
                                                uint32_t &rmax) {
    rmin = lo; rmax = hi;
    if (hi <= lo) return;
    const uint32_t mask = (1u << r.shift) - 1u;
    const uint32_t j0 = (lo - r.row0 + mask) >> r.shift, j1 = (hi - r.row0 + mask) >> r.shift;
    if (j1 > j0) {
        const uint32_t jj = coop ? wave_bound(r.idx, j0, j1, v, upper)
                                 : (upper ? upper_bound_a(r.idx, j0, j1, v) : lower_bound_a(r.idx, j0, j1, v));
        if (jj > j0) rmin = r.row0 + ((jj - 1) << r.shift) + 1;
        if (jj < j1) rmax = r.row0 + (jj << r.shift);
    }
}
__device__ __forceinline__ uint32_t bound_idx(bool coop, const RowIdx &r, uint32_t lo, uint32_t hi, double v, bool upper) {
    if (r.c_n && lo >= r.c_row0 && hi <= r.c_row0 + r.c_n && hi >= lo) {   // entirely inside the cached window
        const uint32_t l2 = lo - r.c_row0, h2 = hi - r.c_row0;
        const uint32_t res = coop ? wave_bound(r.cache, l2, h2, v, upper)
                                  : (upper ? upper_bound_a(r.cache, l2, h2, v) : lower_bound_a(r.cache, l2, h2, v));
        return r.c_row0 + res;
    }
    if (hi - lo > 8) {
        const uint32_t mask = (1u << r.shift) - 1u;
        const uint32_t j0 = (lo - r.row0 + mask) >> r.shift, j1 = (hi - r.row0 + mask) >> r.shift;   // samples with lo <= row < hi
        if (j1 > j0) {
            const uint32_t jj = coop ? wave_bound(r.idx, j0, j1, v, upper)
                                     : (upper ? upper_bound_a(r.idx, j0, j1, v) : lower_bound_a(r.idx, j0, j1, v));
            if (jj > j0) lo = r.row0 + ((jj - 1) << r.shift) + 1;
            if (jj < j1) hi = r.row0 + (jj << r.shift);
        }
    }
    if (coop) return wave_bound(r.a, lo, hi, v, upper);
    return upper ? upper_bound_a(r.a, lo, hi, v) : lower_bound_a(r.a, lo, hi, v);
}
__device__ __forceinline__ uint32_t lb(bool coop, const RowIdx &r, uint32_t lo, uint32_t hi, double v) { return bound_idx(coop, r, lo, hi, v, false); }
__device__ __forceinline__ uint32_t ub_(bool coop, const RowIdx &r, uint32_t lo, uint32_t hi, double v) { return bound_idx(coop, r, lo, hi, v, true); }

// ---------------------------------------------------------------------------------------------
// a12: the batched exact LAD solver
// ---------------------------------------------------------------------------------------------
constexpr int LAD_BLOCK = 256;
constexpr int LAD_KWIDE = 16;    // patterns up to which a wave searches cooperatively / the line search runs wide rounds
constexpr int LAD_KLDS = 256;    // patterns whose solver state fits the roomy LDS arrays (72 B each); more go through global scratch

// The LDS "shape" of a solver workgroup of the <= 16-column instance: how many samples the row index keeps (IDX_N), how many candidate
// rows of a line search are cached (CACHE_N) and how many patterns keep their state in LDS (KLDS; a species with more takes the
// global-scratch body).  The tables only speed one species' searches: the searches are exact at any index stride, the cache is a copy,
// and the line search ends in the same exact weighted median with or without the wide rounds -- x, status and iterations are the
// same bits under every shape.  What the shape decides is how many workgroups a CU holds (160 KiB of LDS):
//   roomy   87 912 B, 142 VGPRs -> one workgroup a CU: a few large LPs, where nothing waits for a CU and the finer index pays
//   compact 39 016 B, at most 128 VGPRs -> four a CU: more species than CUs, where co-resident workgroups hide each other's barriers and searches
// WAVES is the kernel's waves-per-SIMD hint (it holds the instance to 128 VGPRs): without it the compact instance took 130 VGPRs and three workgroups fit (cfg4, 1 000 species:
// lad_pair_kernel 1.27 ms roomy, 1.06 compact without the hint, 0.76 with it).
// lad_shape() (stage_lp_rows.hip) chooses on the host before the launch.  The 17..64-column and the wide instances have one shape.
struct LadRoomy { static constexpr uint32_t IDX_N = 4096, CACHE_N = 2048; static constexpr int KLDS = LAD_KLDS, WAVES = 1; };
struct LadCompact { static constexpr uint32_t IDX_N = 1024, CACHE_N = 1024; static constexpr int KLDS = 32, WAVES = 4; };
enum { C_LB = 0, C_UB = 1, C_PAT = 2, C_FIXED = 3 };

// -DLAD_PROFILE (tools/lad_phase_probe.sh builds such a library beside the product): thread 0 of every solver workgroup adds
// the 100-MHz wall clock spent in each phase of a pivot to prof[species * 16 + phase] and counts the visits in [+ 8 + phase].
// The marks sit in lad_solve_body, at the borders of the phases; v is the workgroup's LadView.
#define LAD_TICK(v, ph) (v).tick(ph)


template <int PS>
struct LadShared {
    double x[PS], c[PS], lam[PS], d[PS], ub[PS], fac[PS], score[PS], deriv[PS];
    long long g[PS];
    int act_type[PS], act_jk[PS], dir[PS];
    uint32_t act_i0[PS], act_i1[PS];
    double red[LAD_BLOCK / 64];
    double red_t[LAD_BLOCK / 64];
    double xs[2][LAD_BLOCK / 64][4];   // double-buffered exchange slots of the line search: one barrier per exchange
    int red_k[LAD_BLOCK / 64];
    // control words written by one thread, read by all after a barrier
    int best, bdir, done, bj, btype, status, ent_type, piv;
    uint32_t ent_k, ent_i0, ent_i1;
    double bderiv, tmax, S_lo;
};

// number of breakpoints of pattern k crossed when moving t along the search direction
__device__ __forceinline__ uint32_t crossed(bool COOP, const RowIdx &a, double rho, double s0, double eps, uint32_t st, uint32_t en,
                                            uint32_t lo, uint32_t up, double t, uint32_t c_lo, uint32_t c_hi) {
    double sv = s0 - eps + t * rho;
    if (rho > 0) return ub_(COOP, a, up + c_lo, up + c_hi, sv) - up;           // rows a_i <= sv among [up,en)
    return lo - lb(COOP, a, lo - c_hi, lo - c_lo, sv);                         // rows a_i >= sv among [st,lo)
}

// the same count from the LDS samples alone: cmin <= crossed(...) <= cmax
__device__ __forceinline__ void crossed_range(bool COOP, const RowIdx &a, double rho, double s0, double eps, uint32_t lo, uint32_t up, double t,
                                              uint32_t c_lo, uint32_t c_hi, uint32_t &cmin, uint32_t &cmax) {
    double sv = s0 - eps + t * rho;
    uint32_t rmin, rmax;
    if (rho > 0) { bound_idx_range(COOP, a, up + c_lo, up + c_hi, sv, true, rmin, rmax); cmin = rmin - up; cmax = rmax - up; }
    else { bound_idx_range(COOP, a, lo - c_hi, lo - c_lo, sv, false, rmin, rmax); cmin = lo - rmax; cmax = lo - rmin; }
}

// COOP (per species, block-uniform) = few patterns: every wave owns whole patterns (its 64 lanes search
// cooperatively, lane 0 is the "leader" that accumulates); otherwise one thread per pattern with scalar searches.
// (inside a member of LadView: names nothing but the view)
#define PAT_LOOP(k) for (uint32_t k = k0 + (COOP ? (uint32_t)(tid >> 6) : (uint32_t)tid); k < k1; k += (COOP ? LAD_BLOCK / 64 : LAD_BLOCK))
// LDS of one solver workgroup
template <int PS, int NW, class SH = LadRoomy>
struct LadLds {
    static_assert(PS <= 16 || SH::KLDS == LAD_KLDS, "only the 16-column instance has more than one shape");
    static constexpr int KLDS = SH::KLDS;
    static constexpr uint32_t IDX_N = PS <= 16 ? SH::IDX_N : 2048;     // samples of the row index (the 64-column instance spends its LDS on W and G)
    // cached candidate rows of a line search.  The 64-column instance has no LDS to spare, but its elimination scratch G is idle
    // between two basis updates: the cache of a line search lives there (8192 rows instead of 512: with a hundred patterns the
    // sample-only rounds leave a few thousand candidates, and the exact rounds then run in LDS instead of in memory)
    static constexpr bool CACHE_IN_G = NW == 1 && PS > 16;
    static constexpr uint32_t CACHE_N = PS <= 16 ? SH::CACHE_N : CACHE_IN_G ? PS * 2 * PS : 512;
    LadShared<PS> sh;
    double W[NW == 1 ? PS * PS : 1];          // wide species: W and G in global scratch (LadArgs::wide_W / wide_G)
    double G[NW == 1 ? PS * 2 * PS : 1];
    // per-pattern solver state (species with at most KLDS patterns, the usual case; else the global scratch arrays)
    double L_s[KLDS], L_rho[KLDS], L_eps[KLDS];
    uint64_t L_mask[KLDS];
    uint32_t L_lo[KLDS], L_up[KLDS], L_lslo[KLDS], L_lshi[KLDS], L_lsmid[KLDS], L_start[KLDS + 1];
    double L_idx[IDX_N];      // top level of every row search: every (1 << shift)-th row of the species' sorted rows
    double L_cache[CACHE_IN_G ? 1 : CACHE_N];
    uint32_t L_lsmid2[KLDS], L_coff[KLDS + 1], L_cn[KLDS], L_crow0[KLDS];
    // wide rounds of the line search (species with at most LAD_KWIDE patterns): crossed-count bounds of every
    // pattern at 64 pivots, and the per-wave slope contributions at those pivots
    uint32_t W_cmin[LAD_KWIDE][64], W_cmax[LAD_KWIDE][64];
    double W_acc[LAD_BLOCK / 64][2][64];
};

// The running state of one line search, handed from phase to phase (bracket -> wide rounds -> binary rounds -> walk).  Every field is block-uniform.
// ls_lo / ls_hi of the view bracket the crossed-count of every pattern; slope(t_lo) < 0 <= slope(t_hi).
struct LadSearch {
    double S0;                              // slope just after t = 0
    double t_lo = 0.0, t_hi = 0.0, S_lo, S_hi = 0.0;
    unsigned long long prev_cand = ~0ull;   // candidates left after the previous binary round, and how many exact rounds did not shrink them
    int stall = 0;
    // Rounds first run on the LDS samples alone (bounds on every crossed-count, no memory access) for
    // as long as the sign of the slope at the pivot is certain; then the remaining candidate rows of
    // every pattern are copied to LDS once and the exact rounds finish there.
    bool approx, cached = false, wide_done = false;   // wide_done: the wide rounds left only bracket-end tie groups
    int xp = 0;                             // exchange buffer in use
    __device__ __forceinline__ LadSearch(double S0_, bool use_samples) : S0(S0_), S_lo(S0_), approx(use_samples) {}
};

// One view of the solver state of species s for the length of a solve, built once at the top of lad_solve_body: where the column state (q_*), the
// pattern state (P_*: LDS arrays indexed from the species' first pattern, or the global scratch), W, G, the mask words and the row index are, and
// who this thread is.  Its member functions are the phases; each says what it reads and writes, and whether it ends on a barrier.
// USEL is a compile-time constant so that every access to the pattern state is a plain LDS (or plain global)
// instruction; a run-time choice between the two would turn them all into flat accesses.
template <int PS, bool USEL, int NW, class SH>
struct LadView {
    static_assert(NW == 1 || !USEL, "wide species keep their pattern state in global scratch");
    static constexpr uint32_t IDX_N = LadLds<PS, NW, SH>::IDX_N, CACHE_N = LadLds<PS, NW, SH>::CACHE_N;
    // NW == 0 ("huge", more than LAD_WIDEP haplotypes): the number of mask words and with it the row length of W / G are
    // run-time values, and everything that is sized by the columns lives in global scratch -- any number of columns
    static constexpr bool HUGE = NW == 0;
    static constexpr bool useL = USEL;
    static constexpr double tol = 1e-7;
    const LadArgs &A;
    LadLds<PS, NW, SH> &m;
    LadShared<PS> &sh;
    const int s, p;
    const uint32_t k0, k1;
    const int nw, ps;                 // mask words; row length of W (G: 2 * ps)
    const int tid;
    const bool COOP, leader;
    const uint32_t kofs;              // LDS arrays are indexed from the species' first pattern
    double *W, *G;
    const uint64_t *patw = nullptr;   // wide: mask words of pattern k at patw + (k - k0) * nw
    double *q_x, *q_c, *q_d, *q_ub, *q_fac, *q_score, *q_deriv;
    long long *q_g;
    int *q_type, *q_jk, *q_dir;
    uint32_t *q_i0, *q_i1;
    double *P_sc_s, *P_sc_rho, *P_pat_eps;
    uint32_t *P_sc_lo, *P_sc_up, *P_ls_lo, *P_ls_hi, *P_ls_mid;
    const uint64_t *P_pat_mask;
    const uint32_t *P_pat_start;
    double *L_idx, *L_cache;
    uint32_t *L_lsmid2, *L_coff, *L_cn, *L_crow0;
    uint32_t (*W_cmin)[64], (*W_cmax)[64];
    double (*W_acc)[2][64];
    RowIdx ra;
#ifdef LAD_PROFILE
    unsigned long long t_prev_;
#endif

    __device__ __forceinline__ LadView(const LadArgs &A_, LadLds<PS, NW, SH> &m_, int s_, int p_, uint32_t k0_, uint32_t k1_)
        : A(A_), m(m_), sh(m_.sh), s(s_), p(p_), k0(k0_), k1(k1_), nw(HUGE ? (int)A_.wide_nw[s_] : NW), ps(HUGE ? 64 * nw : PS), tid(threadIdx.x),
          COOP((k1_ - k0_) <= (uint32_t)LAD_KWIDE), leader(COOP ? ((tid & 63) == 0) : true), kofs(useL ? k0_ : 0u) {
        if constexpr (NW == 1) { W = m.W; G = m.G; }
        else {
            const uint64_t wo = A.wide_woff[A.wide_slot[s]];
            W = A.wide_W + wo; G = A.wide_G + 2 * wo;
            patw = A.pat_or + (size_t)A.wide_off[s] * LAD_WIDE_NW;
        }
        if constexpr (HUGE) {
            double *f = A.huge_f64 + (size_t)A.wide_coff[A.wide_slot[s]] * 8;
            int *i32 = A.huge_i32 + (size_t)A.wide_coff[A.wide_slot[s]] * 5;
            q_x = f; q_c = f + ps; q_d = f + 2 * ps; q_ub = f + 3 * ps; q_fac = f + 4 * ps; q_score = f + 5 * ps; q_deriv = f + 6 * ps;
            q_g = reinterpret_cast<long long *>(f + 7 * (size_t)ps);
            q_type = i32; q_jk = i32 + ps; q_dir = i32 + 2 * ps;
            q_i0 = reinterpret_cast<uint32_t *>(i32 + 3 * (size_t)ps); q_i1 = reinterpret_cast<uint32_t *>(i32 + 4 * (size_t)ps);
        } else {
            q_x = sh.x; q_c = sh.c; q_d = sh.d; q_ub = sh.ub; q_fac = sh.fac; q_score = sh.score; q_deriv = sh.deriv; q_g = sh.g;
            q_type = sh.act_type; q_jk = sh.act_jk; q_dir = sh.dir; q_i0 = sh.act_i0; q_i1 = sh.act_i1;
        }
        L_idx = m.L_idx;
        if constexpr (LadLds<PS, NW, SH>::CACHE_IN_G) L_cache = m.G; else L_cache = m.L_cache;
        L_lsmid2 = m.L_lsmid2; L_coff = m.L_coff; L_cn = m.L_cn; L_crow0 = m.L_crow0;
        W_cmin = m.W_cmin; W_cmax = m.W_cmax; W_acc = m.W_acc;
        P_sc_s = useL ? m.L_s : A.sc_s; P_sc_rho = useL ? m.L_rho : A.sc_rho; P_pat_eps = useL ? m.L_eps : A.pat_eps;
        P_sc_lo = useL ? m.L_lo : A.sc_lo; P_sc_up = useL ? m.L_up : A.sc_up; P_ls_lo = useL ? m.L_lslo : A.ls_lo;
        P_ls_hi = useL ? m.L_lshi : A.ls_hi; P_ls_mid = useL ? m.L_lsmid : A.ls_mid;
        P_pat_mask = useL ? m.L_mask : A.pat_mask;
        P_pat_start = useL ? m.L_start : A.pat_start;
        ra.a = A.row_a; ra.idx = L_idx; ra.cache = L_cache; ra.c_row0 = 0; ra.c_n = 0;
    }

    // first column slot of the species.  Read where it is used (start and final vertex), like amax in bracket(): with either value kept in the view across the
    // pivot loop the compact instances fill the 128 VGPRs of their waves-per-SIMD hint (the pair instance with two spilled), without them they take 114 / 113
    __device__ __forceinline__ uint64_t c0() const { return A.col_off[s]; }
    __device__ __forceinline__ void tick(int ph) {
#ifdef LAD_PROFILE
        if (tid == 0 && A.prof) { const unsigned long long now_ = wall_clock64(); A.prof[(size_t)s * 16 + ph] += now_ - t_prev_;
                                  A.prof[(size_t)s * 16 + 8 + ph] += 1; t_prev_ = now_; }
#else
        (void)ph;
#endif
    }
    __device__ __forceinline__ void tick_start() {
#ifdef LAD_PROFILE
        t_prev_ = wall_clock64();
#endif
    }
    // which slot of the basis holds pattern k (-1: none).  Up to LAD_WIDEP columns the slots are scanned; beyond, a map is kept.
    __device__ __forceinline__ int slot_of_pattern(uint32_t k) const {
        if constexpr (HUGE) return A.pat_act[k];
        else { int ai = -1; for (int i = 0; i < p; ++i) if (q_type[i] == C_PAT && (uint32_t)q_jk[i] == k) ai = i; return ai; }
    }
    // the row index as pattern k searches it: with the pattern's cached candidate rows once the line search has built the cache
    __device__ __forceinline__ RowIdx row_index_of(const LadSearch &ls, uint32_t k) const {
        RowIdx rk = ra;
        if (ls.cached) { rk.cache = L_cache + L_coff[k - k0]; rk.c_row0 = L_crow0[k - k0]; rk.c_n = L_cn[k - k0]; }
        return rk;
    }
    __device__ __forceinline__ void fail(int status) {   // (called block-uniformly) ends on a barrier
        if (tid == 0) { sh.status = status; sh.done = 1; }
        __syncthreads();
    }

    // ---------------------------------------------------------------- set-up
    // pattern tables to LDS (LDS state only) and the row-index samples: every (1 << shift)-th row of the species.  Writes L_mask, L_start, ra, L_idx;
    // the caller's barrier follows.
    __device__ __forceinline__ void load_tables_and_row_index() {
        if (useL) {
            for (uint32_t kk = k0 + tid; kk < k1; kk += LAD_BLOCK) m.L_mask[kk - k0] = A.pat_mask[kk];
            for (uint32_t kk = k0 + tid; kk <= k1; kk += LAD_BLOCK) m.L_start[kk - k0] = A.pat_start[kk];
        }
        ra.row0 = A.pat_start[k0];
        const uint32_t nrow = A.pat_start[k1] - ra.row0;
        uint32_t sh_ = 0;
        while (nrow && ((nrow - 1) >> sh_) + 1 > IDX_N) ++sh_;
        ra.shift = sh_;
        ra.n_idx = nrow ? ((nrow - 1) >> sh_) + 1 : 0;
        for (uint32_t j = tid; j < ra.n_idx; j += LAD_BLOCK) L_idx[j] = A.row_a[ra.row0 + (j << sh_)];
    }
    // perturbations of the right-hand sides: pat_eps of every pattern from a hash of its mask.  Reads P_pat_mask (after the barrier), writes P_pat_eps
    __device__ __forceinline__ void perturb_patterns() {
        const double amax = A.amax[s];
        const double delta = 1e-10 * (amax > 1.0 ? amax : 1.0);
        for (uint32_t kk = k0 + tid; kk < k1; kk += LAD_BLOCK)
            P_pat_eps[kk - kofs] = delta * (0.25 + 0.5 * (double)(splitmix64(P_pat_mask[kk - kofs]) >> 11) * (1.0 / 9007199254740992.0));
    }
    // box and column types, the slot map of a huge species, W = I, the control words.  Writes q_ub, q_type, q_jk, q_i0, q_i1, W, sh.done, sh.status; ends on a barrier
    __device__ __forceinline__ void start_basis() {
        for (int j = tid; j < p; j += LAD_BLOCK) {
            // box: 0 <= x <= 1.05 * max(a) (profile.rs:1327); pinned to 0 in the second solve (:1484-1488)
            double u = (A.fixed && A.fixed[c0() + j]) ? 0.0 : 1.05 * A.amax[s];
            q_ub[j] = u;
            q_type[j] = u > 0.0 ? C_LB : C_FIXED;
            q_jk[j] = j;
            q_i0[j] = q_i1[j] = 0;
        }
        if constexpr (HUGE) for (uint32_t kk = k0 + tid; kk < k1; kk += LAD_BLOCK) A.pat_act[kk] = -1;
        for (int64_t i = tid; i < (int64_t)p * p; i += LAD_BLOCK) W[(i / p) * ps + (i % p)] = (i / p == i % p) ? 1.0 : 0.0;
        if (tid == 0) { sh.done = 0; sh.status = 0; }
        __syncthreads();
    }
    // rows of one pattern must agree in every mask word (they were grouped by a hash of the words): status 7 otherwise.  Ends on a barrier; sh.done is block-uniform after it
    __device__ __forceinline__ void check_wide_masks() {
        bool bad = false;
        for (uint32_t kk = tid; kk < (k1 - k0) * (uint32_t)nw; kk += LAD_BLOCK) bad |= patw[kk] != A.pat_and[(size_t)A.wide_off[s] * LAD_WIDE_NW + kk];
        if (bad) { sh.status = 7; sh.done = 1; }
        __syncthreads();
    }

    // ---------------------------------------------------------------- a pivot
    // vertex of the perturbed problem: x = W c.  Reads the basis (q_type, q_jk, q_i0), W; writes q_c, q_x, and zeroes q_g.  Ends on a barrier
    __device__ __forceinline__ void vertex() {
        for (int j = tid; j < p; j += LAD_BLOCK) {
            int ty = q_type[j];
            q_c[j] = ty == C_UB ? q_ub[q_jk[j]] : ty == C_PAT ? ra.a[q_i0[j]] + P_pat_eps[q_jk[j] - kofs] : 0.0;
        }
        __syncthreads();
        if constexpr (NW == 1) {
            if (tid < p) {
                double v = 0.0;
                for (int i = 0; i < p; ++i) v += W[tid * ps + i] * q_c[i];
                q_x[tid] = v;
                q_g[tid] = 0;
            }
        } else {
            // W lives in global memory: a wave per row, lanes along the row (coalesced), instead of a thread per row -- four rows of a wave in flight
            // (round 6: their loads overlap; every row's sum keeps its order of additions: same bits)
            constexpr int XR = 4;
            for (int j0 = (tid >> 6) * XR; j0 < p; j0 += (LAD_BLOCK / 64) * XR) {
                double v[XR];
#pragma unroll
                for (int r = 0; r < XR; ++r) v[r] = 0.0;
                for (int i = tid & 63; i < p; i += 64) {
                    const double ci = q_c[i];
#pragma unroll
                    for (int r = 0; r < XR; ++r) if (j0 + r < p) v[r] += W[(j0 + r) * ps + i] * ci;
                }
#pragma unroll
                for (int r = 0; r < XR; ++r) {
                    const double vr = wave_reduce(v[r], [](double x_, double y_) { return x_ + y_; });
                    if ((tid & 63) == 0 && j0 + r < p) { q_x[j0 + r] = vr; q_g[j0 + r] = 0; }
                }
            }
        }
        __syncthreads();
    }
    // pattern pass: position of every pattern, integer sub-gradient g = sum sigma_k m_k.  Reads q_x, the basis; writes P_sc_s / lo / up, q_g.  Ends on a barrier
    __device__ __forceinline__ void pattern_pass() {
        PAT_LOOP(k) {
            uint64_t mk = P_pat_mask[k - kofs];
            const uint64_t *mw = NW != 1 ? patw + (size_t)(k - k0) * nw : nullptr;
            uint32_t st = P_pat_start[k - kofs], en = P_pat_start[(k + 1) - kofs];
            const int ai = slot_of_pattern(k);
            uint32_t lo, up; double sk;
            if (ai >= 0) { lo = q_i0[ai]; up = q_i1[ai]; sk = ra.a[lo] + P_pat_eps[k - kofs]; }
            else {
                if constexpr (NW == 1) sk = mdot(mk, q_x); else sk = mdotx<NW>(mw, nw, q_x);
                double sv = sk - P_pat_eps[k - kofs];
                lo = lb(COOP, ra, st, en, sv);
                up = ub_(COOP, ra, lo, en, sv);
            }
            P_sc_s[k - kofs] = sk; P_sc_lo[k - kofs] = lo; P_sc_up[k - kofs] = up;
            long long sigma = (long long)(lo - st) - (long long)(en - up);
            if (sigma && leader) {
                if constexpr (NW == 1) {
                    uint64_t bits = mk;
                    while (bits) { int j = __ffsll((long long)bits) - 1; bits &= bits - 1; atomicAdd((unsigned long long *)&q_g[j], (unsigned long long)sigma); }
                } else {
                    for (int w = 0; w < nw; ++w) {
                        uint64_t bits = mw[w];
                        while (bits) { int j = 64 * w + __ffsll((long long)bits) - 1; bits &= bits - 1; atomicAdd((unsigned long long *)&q_g[j], (unsigned long long)sigma); }
                    }
                }
            }
        }
        __syncthreads();
    }
    // multipliers lam_i = -g . W[:,i]; steepest-edge choice of the constraint to relax.  Reads q_g, W, the basis; writes q_dir, q_deriv, q_score, sh.best / bdir /
    // bderiv.  false (block-uniform, read after the barrier): no constraint improves, the vertex is optimal
    __device__ __forceinline__ bool choose_leaving() {
        for (int i = tid; i < p; i += LAD_BLOCK) {
            double sdot = 0.0, nrm = 0.0;
            if constexpr (NW == 1) {
                for (int j = 0; j < p; ++j) { double w = W[j * ps + i]; sdot += (double)q_g[j] * w; nrm += w * w; }
            } else {   // W in global memory: eight rows' loads in flight, the sums in the same order (same bits)
                int j = 0;
                for (; j + 8 <= p; j += 8) {
                    double w8[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) w8[r] = W[(j + r) * ps + i];
#pragma unroll
                    for (int r = 0; r < 8; ++r) { sdot += (double)q_g[j + r] * w8[r]; nrm += w8[r] * w8[r]; }
                }
                for (; j < p; ++j) { double w = W[j * ps + i]; sdot += (double)q_g[j] * w; nrm += w * w; }
            }
            double lam = -sdot; nrm = sqrt(nrm);
            double deriv = 0.0; int dir = 0; int ty = q_type[i];
            if (ty == C_PAT) {
                double w = (double)(q_i1[i] - q_i0[i]);
                if (lam > w + tol) { dir = +1; deriv = w - lam; } else if (lam < -w - tol) { dir = -1; deriv = w + lam; }
            } else if (ty == C_LB) { if (lam > tol) { dir = +1; deriv = -lam; } }
            else if (ty == C_UB) { if (lam < -tol) { dir = -1; deriv = lam; } }
            q_dir[i] = dir; q_deriv[i] = deriv; q_score[i] = dir ? deriv / nrm : 0.0;
        }
        __syncthreads();
        if (tid == 0) {
            int best = -1; double bs = -tol;
            for (int i = 0; i < p; ++i) if (q_dir[i] && q_score[i] < bs) { bs = q_score[i]; best = i; }
            sh.best = best;
            if (best < 0) sh.done = 1; else { sh.bdir = q_dir[best]; sh.bderiv = q_deriv[best]; }
        }
        __syncthreads();
        return !sh.done;
    }
    // direction d = bdir * W[:,best] and the ratio test against the box.  Writes q_d, sh.tmax / bj / btype (thread 0: visible after the next barrier)
    __device__ __forceinline__ void direction_and_ratio_test(const int best, const double bdir) {
        for (int j = tid; j < p; j += LAD_BLOCK) q_d[j] = bdir * W[j * ps + best];
        __syncthreads();
        if (tid == 0) {   // ratio test against the box
            double tmax = INFINITY; int bj = -1, bt = C_LB;
            for (int j = 0; j < p; ++j) {
                if (q_ub[j] <= 0.0) continue;
                double dj = q_d[j];
                if (dj < -1e-12) { double t = q_x[j] / (-dj); if (t < 0) t = 0; if (t < tmax) { tmax = t; bj = j; bt = C_LB; } }
                else if (dj > 1e-12) { double t = (q_ub[j] - q_x[j]) / dj; if (t < 0) t = 0; if (t < tmax) { tmax = t; bj = j; bt = C_UB; } }
            }
            sh.tmax = tmax; sh.bj = bj; sh.btype = bt;
        }
    }
    // line search set-up: rate rho_k of every pattern along d.  Reads q_d, the basis, P_sc_lo / up; writes P_sc_rho, P_ls_lo, P_ls_hi, sh.ent_type, sh.S_lo.
    // -> the slope just after t = 0 (block-uniform).  Ends on a barrier
    __device__ __forceinline__ double search_setup(const int best, const double bdir) {
        double part = 0.0;
        PAT_LOOP(k) {
            uint64_t mk = P_pat_mask[k - kofs];
            const int ai = slot_of_pattern(k);
            double rho;
            if (ai >= 0) rho = (ai == best) ? bdir : 0.0;   // other tight patterns stay tight: n_i . d = 0
            else { if constexpr (NW == 1) rho = mdot(mk, q_d); else rho = mdotx<NW>(patw + (size_t)(k - k0) * nw, nw, q_d); if (fabs(rho) < 1e-12) rho = 0.0; if (leader) part += fabs(rho) * (double)(P_sc_up[k - kofs] - P_sc_lo[k - kofs]); }
            P_sc_rho[k - kofs] = rho;
            P_ls_lo[k - kofs] = 0;
            P_ls_hi[k - kofs] = rho > 0 ? P_pat_start[(k + 1) - kofs] - P_sc_up[k - kofs] : rho < 0 ? P_sc_lo[k - kofs] - P_pat_start[k - kofs] : 0;
        }
        double S0 = sh.bderiv + block_sum_f64<LAD_BLOCK>(part, sh.red);   // slope just after t = 0
        if (tid == 0) { sh.ent_type = -1; sh.S_lo = S0; }
        __syncthreads();
        return S0;
    }
    // degenerate: an unsplit tie group blocks the move at t = 0 -> it enters (step length 0).  Writes sh.ent_* (or status 4).  Ends on a barrier
    __device__ __forceinline__ void degenerate_entry() {
        double tb = INFINITY; int kb = 0x7fffffff;
        PAT_LOOP(k)
            if (P_sc_rho[k - kofs] != 0.0 && P_sc_up[k - kofs] > P_sc_lo[k - kofs]) { const int ai = slot_of_pattern(k); if (ai < 0 && (int)k < kb) { kb = (int)k; tb = 0.0; } }
        kb = wave_reduce(kb, [](int x, int y) { return x < y ? x : y; });
        if ((tid & 63) == 0) sh.red_k[tid >> 6] = kb;
        __syncthreads();
        if (tid == 0) {
            int kk = sh.red_k[0];
            for (int w = 1; w < LAD_BLOCK / 64; ++w) if (sh.red_k[w] < kk) kk = sh.red_k[w];
            if (kk != 0x7fffffff) { sh.ent_type = C_PAT; sh.ent_k = (uint32_t)kk; sh.ent_i0 = P_sc_lo[kk - kofs]; sh.ent_i1 = P_sc_up[kk - kofs]; }
            else { sh.status = 4; sh.done = 1; }
        }
        (void)tb;
        __syncthreads();
    }
    // bracket: find t_hi with slope(t_hi) >= -tol (or the box bound enters).  Reads P_sc_*; writes P_ls_hi, ls.t_hi, ls.S_hi.  false (block-uniform): the box
    // bound enters, sh.ent_* (or status 2) is written and a barrier passed
    __device__ __forceinline__ bool bracket(LadSearch &ls, const double tmax) {
        const double amax = A.amax[s];   // (read here, not kept in the view across the pivot loop: see c0())
        ls.t_hi = isfinite(tmax) ? tmax : (amax > 1.0 ? amax : 1.0);
        ls.S_hi = 0.0;
        bool bound_enters = false;
        for (int grow = 0; grow < 200; ++grow) {
            double acc = 0.0;
            PAT_LOOP(k) {
                double rho = P_sc_rho[k - kofs];
                if (rho == 0.0) continue;
                uint32_t st = P_pat_start[k - kofs], en = P_pat_start[(k + 1) - kofs];
                uint32_t cmax = rho > 0 ? en - P_sc_up[k - kofs] : P_sc_lo[k - kofs] - st;
                uint32_t c = crossed(COOP, ra, rho, P_sc_s[k - kofs], P_pat_eps[k - kofs], st, en, P_sc_lo[k - kofs], P_sc_up[k - kofs], ls.t_hi, 0, cmax);
                P_ls_hi[k - kofs] = c;
                if (leader) acc += fabs(rho) * 2.0 * (double)c;
            }
            ls.S_hi = ls.S0 + block_sum_f64<LAD_BLOCK>(acc, sh.red);
            if (ls.S_hi >= -tol) break;
            if (isfinite(tmax)) { bound_enters = true; break; }
            ls.t_hi *= 4.0;
            if (grow == 199) bound_enters = true;   // cannot happen: slope(inf) >= 0 for a LAD objective
        }
        if (bound_enters) {
            if (tid == 0) {
                if (sh.bj >= 0) { sh.ent_type = sh.btype; sh.ent_k = (uint32_t)sh.bj; }
                else { sh.status = 2; sh.done = 1; }
            }
            __syncthreads();
        }
        return !bound_enters;
    }
    // copy every pattern's remaining candidate rows to the LDS cache (L_cache; offsets in L_coff / L_cn / L_crow0).  Ends on a barrier
    __device__ __forceinline__ void build_cache(LadSearch &ls) {
        if (tid == 0) {
            uint32_t off = 0;
            for (uint32_t kk = 0; kk < k1 - k0; ++kk) {
                const double rho = m.L_rho[kk];
                const uint32_t cl = m.L_lslo[kk], ch = m.L_lshi[kk];
                const uint32_t n = (rho != 0.0 && ch > cl) ? ch - cl : 0u;
                L_coff[kk] = off; L_cn[kk] = n;
                L_crow0[kk] = rho > 0 ? m.L_up[kk] + cl : m.L_lo[kk] - ch;
                off += n;
            }
            L_coff[k1 - k0] = off;
        }
        __syncthreads();
        const uint32_t total = L_coff[k1 - k0];
        for (uint32_t e = tid; e < total; e += LAD_BLOCK) {
            uint32_t kk = 0, kh = k1 - k0;   // last pattern whose first cached row is <= e (empty patterns repeat offsets)
            while (kh - kk > 1) { const uint32_t km_ = (kk + kh) >> 1; if (L_coff[km_] <= e) kk = km_; else kh = km_; }
            L_cache[e] = ra.a[L_crow0[kk] + (e - L_coff[kk])];
        }
        __syncthreads();
        ls.cached = true;
    }
    // wide rounds (few patterns, LDS state): the slope is bounded (samples) or evaluated (cached rows) at 64 pivots at once.
    // Pivots are evenly spaced candidates of the pattern that holds the most weighted candidates,
    // lane order = increasing t; every lane searches each pattern of its wave for its own pivot; the
    // bracket moves to the last pivot that is certainly before the minimiser and the first that is
    // certainly at or past it.  ~64x fewer candidates per round instead of 2x.
    // Reads P_sc_*; writes P_ls_lo / hi, the bracket of ls, ls.wide_done, ls.approx, maybe the cache.  Every break / continue is block-uniform.  Ends on a barrier
    __device__ __forceinline__ void wide_rounds(LadSearch &ls) {
        const int lane = tid & 63, wave = tid >> 6;
        bool exact = false;
        unsigned long long prev_w = ~0ull;
        for (int wr = 0; wr < 64; ++wr) {
            double cs = 0.0, wb = 0.0;
            int kbest = 0x7fffffff;
            PAT_LOOP(k) {
                const double rho = P_sc_rho[k - kofs];
                const uint32_t cl = P_ls_lo[k - kofs], ch = P_ls_hi[k - kofs];
                if (rho == 0.0 || ch <= cl) continue;
                cs += (double)(ch - cl);
                const double w = fabs(rho) * (double)(ch - cl);
                if (w > wb || (w == wb && (int)k < kbest)) { wb = w; kbest = (int)k; }
            }
            if (lane == 0) { sh.xs[ls.xp][wave][0] = cs; sh.xs[ls.xp][wave][1] = wb; sh.xs[ls.xp][wave][2] = (double)kbest; }
            __syncthreads();
            cs = 0.0; wb = 0.0; kbest = 0x7fffffff;
#pragma unroll
            for (int w = 0; w < LAD_BLOCK / 64; ++w) {
                cs += sh.xs[ls.xp][w][0];
                const double w2 = sh.xs[ls.xp][w][1]; const int k2 = (int)sh.xs[ls.xp][w][2];
                if (w2 > wb || (w2 == wb && w2 > 0.0 && k2 < kbest)) { wb = w2; kbest = k2; }
            }
            ls.xp ^= 1;
            const unsigned long long cand = (unsigned long long)cs;
            if (cand <= 8 || kbest == 0x7fffffff) { ls.wide_done = true; break; }
            // exact rounds that cannot move the bracket any more: what is left sits on its ends (tie groups)
            if (cand == prev_w) { if (exact) { ls.wide_done = true; break; } exact = true; }
            prev_w = cand;
            if (exact && !ls.cached) { if (cand > CACHE_N) break; build_cache(ls); }
            // pivots of the heaviest pattern
            const uint32_t kq = (uint32_t)kbest - kofs;
            const double rho_b = P_sc_rho[kq], s_b = P_sc_s[kq], eps_b = P_pat_eps[kq];
            const uint32_t rl = rho_b > 0 ? P_sc_up[kq] + P_ls_lo[kq] : P_sc_lo[kq] - P_ls_hi[kq];
            const uint32_t rh = rho_b > 0 ? P_sc_up[kq] + P_ls_hi[kq] : P_sc_lo[kq] - P_ls_lo[kq];
            uint32_t pa, pn;   // pivot positions [pa, pa + pn): sample indices or rows
            if (!exact) {
                const uint32_t msk = (1u << ra.shift) - 1u;
                pa = (rl - ra.row0 + msk) >> ra.shift;
                const uint32_t pb = (rh - ra.row0 + msk) >> ra.shift;
                pn = pb > pa ? pb - pa : 0u;
                if (pn < 2) { exact = true; prev_w = ~0ull; continue; }   // too few samples left among the candidates
            } else { pa = rl; pn = rh - rl; }
            const uint32_t pm = pn < 64u ? pn : 64u;
            double t_piv = 0.0;
            bool valid = (uint32_t)lane < pm;
            if (valid) {
                const uint32_t q = (uint32_t)(((uint64_t)(2 * lane + 1) * pn) / (2ull * pm));
                const uint32_t pos = rho_b > 0 ? pa + q : pa + pn - 1 - q;
                double av;
                if (!exact) av = ra.idx[pos];
                else { const RowIdx rk = row_index_of(ls, (uint32_t)kbest); av = row_val(rk, pos); }
                t_piv = (av + eps_b - s_b) / rho_b;
                if (t_piv < 0) t_piv = 0;
                valid = t_piv > ls.t_lo && t_piv < ls.t_hi;
            }
            double a0 = 0.0, a1 = 0.0;
            PAT_LOOP(k) {
                const double rho = P_sc_rho[k - kofs];
                if (rho == 0.0) continue;
                uint32_t cmin = 0, cmax = 0;
                if (valid) {
                    if (!exact) crossed_range(false, ra, rho, P_sc_s[k - kofs], P_pat_eps[k - kofs], P_sc_lo[k - kofs], P_sc_up[k - kofs], t_piv,
                                              P_ls_lo[k - kofs], P_ls_hi[k - kofs], cmin, cmax);
                    else {
                        const RowIdx rk = row_index_of(ls, k);
                        cmin = cmax = crossed(false, rk, rho, P_sc_s[k - kofs], P_pat_eps[k - kofs], P_pat_start[k - kofs], P_pat_start[(k + 1) - kofs],
                                              P_sc_lo[k - kofs], P_sc_up[k - kofs], t_piv, P_ls_lo[k - kofs], P_ls_hi[k - kofs]);
                    }
                }
                W_cmin[k - k0][lane] = cmin; W_cmax[k - k0][lane] = cmax;
                a0 += fabs(rho) * 2.0 * (double)cmin; a1 += fabs(rho) * 2.0 * (double)cmax;
            }
            W_acc[wave][0][lane] = a0; W_acc[wave][1][lane] = a1;
            __syncthreads();
            double S_min = ls.S0, S_max = ls.S0;
#pragma unroll
            for (int w = 0; w < LAD_BLOCK / 64; ++w) { S_min += W_acc[w][0][lane]; S_max += W_acc[w][1][lane]; }
            const unsigned long long mlo = __ballot(valid && S_max < -tol), mhi = __ballot(valid && S_min >= -tol);
            const int jl = mlo ? 63 - __clzll((long long)mlo) : -1;
            const int jh = mhi ? __ffsll((long long)mhi) - 1 : -1;
            if ((jl < 0 && jh < 0) || (jl >= 0 && jh >= 0 && jl >= jh)) { if (exact) { ls.wide_done = true; break; } exact = true; prev_w = ~0ull; continue; }
            if (jl >= 0) {
                ls.t_lo = __shfl(t_piv, jl); ls.S_lo = __shfl(S_max, jl);
                PAT_LOOP(k) if (P_sc_rho[k - kofs] != 0.0) P_ls_lo[k - kofs] = W_cmin[k - k0][jl];
            }
            if (jh >= 0) {
                ls.t_hi = __shfl(t_piv, jh); ls.S_hi = __shfl(S_min, jh);
                PAT_LOOP(k) if (P_sc_rho[k - kofs] != 0.0) P_ls_hi[k - kofs] = W_cmax[k - k0][jh];
            }
        }
        if (exact) ls.approx = false;
        __syncthreads();   // bracket state written by the owning waves is read by everyone below
    }
    // one exchange of a binary round: candidate count (sum) and the heaviest pattern's proposed pivot (its median remaining breakpoint)
    __device__ __forceinline__ void propose_pivot(LadSearch &ls, unsigned long long &cand, double &bt) {
        double wbest = 0.0, tprop = 0.0; cand = 0;
        PAT_LOOP(k) {
            double rho = P_sc_rho[k - kofs];
            uint32_t cl = P_ls_lo[k - kofs], ch = P_ls_hi[k - kofs];
            if (rho == 0.0 || ch <= cl) continue;
            if (leader) cand += ch - cl;
            double w = fabs(rho) * (double)(ch - cl);
            if (w > wbest) {
                uint32_t mth = cl + (ch - cl) / 2;   // mth breakpoint ahead (0-based) of this pattern
                uint32_t r = rho > 0 ? P_sc_up[k - kofs] + mth : P_sc_lo[k - kofs] - 1 - mth;
                double av;
                bool have = false;
                if (ls.approx) {   // a sampled row among the candidates serves as well as the exact median
                    const uint32_t rl = rho > 0 ? P_sc_up[k - kofs] + cl : P_sc_lo[k - kofs] - ch;
                    const uint32_t rh = rho > 0 ? P_sc_up[k - kofs] + ch : P_sc_lo[k - kofs] - cl;
                    uint32_t j = (r - ra.row0) >> ra.shift;
                    uint32_t rs = ra.row0 + (j << ra.shift);
                    if (rs < rl) { ++j; rs += 1u << ra.shift; }
                    if (rs < rh && j < ra.n_idx) { av = ra.idx[j]; have = true; }
                }
                if (!have) { const RowIdx rk = row_index_of(ls, k); av = row_val(rk, r); }
                double t = (av + P_pat_eps[k - kofs] - P_sc_s[k - kofs]) / rho;
                wbest = w; tprop = t < 0 ? 0 : t;
            }
        }
        // one exchange: candidate count (sum) and the heaviest proposal (max over the block, ties -> smaller t)
        {
            double cs = wave_reduce((double)cand, [](double x, double y) { return x + y; });
            wave_reduce_pair(wbest, tprop, [](double w2, double t2, double w, double t) { return w2 > w || (w2 == w && t2 < t); });
            if ((tid & 63) == 0) { sh.xs[ls.xp][tid >> 6][0] = cs; sh.xs[ls.xp][tid >> 6][1] = wbest; sh.xs[ls.xp][tid >> 6][2] = tprop; }
            __syncthreads();
            cs = 0.0;
            double bw = sh.xs[ls.xp][0][1];
            bt = sh.xs[ls.xp][0][2];
#pragma unroll
            for (int w = 0; w < LAD_BLOCK / 64; ++w) {
                cs += sh.xs[ls.xp][w][0];
                const double w2 = sh.xs[ls.xp][w][1], t2 = sh.xs[ls.xp][w][2];
                if (w > 0 && (w2 > bw || (w2 == bw && t2 < bt))) { bw = w2; bt = t2; }
            }
            ls.xp ^= 1;
            cand = (unsigned long long)cs;
        }
    }
    // a round on the LDS samples alone: true when the bracket moved (the slope's sign at t_mid was certain), false: undecided at sample resolution
    __device__ __forceinline__ bool sample_round(LadSearch &ls, const double t_mid) {
        double acc0 = 0.0, acc1 = 0.0;
        PAT_LOOP(k) {
            double rho = P_sc_rho[k - kofs];
            if (rho == 0.0) continue;
            uint32_t cmin, cmax;
            crossed_range(COOP, ra, rho, P_sc_s[k - kofs], P_pat_eps[k - kofs], P_sc_lo[k - kofs], P_sc_up[k - kofs], t_mid,
                          P_ls_lo[k - kofs], P_ls_hi[k - kofs], cmin, cmax);
            P_ls_mid[k - kofs] = cmin; L_lsmid2[k - k0] = cmax;
            if (leader) { acc0 += fabs(rho) * 2.0 * (double)cmin; acc1 += fabs(rho) * 2.0 * (double)cmax; }
        }
        acc0 = wave_reduce(acc0, [](double x, double y) { return x + y; });
        acc1 = wave_reduce(acc1, [](double x, double y) { return x + y; });
        if ((tid & 63) == 0) { sh.xs[ls.xp][tid >> 6][0] = acc0; sh.xs[ls.xp][tid >> 6][1] = acc1; }
        __syncthreads();
        double S_min = ls.S0, S_max = ls.S0;
#pragma unroll
        for (int w = 0; w < LAD_BLOCK / 64; ++w) { S_min += sh.xs[ls.xp][w][0]; S_max += sh.xs[ls.xp][w][1]; }
        ls.xp ^= 1;
        if (S_max < -tol) {          // certainly still descending at t_mid
            PAT_LOOP(k) if (P_sc_rho[k - kofs] != 0.0) P_ls_lo[k - kofs] = P_ls_mid[k - kofs];
            ls.t_lo = t_mid; ls.S_lo = S_max;
            return true;
        }
        if (S_min >= -tol) {         // certainly past the minimiser
            PAT_LOOP(k) if (P_sc_rho[k - kofs] != 0.0) P_ls_hi[k - kofs] = L_lsmid2[k - k0];
            ls.t_hi = t_mid; ls.S_hi = S_min;
            return true;
        }
        ls.approx = false;              // undecided at sample resolution: exact from here on (same pivot)
        return false;
    }
    // an exact round: the slope at t_mid from every pattern's crossed count; one end of the bracket moves there
    __device__ __forceinline__ void exact_round(LadSearch &ls, const double t_mid) {
        double acc = 0.0;
        PAT_LOOP(k) {
            double rho = P_sc_rho[k - kofs];
            if (rho == 0.0) continue;
            const RowIdx rk = row_index_of(ls, k);
            uint32_t c = crossed(COOP, rk, rho, P_sc_s[k - kofs], P_pat_eps[k - kofs], P_pat_start[k - kofs], P_pat_start[(k + 1) - kofs], P_sc_lo[k - kofs], P_sc_up[k - kofs],
                                 t_mid, P_ls_lo[k - kofs], P_ls_hi[k - kofs]);
            P_ls_mid[k - kofs] = c;
            if (leader) acc += fabs(rho) * 2.0 * (double)c;
        }
        acc = wave_reduce(acc, [](double x, double y) { return x + y; });
        if ((tid & 63) == 0) sh.xs[ls.xp][tid >> 6][0] = acc;
        __syncthreads();
        double S_mid = ls.S0;
#pragma unroll
        for (int w = 0; w < LAD_BLOCK / 64; ++w) S_mid += sh.xs[ls.xp][w][0];
        ls.xp ^= 1;
        bool go_hi = S_mid >= -tol;
        PAT_LOOP(k) {
            if (P_sc_rho[k - kofs] == 0.0) continue;
            if (go_hi) P_ls_hi[k - kofs] = P_ls_mid[k - kofs]; else P_ls_lo[k - kofs] = P_ls_mid[k - kofs];
        }
        if (go_hi) { ls.t_hi = t_mid; ls.S_hi = S_mid; } else { ls.t_lo = t_mid; ls.S_lo = S_mid; }
    }
    // narrow the bracket.  Rounds alternate between pivots so that the search is
    // both scale-free and robust to many patterns: the median remaining breakpoint of
    // the pattern that still holds the most weighted candidates, a secant step on the slope, the midpoint in t.
    // Reads P_sc_*; writes P_ls_lo / mid / hi and ls.  Every break / continue is block-uniform (cand, the slopes and ls come out of exchanges)
    __device__ __forceinline__ void binary_rounds(LadSearch &ls, const bool quick) {
        for (int bi = 0; bi < 400 && !quick; ++bi) {
            unsigned long long cand; double bt;
            propose_pivot(ls, cand, bt);

            if (cand <= 8) break;
            // three exact rounds (one of each pivot kind) without shrinking: only tie groups remain -> walk them
            const bool shrunk = cand != ls.prev_cand;
            ls.prev_cand = cand;
            if (ls.approx) { if (!shrunk) ls.approx = false; }
            else {
                ls.stall = shrunk ? 0 : ls.stall + 1;
                if (ls.stall >= 3) break;
            }
            if (!ls.approx && !ls.cached && useL && cand <= CACHE_N) build_cache(ls);
            double t_mid;
            const int mode = bi % 3;   // 0: heaviest pattern's median breakpoint, 1: secant on the slope, 2: midpoint
            if (mode == 0) { t_mid = bt; if (!(t_mid >= ls.t_lo && t_mid <= ls.t_hi)) t_mid = 0.5 * (ls.t_lo + ls.t_hi); }
            else {
                const double den = ls.S_hi - ls.S_lo;
                t_mid = (mode == 1 && den > 0.0) ? ls.t_lo + (ls.t_hi - ls.t_lo) * (-ls.S_lo / den) : 0.5 * (ls.t_lo + ls.t_hi);
                if (!(t_mid > ls.t_lo && t_mid < ls.t_hi)) t_mid = 0.5 * (ls.t_lo + ls.t_hi);
            }
            if (ls.approx && sample_round(ls, t_mid)) continue;
            exact_round(ls, t_mid);
        }
    }
    // walk the few remaining breakpoint groups in order of t until the slope turns: the group it turns in enters.  Reads P_sc_*, P_ls_*; writes P_ls_lo, sh.S_lo,
    // sh.ent_* (or status 5).  true (block-uniform, read after a barrier): an entering constraint was found or the solve failed
    __device__ __forceinline__ bool walk(const LadSearch &ls, const bool quick) {
        // slope of the crossed set the walk starts from (sample-only rounds leave lower bounds in ls_lo, so
        // it is recomputed from the counts; with exact counts it equals the slope at t_lo)
        {
            double acc = 0.0;
            PAT_LOOP(k) { double rho = P_sc_rho[k - kofs]; if (rho != 0.0 && leader) acc += fabs(rho) * 2.0 * (double)P_ls_lo[k - kofs]; }
            const double S_start = ls.S0 + block_sum_f64<LAD_BLOCK>(acc, sh.red);
            if (tid == 0) sh.S_lo = S_start;
        }
        __syncthreads();
        // ---- walk the few remaining breakpoint groups in order of t.  ls_lo may split a tie group (sample
        // bounds are not group aligned): a step crosses the rest of the group its first uncrossed row is in.
        for (int step = 0, cap = quick ? 48 : 4096; step < cap; ++step) {
            double tb = INFINITY; int kb = 0x7fffffff;
            PAT_LOOP(k) {
                double rho = P_sc_rho[k - kofs];
                if (rho == 0.0 || P_ls_hi[k - kofs] <= P_ls_lo[k - kofs]) continue;
                uint32_t r = rho > 0 ? P_sc_up[k - kofs] + P_ls_lo[k - kofs] : P_sc_lo[k - kofs] - 1 - P_ls_lo[k - kofs];
                const RowIdx rk = row_index_of(ls, k);
                double t = (row_val(rk, r) + P_pat_eps[k - kofs] - P_sc_s[k - kofs]) / rho;
                if (t < 0) t = 0;
                if (t < tb || (t == tb && (int)k < kb)) { tb = t; kb = (int)k; }
            }
            wave_reduce_pair(tb, kb, [](double t2, int k2, double t, int k) { return t2 < t || (t2 == t && k2 < k); });
            if ((tid & 63) == 0) { sh.red_t[tid >> 6] = tb; sh.red_k[tid >> 6] = kb; }
            __syncthreads();
            if (tid < 64) {   // wave 0: its lanes search together, lane 0 writes
                const bool l0 = tid == 0;
                double tt = sh.red_t[0]; int kk = sh.red_k[0];
                for (int w = 1; w < LAD_BLOCK / 64; ++w) if (sh.red_t[w] < tt || (sh.red_t[w] == tt && sh.red_k[w] < kk)) { tt = sh.red_t[w]; kk = sh.red_k[w]; }
                if (kk == 0x7fffffff) {
                    // bracket exhausted without crossing (rounding): fall back to the box bound or fail
                    if (l0) { if (sh.bj >= 0 && isfinite(sh.tmax)) { sh.ent_type = sh.btype; sh.ent_k = (uint32_t)sh.bj; } else { sh.status = 5; sh.done = 1; } }
                } else {
                    double rho = P_sc_rho[kk - kofs];
                    uint32_t st = P_pat_start[kk - kofs], en = P_pat_start[(kk + 1) - kofs];
                    uint32_t r = rho > 0 ? P_sc_up[kk - kofs] + P_ls_lo[kk - kofs] : P_sc_lo[kk - kofs] - 1 - P_ls_lo[kk - kofs];
                    const RowIdx rk = row_index_of(ls, (uint32_t)kk);
                    double av = row_val(rk, r);
                    // extent [g0,g1) of the tie group of r: inside the cached rows first; a group that reaches the
                    // end of the cached rows is settled by the neighbouring row, else by the full searches
                    uint32_t g0 = r, g1 = r + 1;
                    bool open0 = true, open1 = true;
                    if (r - rk.c_row0 < rk.c_n) {
                        const uint32_t o = r - rk.c_row0;
                        g0 = rk.c_row0 + wave_bound(rk.cache, 0, o, av, false);
                        g1 = rk.c_row0 + wave_bound(rk.cache, o + 1, rk.c_n, av, true);
                        open0 = g0 == rk.c_row0 && g0 > st;
                        open1 = g1 == rk.c_row0 + rk.c_n && g1 < en;
                    }
                    if (g0 <= st) open0 = false;
                    if (g1 >= en) open1 = false;
                    const double below = open0 ? ra.a[g0 - 1] : 0.0, above = open1 ? ra.a[g1] : 0.0;
                    if (open0 && below != av) open0 = false;
                    if (open1 && above != av) open1 = false;
                    if (open0) g0 = lb(true, ra, st, g0, av);
                    if (open1) g1 = ub_(true, ra, g1, en, av);
                    uint32_t gs = rho > 0 ? g1 - r : r - g0 + 1;      // rows of the group not crossed yet
                    double Sn = sh.S_lo + 2.0 * fabs(rho) * (double)gs;
                    if (l0) {
                        P_ls_lo[kk - kofs] += gs;
                        sh.S_lo = Sn;
                        if (Sn >= -tol) { sh.ent_type = C_PAT; sh.ent_k = (uint32_t)kk; sh.ent_i0 = g0; sh.ent_i1 = g1; }
                    }
                }
            }
            __syncthreads();
            if (sh.ent_type >= 0 || sh.done) break;
        }
        return sh.ent_type >= 0 || sh.done;
    }
    // constraint `best` leaves, the entering one takes its slot.  Writes the basis (and the slot map of a huge species).  Ends on a barrier
    __device__ __forceinline__ void swap_basis(const int best) {
        if (tid == 0) {
            if constexpr (HUGE) {
                if (q_type[best] == C_PAT) A.pat_act[q_jk[best]] = -1;
                if (sh.ent_type == C_PAT) A.pat_act[sh.ent_k] = best;
            }
            q_type[best] = sh.ent_type;
            q_jk[best] = (int)sh.ent_k;
            q_i0[best] = sh.ent_i0; q_i1[best] = sh.ent_i1;
        }
        __syncthreads();
    }
    // rank-one update of W for the row of N that changed.  true (block-uniform): the divisor is small, W must be rebuilt.  Uses q_fac, q_score.  Ends on a barrier
    __device__ __forceinline__ bool rank_one_update(const int best) {
        for (int c_ = tid; c_ < p; c_ += LAD_BLOCK) {
            double y;
            if (q_type[best] == C_PAT) {
                y = 0.0;
                if constexpr (NW == 1) {
                    uint64_t bits = P_pat_mask[q_jk[best] - kofs];
                    while (bits) { const int j = __ffsll((long long)bits) - 1; bits &= bits - 1; y += W[j * ps + c_]; }
                } else {
                    const uint64_t *mb = patw + (size_t)((uint32_t)q_jk[best] - k0) * nw;
                    for (int w = 0; w < nw; ++w) {     // four rows' loads in flight, added in bit order (same bits as one at a time)
                        uint64_t bits = mb[w];
                        while (bits) {
                            int jj[4]; bool on[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) { on[r] = bits != 0ull; jj[r] = on[r] ? 64 * w + __ffsll((long long)bits) - 1 : 0; bits &= bits - 1; }
                            double t4[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) t4[r] = W[jj[r] * ps + c_];
#pragma unroll
                            for (int r = 0; r < 4; ++r) if (on[r]) y += t4[r];
                        }
                    }
                }
            } else y = W[q_jk[best] * ps + c_];
            q_fac[c_] = y;
            q_score[c_] = W[c_ * ps + best];
        }
        __syncthreads();
        const double alpha = q_fac[best];
        if (fabs(alpha) < 1e-7) return true;   // (block-uniform: read from LDS after the barrier)
        const double ainv = 1.0 / alpha;
        if constexpr (NW == 1) {
            for (int i = tid; i < p * p; i += LAD_BLOCK) {
                const int j = i / p, cc = i % p;
                W[j * ps + cc] -= q_score[j] * (q_fac[cc] - (cc == best ? 1.0 : 0.0)) * ainv;
            }
        } else {   // W in global memory: a wave per row, lanes along it -- coalesced, no divisions; every element's arithmetic is the line above
            for (int j = tid >> 6; j < p; j += LAD_BLOCK / 64) {
                const double sj = q_score[j];
#pragma unroll 4
                for (int cc = tid & 63; cc < p; cc += 64) W[j * ps + cc] -= sj * (q_fac[cc] - (cc == best ? 1.0 : 0.0)) * ainv;
            }
        }
        __syncthreads();
        return false;
    }
    // verify W with one probe vector: |N (W v) - v|.  true (block-uniform): the probe fails, W must be rebuilt.  Uses q_fac
    __device__ __forceinline__ bool inverse_probe_fails() {
        auto probe_v = [](int i) { return 1.0 + 0.25 * (double)(i % 7); };
        for (int j = tid >> 6; j < p; j += LAD_BLOCK / 64) {          // u = W v: a wave per row
            double a_ = 0.0;
            for (int i = tid & 63; i < p; i += 64) a_ += W[j * ps + i] * probe_v(i);
            a_ = wave_reduce(a_, [](double x_, double y_) { return x_ + y_; });
            if ((tid & 63) == 0) q_fac[j] = a_;
        }
        __syncthreads();
        double worst = 0.0;
        for (int i = tid; i < p; i += LAD_BLOCK) {                    // row i of N: a pattern's membership or a unit vector
            const double r_ = q_type[i] == C_PAT ? mdotx<NW>(patw + (size_t)((uint32_t)q_jk[i] - k0) * nw, nw, q_fac) : q_fac[q_jk[i]];
            worst = fmax(worst, fabs(r_ - probe_v(i)));
        }
        worst = block_max_f64<LAD_BLOCK>(worst, sh.red);
        return !(worst <= 1e-10);
    }
    // W = N^-1 from scratch by Gauss-Jordan with partial pivoting in G.  false (block-uniform): N is singular, status 3.  Ends on a barrier
    __device__ __forceinline__ bool rebuild_inverse() {
        for (int i = tid; i < p * 2 * p; i += LAD_BLOCK) {
            int r = i / (2 * p), cc = i % (2 * p);
            double v;
            if (cc >= p) v = (cc - p == r) ? 1.0 : 0.0;
            else if (q_type[r] == C_PAT) {
                if constexpr (NW == 1) v = (P_pat_mask[q_jk[r] - kofs] >> cc) & 1ull ? 1.0 : 0.0;
                else v = (patw[(size_t)((uint32_t)q_jk[r] - k0) * nw + (cc >> 6)] >> (cc & 63)) & 1ull ? 1.0 : 0.0;
            }
            else v = (q_jk[r] == cc) ? 1.0 : 0.0;
            G[r * 2 * ps + cc] = v;
        }
        __syncthreads();
        static_assert(HUGE || PS <= LAD_BLOCK, "one matrix row per thread in the pivot search");
        for (int col = 0; col < p; ++col) {
            // partial pivoting, all rows at once: thread r loads G[r][col] (its elimination factor as well), rows >= col compete
            // for the largest magnitude (ties: the smallest row, as a serial scan would choose); three barriers per column
            double cand_v = 0.0;
            int cand_r = 0x7fffffff;
            for (int r = tid; r < p; r += LAD_BLOCK) {   // (one trip up to LAD_WIDEP columns)
                const double v = G[r * 2 * ps + col];
                q_fac[r] = v;
                if (r >= col && (cand_r == 0x7fffffff || fabs(v) > fabs(cand_v))) { cand_v = v; cand_r = r; }   // ascending r: ties keep the smaller row
            }
            wave_reduce_pair(cand_v, cand_r, [](double v2, int r2, double v1, int r1) { return r2 != 0x7fffffff && (r1 == 0x7fffffff || fabs(v2) > fabs(v1) || (fabs(v2) == fabs(v1) && r2 < r1)); });
            if ((tid & 63) == 0) { sh.red_t[tid >> 6] = cand_v; sh.red_k[tid >> 6] = cand_r; }
            __syncthreads();
            double pv = sh.red_t[0]; int piv = sh.red_k[0];
#pragma unroll
            for (int w = 1; w < LAD_BLOCK / 64; ++w) {
                const double v2 = sh.red_t[w]; const int r2 = sh.red_k[w];
                if (r2 != 0x7fffffff && (piv == 0x7fffffff || fabs(v2) > fabs(pv) || (fabs(v2) == fabs(pv) && r2 < piv))) { pv = v2; piv = r2; }
            }
            if (!(fabs(pv) >= 1e-12)) { if (tid == 0) { sh.status = 3; sh.done = 1; } __syncthreads(); break; }   // (block-uniform)
            const double dinv = 1.0 / pv;
            // row `piv` scaled becomes row `col`; the old row `col` moves to `piv`
            for (int c2 = tid; c2 < 2 * p; c2 += LAD_BLOCK) {
                const double a_ = G[col * 2 * ps + c2], b_ = G[piv * 2 * ps + c2];
                G[col * 2 * ps + c2] = b_ * dinv;
                if (piv != col) G[piv * 2 * ps + c2] = a_;
            }
            const double f_colrow = q_fac[col];   // the factor of the row that now sits at `piv`
            __syncthreads();
            for (int i = tid; i < p * 2 * p; i += LAD_BLOCK) {
                const int r = i / (2 * p), cc = i % (2 * p);
                if (r != col) G[r * 2 * ps + cc] -= (r == piv ? f_colrow : q_fac[r]) * G[col * 2 * ps + cc];
            }
            __syncthreads();
        }
        if (sh.done) return false;
        for (int i = tid; i < p * p; i += LAD_BLOCK) W[(i / p) * ps + (i % p)] = G[(i / p) * 2 * ps + p + (i % p)];
        __syncthreads();
        return true;
    }
    // final vertex with the UNPERTURBED right-hand sides, clipped to the box; status and iterations
    __device__ __forceinline__ void final_vertex(const int it, const int max_it) {
        __syncthreads();
        for (int j = tid; j < p; j += LAD_BLOCK) {
            int ty = q_type[j];
            q_c[j] = ty == C_UB ? q_ub[q_jk[j]] : ty == C_PAT ? ra.a[q_i0[j]] : 0.0;
        }
        __syncthreads();
        for (int j = tid; j < p; j += LAD_BLOCK) {
            double v = 0.0;
            for (int i = 0; i < p; ++i) v += W[j * ps + i] * q_c[i];
            if (v < 0.0) v = 0.0;
            if (v > q_ub[j]) v = q_ub[j];
            A.x_out[c0() + j] = v;
        }
        if (tid == 0) {
            A.status[s] = (it >= max_it) ? 1 : sh.status;
            A.iters[s] = it;
        }
    }
};

// One solve of species s: columns [0, p), patterns [k0, k1).  The driver reads as the algorithm; every phase is a member of the view.  All control flow
// here is block-uniform: the flags the phases return are read from LDS after a barrier or come out of block-wide exchanges.
template <int PS, bool USEL, int NW, class SH>
__device__ __forceinline__ void lad_solve_body(const LadArgs &A, LadLds<PS, NW, SH> &m, const int s, const int p, const uint32_t k0, const uint32_t k1) {
    LadView<PS, USEL, NW, SH> v(A, m, s, p, k0, k1);
    LadShared<PS> &sh = m.sh;
    constexpr double tol = LadView<PS, USEL, NW, SH>::tol;
    v.load_tables_and_row_index();
    __syncthreads();
    v.perturb_patterns();
    v.start_basis();
    if constexpr (NW != 1) v.check_wide_masks();
    const int max_it = 200 * p + 2000;
    int it = 0;
    const bool skip = NW != 1 && sh.done;   // (block-uniform: written before the barrier above)
    v.tick_start();
    for (; it < max_it && !skip; ++it) {
        v.vertex();
        v.pattern_pass();
        LAD_TICK(v, 0);
        if (!v.choose_leaving()) break;
        const int best = sh.best; const double bdir = (double)sh.bdir;
        v.direction_and_ratio_test(best, bdir);
        LAD_TICK(v, 1);
        LadSearch ls(v.search_setup(best, bdir), USEL);
        const double tmax = sh.tmax;
        LAD_TICK(v, 2);
        if (ls.S0 >= -tol) v.degenerate_entry();
        else if (v.bracket(ls, tmax)) {
            LAD_TICK(v, 3);
            if (v.COOP && USEL) v.wide_rounds(ls);
            LAD_TICK(v, 4);
            // After finished wide rounds the walk starts at once (few tie groups are left); should it not close within
            // a few dozen groups, the binary rounds narrow further and the walk runs again without a cap.
            for (int attempt = 0; attempt < 2; ++attempt) {
                const bool quick = attempt == 0 && ls.wide_done;
                v.binary_rounds(ls, quick);
                LAD_TICK(v, 5);
                if (v.walk(ls, quick) || !quick) break;
            }
        }
        LAD_TICK(v, 6);
        if (sh.done) break;
        if (sh.ent_type < 0) { v.fail(6); break; }
        // ---- pivot: constraint `best` leaves, the entering one takes its slot; W = N^-1 by Gauss-Jordan
        v.swap_basis(best);
        // One row of N changed: W = N^-1 follows by a rank-one (Sherman-Morrison) update, O(p^2) instead of the O(p^3)
        // elimination with its 4 barriers per column -- 110 of 200 us per pivot at p = 36.  With y = n_new^T W and
        // z = y - e_best:  W' = W - (W e_best) z^T / y[best].  The inverse is rebuilt from scratch every 16th pivot and
        // whenever y[best] is small, so rounding cannot accumulate; up to 8 columns the elimination is cheap and stays.
        // W in global memory (more than 64 columns): the O(p^3) rebuild by one workgroup costs 40 ms at 256 columns, 5 s at 1100 -- a
        // hundred pivots' worth.  There the inverse is VERIFIED every 64th pivot instead (one probe vector: |N (W v) - v|, O(p^2) like
        // a pivot) and rebuilt only if the probe fails, every 1024th pivot, or -- as everywhere -- when the update's divisor is small.
        const int rebuild_mask = NW == 1 ? 15 : 1023;
        bool refactor = p <= 8 || (it & rebuild_mask) == rebuild_mask;
        if (!refactor) refactor = v.rank_one_update(best);
        if constexpr (NW != 1) {
            if (!refactor && (it & 63) == 63) refactor = v.inverse_probe_fails();   // (block-uniform)
        }
        if (refactor && !v.rebuild_inverse()) break;
        LAD_TICK(v, 7);
    }
    v.final_vertex(it, max_it);
}

}  // namespace ptx
