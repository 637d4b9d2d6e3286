// api_strain.cpp -- a9..a14: first_filter_paths (profile.rs:1080-1227), the two LP solves,
// second_filter_paths (:1229-1285), abundace_constraint (:3028-3070), and the solver seam
// pantax_hip_pao_solve (X_opt signature, profile.rs:2690-2698).
//
// The whole strain step is enqueued on the ctx stream without waiting for the host: the two filter
// decisions are taken by small device kernels (stage_hap_stats.hip, second_filter.hpp), row / pattern counts stay on the
// device, and ONE download + synchronisation at the end brings back the raw per-haplotype and
// per-species results.  The host then only redoes the reporting arithmetic (rounded fractions,
// divergence, abundance constraint) on those values, using the decisions the device took.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <memory>
#include "hap_pairs_plan.hpp"
#include "lad.hpp"
#include "primitives.hpp"

using namespace ptx;

namespace {

inline double round2(double x) { return std::round(x * 100.0) / 100.0; }   // f64::round: half away from zero

// Every small per-species / per-haplotype result of the step lives in ONE device arena (db->d_arena):
// it is zeroed with one memset before the step and fetched with one copy after it.  The DevBufs that the
// kernels write through are non-owning views into it.
struct StrainRaw {   // host pointers into db->h_arena after fetch
    const uint32_t *nnz, *nvalid, *nzcnt, *sp_pat_off, *counts;
    const double *meanf, *amax, *nzsum, *x1, *x2, *obj1, *obj2;
    const int32_t *hap_bit, *sp_p, *st1, *st2, *it1, *it2;
    const uint8_t *fixed2, *need2;
    const unsigned long long *ratio;
};

struct ArenaLayout {
    size_t amax, nzsum, obj1, obj2, x1, x2, ratio, meanf, nvalid, nzcnt, sp_p, sp_pat_off, st1, st2, it1, it2, counts, nnz, hap_bit, fixed2, need2, total;
    ArenaLayout(uint32_t S, uint64_t H) {
        size_t off = 0;
        auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 15) & ~size_t(15); return o; };
        const size_t Hn = H ? H : 1;
        amax = take(8 * S); nzsum = take(8 * S); obj1 = take(8 * S); obj2 = take(8 * S);
        x1 = take(8 * Hn); x2 = take(8 * Hn); ratio = take(8 * Hn * 2);   // per column; column k of species s lives at hap_off[s] + k
        meanf = take(8 * Hn);
        nvalid = take(4 * S); nzcnt = take(4 * S); sp_p = take(4 * S); sp_pat_off = take(4 * ((size_t)S + 1));
        st1 = take(4 * S); st2 = take(4 * S); it1 = take(4 * S); it2 = take(4 * S); counts = take(16);
        nnz = take(4 * Hn); hap_bit = take(4 * Hn);
        fixed2 = take(Hn); need2 = take(S);
        total = off;
    }
};

int bind_arena(Ctx *ctx, Db *db, LadBatch &lb, const ArenaLayout &L, bool zeroed) {
    const uint32_t S = db->S;
    const size_t Hn = db->H ? db->H : 1;
    PTX_HIP(ctx, db->d_arena.alloc(L.total));
    uint8_t *b = db->d_arena.p;
    if (!zeroed) PTX_HIP(ctx, hipMemsetAsync(b, 0, L.total, ctx->stream));   // unsolved species read back as x = 0, status 0, 0 pivots
    lb.d_amax.view(b + L.amax, S); lb.d_nzsum.view(b + L.nzsum, S); lb.d_obj.view(b + L.obj1, S); lb.d_obj2.view(b + L.obj2, S);
    lb.d_x.view(b + L.x1, Hn); lb.d_x2.view(b + L.x2, Hn);
    lb.d_ratio.view(b + L.ratio, Hn * 2);
    db->d_hap_mean.view(b + L.meanf, Hn);
    lb.d_nvalid.view(b + L.nvalid, S); lb.d_nzcnt.view(b + L.nzcnt, S); lb.d_p.view(b + L.sp_p, S); lb.d_sp_pat_off.view(b + L.sp_pat_off, (size_t)S + 1);
    lb.d_status.view(b + L.st1, S); lb.d_status2.view(b + L.st2, S); lb.d_iters.view(b + L.it1, S); lb.d_iters2.view(b + L.it2, S);
    lb.d_counts.view(b + L.counts, 4);
    db->d_hap_nnz.view(b + L.nnz, Hn); lb.d_hap_bit.view(b + L.hap_bit, Hn);
    lb.d_fixed2.view(b + L.fixed2, Hn); lb.d_need2.view(b + L.need2, S);
    return 0;
}

int fetch_arena_enqueue(Ctx *ctx, Db *db, const ArenaLayout &L, int slot) {
    for (int k = 0; k < 2; ++k) {   // both slots at once: the first step that runs AHEAD of another one must not pay for page-locking memory
        PTX_HIP(ctx, db->h_arena[k].reserve(L.total));
        if (!db->ev_step[k]) PTX_HIP(ctx, hipEventCreateWithFlags(&db->ev_step[k], hipEventDisableTiming));
    }
    PTX_HIP(ctx, hipMemcpyAsync(db->h_arena[slot].p, db->d_arena.p, L.total, hipMemcpyDeviceToHost, ctx->stream));   // the one host round trip of the step
    PTX_HIP(ctx, hipEventRecord(db->ev_step[slot], ctx->stream));   // a later step may already be enqueued behind it: the wait is for THIS step
    return 0;
}
int fetch_arena_wait(Ctx *ctx, Db *db, LadBatch &lb, const ArenaLayout &L, StrainRaw &r, int slot) {
    PTX_HIP(ctx, hipEventSynchronize(db->ev_step[slot]));
    const uint8_t *b = db->h_arena[slot].p;
    r.amax = (const double *)(b + L.amax); r.nzsum = (const double *)(b + L.nzsum); r.obj1 = (const double *)(b + L.obj1); r.obj2 = (const double *)(b + L.obj2);
    r.x1 = (const double *)(b + L.x1); r.x2 = (const double *)(b + L.x2); r.ratio = (const unsigned long long *)(b + L.ratio);
    r.meanf = (const double *)(b + L.meanf);
    r.nvalid = (const uint32_t *)(b + L.nvalid); r.nzcnt = (const uint32_t *)(b + L.nzcnt); r.sp_p = (const int32_t *)(b + L.sp_p);
    r.sp_pat_off = (const uint32_t *)(b + L.sp_pat_off);
    r.st1 = (const int32_t *)(b + L.st1); r.st2 = (const int32_t *)(b + L.st2); r.it1 = (const int32_t *)(b + L.it1); r.it2 = (const int32_t *)(b + L.it2);
    r.counts = (const uint32_t *)(b + L.counts);
    r.nnz = (const uint32_t *)(b + L.nnz); r.hap_bit = (const int32_t *)(b + L.hap_bit);
    r.fixed2 = b + L.fixed2; r.need2 = b + L.need2;
    if (r.counts[3]) return fail(ctx, PANTAX_HIP_E_STATE, "strain step: %u problems in the kernels that built the unique-trio index this step read (visit groups out of order, "
                                                           "or group offsets that are not this visit table's)", r.counts[3]);
    if (r.counts[2]) return fail(ctx, PANTAX_HIP_E_LIMIT, "strain step: more than %u membership patterns (internal: the pattern tables hold one entry per node)", lb.k_cap);
    return 0;
}

}  // namespace

namespace ptx {

// The two zero-fills of the strain step (result arena, membership masks) issued ahead of time: in the resident step the
// main stream idles before the coverage kernel while the trio index is built on the side stream, so they cost nothing
// there instead of ~10 us between coverage and the first strain kernel.  *zeroed goes to strain_enqueue of the same call, and nowhere else.
int strain_prezero(Ctx *ctx, Db *db, bool *zeroed) {
    LadBatch &lb = db->lad;
    const ArenaLayout L(db->S, db->H);
    *zeroed = false;
    PTX_TRY(bind_arena(ctx, db, lb, L, false));
    PTX_HIP(ctx, lb.d_mask.alloc(db->V));
    if (!use_node_haps(ctx, db)) PTX_TRY(zero_fill(ctx, lb.d_mask.p, db->V * sizeof(uint64_t)));   // (the by-node mask kernel writes every word)
    *zeroed = true;
    return 0;
}

// Enqueues the whole strain step and the download of its result arena; nothing waits for the host.
// d_active: device [S] or null.
int strain_enqueue(Ctx *ctx, Db *db, const pantax_hip_strain_config *cfg, const uint8_t *d_active, int slot, bool zeroed) {
    if (!db->cov.strain_may_run()) return fail(ctx, PANTAX_HIP_E_STATE, "strain_profile: call pantax_hip_node_coverage first");
    if (!db->trio.built()) return fail(ctx, PANTAX_HIP_E_STATE, "strain_profile: call pantax_hip_trio_index first");
    if (cfg->sample_nodes < 0) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_profile: sample_nodes %d", cfg->sample_nodes);
    if (cfg->solver_semantics != PANTAX_HIP_SEMANTICS_GUROBI && cfg->solver_semantics != PANTAX_HIP_SEMANTICS_HIGHS)
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_profile: solver_semantics %d", cfg->solver_semantics);
    const uint32_t S = db->S;
    LadBatch &lb = db->lad;
    const ArenaLayout L(S, db->H);
    const auto t_begin = std::chrono::steady_clock::now();
    double marks[10] = {0}; int n_marks = 0;
    auto mark = [&]() { if (n_marks < 10) marks[n_marks++] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    struct SlowReport { double *m; int *n; bool on; ~SlowReport() {
        if (*n && m[*n - 1] > 2.0 && on) {
            std::fprintf(stderr, "[strain_enqueue] slow call, ms at marks (bind, hap stats, node stats, sample, first filter, lad prepare, lad pair, fetch):");
            for (int i = 0; i < *n; ++i) std::fprintf(stderr, " %.2f", m[i]);
            std::fprintf(stderr, "\n");
        } } } slow_report{marks, &n_marks, ctx->cfg.trace};
    PTX_TRY(bind_arena(ctx, db, lb, L, zeroed));
    // the error word of the index build this step reads (a REBUILD does not wait for the host: its kernels' complaints -- a visit group out of order,
    // group offsets that are not this table's -- come back with the step's results); taken here, before the next step's rebuild may clear it
    if (db->trio_scratch.d_tot.p)
        PTX_HIP(ctx, hipMemcpyAsync(lb.d_counts.p + 3, db->trio_scratch.d_tot.p + 2, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    mark();
    // the resident step (the coverage pass left its counts to node_stats_launch): this call's two statistics passes are the only readers of the coverage
    // arena, once.  How it gets back to zero for the next step's coverage pass is cov_clean_plan's (cov_state.hpp): they zero what they read, a fill goes
    // onto the side stream in front of the LPs (below), or the next pass fills in front of itself.  A stage caller may read bases / trio_bases again, so
    // nothing is cleaned for it.
    const bool resident = db->cov.count_pending();
    const bool clocked = ctx->timing && ctx->timing_filter.empty();     // (named launches only: the fill overlaps, unbracketed)
    const CovClean clean = cov_clean_plan(resident, ctx->cfg.cov_readers_clean, ctx->cfg.cov_clean_async, clocked, db->cov.arena_bytes(), db->U);
    const bool readers_clean = clean == CovClean::readers_clean;
    struct CleanGuard { Db *d; bool armed; ~CleanGuard() { if (armed) d->cov.invalidated(); } } clean_guard{db, readers_clean};   // (a failure among the cleaning readers: neither a result nor zero)
    // the species flags the coverage pass of THIS step masked its reads with: the two statistics passes skip what it skipped
    const uint8_t *skip_absent = resident ? d_active : nullptr;
    PTX_TRY(hap_trio_stats_launch(ctx, db, db->d_hap_nnz, db->d_hap_mean, skip_absent, readers_clean));                 // a9 statistics
    mark();
    // ONE pass over the nodes where the step is eligible (node_rows_kernel, inside lad_prepare's row sort): the first filter reads the unique-trio statistics
    // alone, so the LP columns are known before any node is looked at, and the statistics below are first needed by lad_pair_launch
    const bool fused = node_pass_fused_eligible(ctx, db, cfg, readers_clean);
    const FusedNodePass fused_pass{(double)cfg->min_depth, ctx->cfg.no_absent_skip ? nullptr : skip_absent};
    if (fused) lb.S = S;
    else
    PTX_TRY(node_stats_launch(ctx, db, &lb, cfg->min_depth, skip_absent, readers_clean));                              // abundances + per-species stats
    db->node_cov_enq[slot] = fused ? Db::NodeCov::fused : resident ? Db::NodeCov::split : Db::NodeCov::replaced;   // (a stage caller's d_cov is count_launch's)
    if (readers_clean) { db->cov.readers_cleaned(); clean_guard.armed = false; }   // (the arena no longer holds a coverage result)
    mark();
    PTX_TRY(row_sample_apply(ctx, db, &lb, cfg->sample_nodes));
    mark();                             // a11 (no-op unless a species is larger than --sample)
    const FilterCfg fc{cfg->unique_trio_nodes_fraction, cfg->unique_trio_nodes_mean_count_f, cfg->single_cov_ratio, cfg->shift};
    PTX_TRY(first_filter_launch(ctx, db, &lb, d_active, fc));                               // a9 decision -> LP columns
    // nothing below reads the unique-trio tables: the NEXT step may rebuild them from here on, beside this step's row
    // sort and LPs (api_step.cpp)
    if (!db->ev_trio_free) PTX_HIP(ctx, hipEventCreateWithFlags(&db->ev_trio_free, hipEventDisableTiming));
    // ... by default from behind the ROW COMPACTION (lad_prepare records the event there): the compaction is a chained scan whose tiles
    // spin on their predecessors, and beside the rebuild's kernels its 3 ms stretched to 9-13 (round 4); PANTAX_TRIO_FREE=filter: from here
    const bool free_at_filter = ctx->cfg.trio_free_at_filter;
    if (free_at_filter) { PTX_HIP(ctx, hipEventRecord(db->ev_trio_free, ctx->stream)); db->trio.free_event_recorded(); }
    else db->trio.free_event_awaited();
    mark();
    int pmax_bound = 1;                                                                     // mask bits of a row key: min(#haps, 64) (wide species: a 64-bit hash)
    for (uint32_t s = 0; s < S; ++s) pmax_bound = std::max<int>(pmax_bound, (int)std::min<uint64_t>(db->h_hap_off[s + 1] - db->h_hap_off[s], LAD_MAXP));
    LadRows rows;
    {
        const LadRequest rq{/*cand_on_device=*/true, pmax_bound, zeroed, fused ? &fused_pass : nullptr};
        const int rc_prep = lad_prepare(ctx, db, &lb, rq, &rows);                           // a10 + row grouping
        if (rc_prep != 0) {   // failed before it recorded the event: no stale event may order the next step's rebuild (it falls back to ev_seq)
            db->trio.free_event_void();
            return rc_prep;
        }
    }
    if (db->trio.free_event_pending()) { PTX_HIP(ctx, hipEventRecord(db->ev_trio_free, ctx->stream)); db->trio.free_event_recorded(); }
    mark();
    if (clean == CovClean::side_fill) PTX_TRY(coverage_arena_clean_async(ctx, db));   // beside the LPs: one workgroup per species, most of the memory system idle
    PTX_TRY(lad_pair_launch(ctx, db, &lb, rows, pmax_bound, fc));                           // LP 1 -> a13 decision -> LP 2, objectives
    mark();
    PTX_TRY(fetch_arena_enqueue(ctx, db, L, slot));
    mark();
    return 0;
}

// Waits for the step (the one host round trip) and does the reporting arithmetic.  species_active /
// species_coverage: host [S] (may be null), read only after the wait -- a resident step fills them from the
// device's own species decisions through `after_wait`.
int strain_finish(Ctx *ctx, Db *db, const pantax_hip_strain_config *cfg, const uint8_t *species_active, const double *species_coverage,
                  pantax_hip_hap_metrics *met, pantax_hip_solve_info *info_out, void (*after_wait)(void *), void *after_wait_arg, int slot) {
    const uint32_t S = db->S;
    const uint64_t H = db->H;
    std::memset(met, 0, sizeof(pantax_hip_hap_metrics) * H);
    std::vector<pantax_hip_solve_info> info(S);
    std::memset(info.data(), 0, sizeof(pantax_hip_solve_info) * S);
    for (auto &i : info) i.obj1 = i.obj2 = NAN;
    LadBatch &lb = db->lad;
    const ArenaLayout L(S, H);
    StrainRaw r;
    PTX_TRY(fetch_arena_wait(ctx, db, lb, L, r, slot));                                         // the one host round trip
    if (after_wait) after_wait(after_wait_arg);
    db->stats_slot = slot;
    db->node_cov = db->node_cov_enq[slot];
    lb.n_rows = r.counts[0]; lb.K = r.counts[1];
    lb.h_sp_pat_off.assign(r.sp_pat_off, r.sp_pat_off + S + 1);

    // ---- reporting (host): metrics of every haplotype from the raw values and the device's decisions
    for (uint32_t s = 0; s < S; ++s) {
        if (species_active && !species_active[s]) continue;
        const uint64_t h0 = db->h_hap_off[s], h1 = db->h_hap_off[s + 1];
        const uint32_t Hs = (uint32_t)(h1 - h0);
        if (Hs == 0) continue;
        const uint64_t Us = db->h_hap_trio_off[h1] - db->h_hap_trio_off[h0];
        const bool trio_mode = Hs != 1 && Us != 0;                                          // profile.rs:1098
        const bool single_mode = !trio_mode && (Hs == 1 || db->h_all_same[s]);              // :1191-1205, :1211-1224
        const int p = r.sp_p[s];
        info[s].n_candidates = p < 0 ? -p : p;
        bool failed = false; int fail_code = 0;
        if (p < 0) { failed = true; fail_code = PANTAX_HIP_E_LIMIT; }                        // (not produced any more: the first filter keeps any number of columns)
        std::vector<uint64_t> cand(p > 0 ? p : 0);                                          // column k -> global hap
        for (uint64_t h = h0; h < h1; ++h) if (r.hap_bit[h] >= 0 && r.hap_bit[h] < p) cand[r.hap_bit[h]] = h;
        // first-filter metrics (set for every haplotype that was looked at, candidate or not)
        if (trio_mode) {
            for (uint64_t h = h0; h < h1; ++h) {
                const uint64_t nt = db->h_hap_trio_off[h + 1] - db->h_hap_trio_off[h];
                if (nt == 0) continue;                                                      // :1119
                met[h].unique_trio_nodes_fraction = round2((double)r.nnz[h] / (double)nt); met[h].has |= PANTAX_HIP_HAS_FRACTION;   // :1136-1138
                if (r.hap_bit[h] >= 0) { met[h].frequencies_mean = r.meanf[h]; met[h].has |= PANTAX_HIP_HAS_FREQ_MEAN; }            // :1165 / :1180
            }
        } else if (single_mode) {
            const double fm = r.nzcnt[s] ? r.nzsum[s] / (double)r.nzcnt[s] : 0.0;
            met[h0].frequencies_mean = round2(fm); met[h0].has |= PANTAX_HIP_HAS_FREQ_MEAN;  // :1203-1204, :1222-1223
        }
        if (p > 0) {
            info[s].status1 = r.st1[s]; info[s].iters1 = r.it1[s]; info[s].obj1 = r.obj1[s];
            info[s].n_rows = r.nvalid[s];
            info[s].n_patterns = r.sp_pat_off[s + 1] - r.sp_pat_off[s];
            if (r.st1[s] != 0) { failed = true; fail_code = PANTAX_HIP_E_SOLVER; }           // profile.rs:2999-3003
        }
        if (p > 0 && !failed) {
            for (int k = 0; k < p; ++k) {
                pantax_hip_hap_metrics &m = met[cand[k]];
                // f32 ratio of exact integer sums (profile.rs:1344-1361 accumulates in f32; identical while sums < 2^24)
                const float cov = (float)r.ratio[(h0 + k) * 2], len = (float)r.ratio[(h0 + k) * 2 + 1];
                m.path_cov_ratio = (double)(cov / len); m.has |= PANTAX_HIP_HAS_RATIO;
                m.first_sol = r.x1[h0 + k]; m.has |= PANTAX_HIP_HAS_FIRST;
            }
            if (trio_mode) {                                                                // second_filter_paths, :1234-1268
                const bool rs = r.need2[s] != 0;                                            // LP 2 actually differed from LP 1
                // highs_opt keeps the first K columns of the second solution, K = number of survivors, and zips them with the candidates
                // (profile.rs:2865-2879): a survivor at position >= K gets no second_sol.  Gurobi & co: every survivor its own x (:1500-1508)
                int n_keep = 0;
                for (int k = 0; k < p; ++k) n_keep += r.fixed2[h0 + k] ? 0 : 1;
                const int k_lim = cfg->solver_semantics == PANTAX_HIP_SEMANTICS_HIGHS ? n_keep : p;
                info[s].status2 = rs ? r.st2[s] : r.st1[s]; info[s].iters2 = rs ? r.it2[s] : 0; info[s].obj2 = rs ? r.obj2[s] : r.obj1[s];
                if (info[s].status2 != 0) { failed = true; fail_code = PANTAX_HIP_E_SOLVER; }
                for (int k = 0; k < p && !failed; ++k) {
                    pantax_hip_hap_metrics &m = met[cand[k]];
                    const double fm = (m.has & PANTAX_HIP_HAS_FREQ_MEAN) ? m.frequencies_mean : 0.0;
                    const bool keep = !r.fixed2[h0 + k];
                    if (fm != 0.0) {                                                        // :1238
                        const double sol = m.first_sol;
                        const double f = round2(std::fabs(sol - fm) / (sol + fm));
                        m.divergence = f; m.has |= PANTAX_HIP_HAS_DIVERGENCE;
                        if (keep && f > cfg->unique_trio_nodes_mean_count_f) { m.is_rescue = 1; m.has |= PANTAX_HIP_HAS_RESCUE; }   // :1251-1259
                    }
                    if (keep && k < k_lim) { m.second_sol = rs ? r.x2[h0 + k] : r.x1[h0 + k]; m.has |= PANTAX_HIP_HAS_SECOND; }   // :1500-1508 / :2871-2879
                }
            } else if (single_mode) {                                                       // :1269-1278
                pantax_hip_hap_metrics &m = met[h0];
                const double fm = m.frequencies_mean;
                if (fm > 0.0) {
                    const double sol = m.first_sol;
                    m.divergence = round2(std::fabs(sol - fm) / (sol + fm)); m.has |= PANTAX_HIP_HAS_DIVERGENCE;
                    m.second_sol = sol; m.has |= PANTAX_HIP_HAS_SECOND;
                }
            } else {                                                                        // :1279-1283
                for (int k = 0; k < p; ++k) { pantax_hip_hap_metrics &m = met[cand[k]]; m.second_sol = m.first_sol; m.has |= PANTAX_HIP_HAS_SECOND; }
            }
        }
        // ---- failed species are dropped whole (reference returns None); abundace_constraint for the rest
        if (failed) {
            for (uint64_t h = h0; h < h1; ++h) std::memset(&met[h], 0, sizeof(met[h]));
            info[s].status1 = info[s].status1 ? info[s].status1 : fail_code;
            continue;
        }
        if (!species_coverage) continue;
        const double sc = species_coverage[s];                     // profile.rs:3044-3047
        double sum = 0.0, mx = -INFINITY;
        for (uint64_t h = h0; h < h1; ++h) {
            pantax_hip_hap_metrics &m = met[h];
            if ((m.has & PANTAX_HIP_HAS_RESCUE) && m.is_rescue && (m.has & PANTAX_HIP_HAS_FIRST) && (m.has & PANTAX_HIP_HAS_SECOND))
                m.second_sol = std::min(m.first_sol, m.second_sol);   // :3031-3035
            double v = (m.has & PANTAX_HIP_HAS_SECOND) ? m.second_sol : 0.0;
            sum += v; mx = std::max(mx, v);
        }
        double diff = std::fabs(sum - sc) / ((sum + sc) / 2.0);     // :3050
        for (uint64_t h = h0; h < h1; ++h) { met[h].total_cov_diff = diff; met[h].has |= PANTAX_HIP_HAS_TOTAL_DIFF; }
        if (mx > 1.05 * sc) {                                       // :3055-3066
            double f = sc / sum;
            for (uint64_t h = h0; h < h1; ++h) {
                pantax_hip_hap_metrics &m = met[h];
                if (!((m.has & PANTAX_HIP_HAS_RESCUE) && m.is_rescue) && (m.has & PANTAX_HIP_HAS_SECOND)) m.second_sol *= f;
            }
        }
    }
    if (info_out) std::memcpy(info_out, info.data(), sizeof(pantax_hip_solve_info) * S);
    return 0;
}

}  // namespace ptx

extern "C" {

int pantax_hip_strain_profile(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_strain_config *cfg, const uint8_t *species_active,
                              const double *species_coverage, pantax_hip_hap_metrics *met, pantax_hip_solve_info *info_out) {
    if (!ctx || !db || !cfg || !met) return PANTAX_HIP_E_INVALID;
    PTX_ENTER(ctx);
    const uint8_t *d_active = nullptr;
    if (species_active) { PTX_TRY(upload_small(ctx, db->d_active, species_active, db->S)); d_active = db->d_active.p; }
    if (db->step_inflight) return fail(ctx, PANTAX_HIP_E_STATE, "strain_profile: %d enqueued step(s) of this db have not been collected", db->step_inflight);
    PTX_TRY(strain_enqueue(ctx, db, cfg, d_active, 0));
    return strain_finish(ctx, db, cfg, species_active, species_coverage, met, info_out, nullptr, nullptr, 0);
}

int pantax_hip_strain_node_stats(pantax_hip_ctx *ctx, pantax_hip_db *db, double *amax_out, uint32_t *nvalid_out, double *nzsum_out, uint32_t *nzcnt_out) {
    if (!ctx || !db) return PANTAX_HIP_E_INVALID;
    PTX_ENTER(ctx);
    if (db->stats_slot < 0 || db->h_arena[db->stats_slot].p == nullptr) return fail(ctx, PANTAX_HIP_E_STATE, "strain_node_stats: no strain step of this db has been collected");
    if (db->step_inflight) return fail(ctx, PANTAX_HIP_E_STATE, "strain_node_stats: %d enqueued step(s) of this db have not been collected (their download may reuse the slot)", db->step_inflight);
    const ArenaLayout L(db->S, db->H);
    const uint8_t *b = db->h_arena[db->stats_slot].p;   // (nothing in flight: no download is writing either slot)
    if (amax_out) std::memcpy(amax_out, b + L.amax, sizeof(double) * db->S);
    if (nvalid_out) std::memcpy(nvalid_out, b + L.nvalid, sizeof(uint32_t) * db->S);
    if (nzsum_out) std::memcpy(nzsum_out, b + L.nzsum, sizeof(double) * db->S);
    if (nzcnt_out) std::memcpy(nzcnt_out, b + L.nzcnt, sizeof(uint32_t) * db->S);
    return 0;
}

int pantax_hip_strain_hap_stats(pantax_hip_ctx *ctx, pantax_hip_db *db, uint32_t *nnz_out, double *mean_filtered_out) {
    if (!ctx || !db) return PANTAX_HIP_E_INVALID;
    PTX_ENTER(ctx);
    if (db->stats_slot < 0 || db->h_arena[db->stats_slot].p == nullptr) return fail(ctx, PANTAX_HIP_E_STATE, "strain_hap_stats: no strain step of this db has been collected");
    if (db->step_inflight) return fail(ctx, PANTAX_HIP_E_STATE, "strain_hap_stats: %d enqueued step(s) of this db have not been collected (their download may reuse the slot)", db->step_inflight);
    const ArenaLayout L(db->S, db->H);
    const uint8_t *b = db->h_arena[db->stats_slot].p;   // (nothing in flight: no download is writing either slot)
    if (nnz_out) std::memcpy(nnz_out, b + L.nnz, sizeof(uint32_t) * db->H);
    if (mean_filtered_out) std::memcpy(mean_filtered_out, b + L.meanf, sizeof(double) * db->H);
    return 0;
}

int pantax_hip_strain_node_cov(pantax_hip_ctx *ctx, pantax_hip_db *db, uint32_t *cov_out, double *ab_out) {
    if (!ctx || !db) return PANTAX_HIP_E_INVALID;
    PTX_ENTER(ctx);
    if (db->stats_slot < 0 || db->node_cov == Db::NodeCov::none) return fail(ctx, PANTAX_HIP_E_STATE, "strain_node_cov: no strain step of this db has been collected");
    if (db->step_inflight) return fail(ctx, PANTAX_HIP_E_STATE, "strain_node_cov: %d enqueued step(s) of this db have not been collected (their node pass rewrites the arrays)", db->step_inflight);
    if (db->node_cov == Db::NodeCov::fused) return fail(ctx, PANTAX_HIP_E_STATE, "strain_node_cov: the step collected last took the fused node pass, which stores neither array (option node_pass=split)");
    if (db->node_cov == Db::NodeCov::replaced) return fail(ctx, PANTAX_HIP_E_STATE, "strain_node_cov: a stage call has counted the covered bases since (pantax_hip_node_coverage returns them)");
    if (db->d_cov.n < db->V || db->lad.d_ab.n < db->V) return fail(ctx, PANTAX_HIP_E_STATE, "strain_node_cov: the per-node arrays of the step are gone");
    if (cov_out) PTX_TRY(download(ctx, cov_out, db->d_cov.p, db->V));
    if (ab_out) PTX_TRY(download(ctx, ab_out, db->lad.d_ab.p, db->V));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int pantax_hip_pao_solve_batch(pantax_hip_ctx *ctx, const pantax_hip_species_batch *in, const pantax_hip_solution_batch *out) {
    if (!ctx || !in || !out || !in->node_off || !in->node_len || !in->node_abundance || !in->hap_off || !in->path_off || !in->path_nodes ||
        !in->cand_off || !in->cand_path_idx || !out->x || !out->status)
        return PANTAX_HIP_E_INVALID;
    const uint32_t S = in->n_species;
    if (S == 0) return fail(ctx, PANTAX_HIP_E_INVALID, "pao_solve_batch: n_species == 0");
    PTX_ENTER(ctx);
    const uint64_t V = in->node_off[S], H = in->hap_off[S];
    // a resident DB around the caller's graphs: species s takes the node ids node_off[s]+1 .. node_off[s+1]
    std::vector<int64_t> rs(S), re(S);
    for (uint32_t s = 0; s < S; ++s) {
        if (in->node_off[s + 1] <= in->node_off[s]) return fail(ctx, PANTAX_HIP_E_INVALID, "pao_solve_batch: species %u has no nodes", s);
        rs[s] = (int64_t)in->node_off[s] + 1; re[s] = (int64_t)in->node_off[s + 1];
    }
    pantax_hip_graphs g{S, rs.data(), re.data(), in->node_off, in->node_len, in->hap_off, in->path_off, in->path_nodes};
    pantax_hip_db *db = nullptr;
    PTX_TRY(pantax_hip_db_upload(ctx, &g, &db));
    std::unique_ptr<pantax_hip_db, void (*)(pantax_hip_db *)> guard(db, [](pantax_hip_db *d) { delete d; });
    LadBatch &lb = db->lad;
    lb.S = S;
    const ArenaLayout L(S, H);
    PTX_TRY(bind_arena(ctx, db, lb, L, false));
    std::vector<uint32_t> cov32(V ? V : 1, 0);
    if (in->node_base_cov) for (uint64_t v = 0; v < V; ++v) cov32[v] = (uint32_t)in->node_base_cov[v];
    PTX_TRY(upload(ctx, db->d_cov, cov32.data(), V));
    PTX_TRY(upload(ctx, lb.d_ab, in->node_abundance, V));
    std::vector<double> amax(S);
    std::vector<uint32_t> nvalid(S);
    lb.h_p.assign(S, 0);
    lb.h_cand.assign(H ? H : 1, 0);
    std::vector<uint8_t> fixed(H ? H : 1, 0);
    int pmax = 1;
    for (uint32_t s = 0; s < S; ++s) {
        double mx = -INFINITY; uint32_t nv = 0;
        for (uint64_t v = in->node_off[s]; v < in->node_off[s + 1]; ++v) { mx = std::max(mx, in->node_abundance[v]); if (in->node_abundance[v] > 0.0) ++nv; }
        amax[s] = mx; nvalid[s] = nv;
        const uint64_t c0 = in->cand_off[s], c1 = in->cand_off[s + 1], nh = in->hap_off[s + 1] - in->hap_off[s];
        out->status[s] = 0;
        if (c1 - c0 > nh) return fail(ctx, PANTAX_HIP_E_INVALID, "pao_solve_batch: species %u has %llu candidates for %llu paths", s, (unsigned long long)(c1 - c0), (unsigned long long)nh);
        for (uint64_t k = c0; k < c1; ++k) {
            if (in->cand_path_idx[k] >= nh) return fail(ctx, PANTAX_HIP_E_INVALID, "pao_solve_batch: species %u candidate %llu names path %u of %llu", s, (unsigned long long)(k - c0), in->cand_path_idx[k], (unsigned long long)nh);
            lb.h_cand[in->hap_off[s] + (k - c0)] = in->cand_path_idx[k];
            fixed[in->hap_off[s] + (k - c0)] = (in->fixed_zero && in->fixed_zero[k]) ? 1 : 0;
        }
        lb.h_p[s] = (int32_t)(c1 - c0);
        pmax = std::max(pmax, (int)std::min<uint64_t>(c1 - c0, LAD_MAXP));
    }
    PTX_TRY(upload(ctx, lb.d_amax, amax.data(), S));
    PTX_TRY(upload(ctx, lb.d_nvalid, nvalid.data(), S));
    LadRows rows;
    PTX_TRY(lad_prepare(ctx, db, &lb, LadRequest{/*cand_on_device=*/false, pmax, /*zeroed=*/false, /*fused=*/nullptr}, &rows));
    PTX_TRY(upload(ctx, lb.d_fixed2, fixed.data(), fixed.size()));
    PTX_TRY(lad_solve_launch(ctx, db, &lb, rows, pmax, nullptr, lb.d_fixed2.p, lb.d_x.p, lb.d_obj.p, lb.d_status.p, lb.d_iters.p));
    std::vector<double> x(H ? H : 1), obj(S);
    std::vector<unsigned long long> ratio((H ? H : 1) * 2);
    std::vector<int32_t> st(S), it(S);
    std::vector<uint32_t> counts(4);
    PTX_TRY(download(ctx, x.data(), lb.d_x.p, x.size()));
    PTX_TRY(download(ctx, obj.data(), lb.d_obj.p, S));
    PTX_TRY(download(ctx, st.data(), lb.d_status.p, S));
    PTX_TRY(download(ctx, it.data(), lb.d_iters.p, S));
    PTX_TRY(download(ctx, ratio.data(), lb.d_ratio.p, ratio.size()));
    PTX_TRY(download(ctx, counts.data(), lb.d_counts.p, 4));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (counts[2]) return fail(ctx, PANTAX_HIP_E_LIMIT, "pao_solve_batch: more membership patterns than this build sizes for");
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t c0 = in->cand_off[s];
        const int p = lb.h_p[s];
        for (int k = 0; k < p; ++k) {
            out->x[c0 + k] = x[in->hap_off[s] + k];
            if (out->path_cov_ratio) out->path_cov_ratio[c0 + k] = (float)ratio[(in->hap_off[s] + k) * 2] / (float)ratio[(in->hap_off[s] + k) * 2 + 1];
        }
        if (out->obj) out->obj[s] = (p > 0 && nvalid[s]) ? obj[s] : 0.0;
        if (out->iters) out->iters[s] = p > 0 ? it[s] : 0;
        if (p > 0 && st[s] != 0) out->status[s] = PANTAX_HIP_E_SOLVER;
    }
    return 0;
}

// one species = a batch of one (same kernels, same answers)
int pantax_hip_pao_solve(pantax_hip_ctx *ctx, uint32_t n_nodes, const int64_t *node_len, const double *node_abundance,
                         const uint64_t *node_base_cov, uint32_t n_paths, const uint64_t *path_off, const uint32_t *path_nodes,
                         uint32_t n_cand, const uint32_t *cand_path_idx, const uint8_t *fixed_zero, double *x_out,
                         float *path_cov_ratio_out, double *obj_out, int32_t *status_out) {
    if (!ctx || !node_len || !node_abundance || !path_off || !path_nodes || !cand_path_idx || !x_out) return PANTAX_HIP_E_INVALID;
    if (n_cand == 0) return fail(ctx, PANTAX_HIP_E_INVALID, "pao_solve: no candidate paths (the reference skips the solver, profile.rs:2968)");
    PTX_ENTER(ctx);
    const uint64_t node_off[2] = {0, n_nodes}, hap_off[2] = {0, n_paths}, cand_off[2] = {0, n_cand};
    const pantax_hip_species_batch in{1, node_off, node_len, node_abundance, node_base_cov, hap_off, path_off, path_nodes, cand_off, cand_path_idx, fixed_zero};
    int32_t st = 0, it = 0;
    const pantax_hip_solution_batch out{x_out, path_cov_ratio_out, obj_out, &st, &it};
    PTX_TRY(pantax_hip_pao_solve_batch(ctx, &in, &out));
    if (status_out) *status_out = st == PANTAX_HIP_E_SOLVER ? 1 : st;
    if (st != 0) return fail(ctx, PANTAX_HIP_E_SOLVER, "pao_solve: LAD solver stopped after %d pivots", it);
    return 0;
}

// the state every pass over the reads' candidate masks needs (read strains, read support, read classes, mosaic reads, read rescue): reads binned and grouped
// against this db, a db with graphs, no step in flight
static int check_read_pass_state(pantax_hip_ctx *ctx, const pantax_hip_db *db, const pantax_hip_reads *reads, const char *what) {
    if (!reads->state.binned_against(db->uid) || !reads->state.grouped())
        return fail(ctx, PANTAX_HIP_E_STATE, "%s: call pantax_hip_bin_reads on these reads against this db first", what);
    if (db->d_path_nodes.p == nullptr || db->h_path_off.size() != db->H + 1)
        return fail(ctx, PANTAX_HIP_E_STATE, "%s: the db was uploaded without graphs (ranges only)", what);
    if (db->step_inflight) return fail(ctx, PANTAX_HIP_E_STATE, "%s: %d enqueued step(s) of this db have not been collected", what, db->step_inflight);
    return 0;
}

// what the three passes over the reads' candidate masks (read strains, read support, read classes) share: the state they need, a candidate set in range and without repeats -> every species'
// candidates in ascending haplotype order (bit order = the order of the sum and of the tie rule), ord[c] = the caller's entry of sorted candidate c
static int check_read_strain_set(pantax_hip_ctx *ctx, const pantax_hip_db *db, const pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand,
                                 const char *what, std::vector<uint32_t> &hap, std::vector<double> &w, std::vector<uint64_t> &ord_all, bool need_w = true) {
    const uint32_t S = db->S;
    if (cand->n_species != S) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: the candidate set has %u species, the db %u", what, cand->n_species, S);
    PTX_TRY(check_read_pass_state(ctx, db, reads, what));
    if (cand->cand_off[0] != 0) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: cand_off[0] = %llu", what, (unsigned long long)cand->cand_off[0]);
    for (uint32_t s = 0; s < S; ++s)
        if (cand->cand_off[s + 1] < cand->cand_off[s]) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: cand_off decreases at species %u", what, s);
    const uint64_t C = cand->cand_off[S];
    if (C && (!cand->cand_hap || (need_w && !cand->cand_w))) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: null cand_hap / cand_w", what);
    hap.resize(C); w.resize(C); ord_all.resize(C);
    std::vector<uint64_t> ord;
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t c0 = cand->cand_off[s], c1 = cand->cand_off[s + 1], nh = db->h_hap_off[s + 1] - db->h_hap_off[s];
        ord.resize(c1 - c0);
        for (uint64_t c = c0; c < c1; ++c) {
            if (cand->cand_hap[c] >= nh) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: species %u has %llu haplotypes, candidate %u", what, s, (unsigned long long)nh, cand->cand_hap[c]);
            ord[c - c0] = c;
        }
        std::sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) { return cand->cand_hap[a] < cand->cand_hap[b]; });
        for (uint64_t i = 0; i < ord.size(); ++i) {
            if (i && cand->cand_hap[ord[i]] == cand->cand_hap[ord[i - 1]])
                return fail(ctx, PANTAX_HIP_E_INVALID, "%s: haplotype %u of species %u is a candidate twice", what, cand->cand_hap[ord[i]], s);
            hap[c0 + i] = cand->cand_hap[ord[i]];
            w[c0 + i] = cand->cand_w ? cand->cand_w[ord[i]] : 0.0;   // (the read classes take a set without weights)
            ord_all[c0 + i] = ord[i];
        }
    }
    return 0;
}

int pantax_hip_read_strains(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand,
                            uint32_t *hap_out, int32_t *n_out, double *post_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !reads || !cand || !cand->cand_off || (reads->R && (!hap_out || !n_out || !post_out)))
        return fail(ctx, PANTAX_HIP_E_INVALID, "read_strains: null argument");
    PTX_ENTER(ctx);
    std::vector<uint32_t> hap;
    std::vector<double> w;
    std::vector<uint64_t> ord;
    PTX_TRY(check_read_strain_set(ctx, db, reads, cand, "read_strains", hap, w, ord));
    return read_strains_launch(ctx, db, reads, cand->cand_off, hap.data(), w.data(), hap_out, n_out, post_out);
}

// the one argument check of pantax_hip_strain_read_support and pantax_hip_strain_mosaic: the set check above, then pair_off_out (always written from here
// on) and the pair_cap rule
static int check_read_pair_set(pantax_hip_ctx *ctx, const pantax_hip_db *db, const pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand, const char *what,
                               uint64_t *pair_off_out, uint64_t pair_cap, std::vector<uint32_t> &hap, std::vector<double> &w, std::vector<uint64_t> &ord) {
    PTX_TRY(check_read_strain_set(ctx, db, reads, cand, what, hap, w, ord));
    const uint32_t S = db->S;
    pair_off_out[0] = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t K = cand->cand_off[s + 1] - cand->cand_off[s];
        pair_off_out[s + 1] = pair_off_out[s] + (K <= 64 ? K * K : 0);
    }
    if (pair_off_out[S] > pair_cap)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "%s: %llu pair entries, the caller's array holds %llu", what, (unsigned long long)pair_off_out[S], (unsigned long long)pair_cap);
    return 0;
}

int pantax_hip_strain_read_support(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand,
                                   uint64_t *hap_out, uint64_t *species_out, uint64_t *pair_off_out, uint64_t pair_cap, uint64_t *pair_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !reads || !cand || !cand->cand_off || !pair_off_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_read_support: null argument");
    PTX_ENTER(ctx);
    std::vector<uint32_t> hap;
    std::vector<double> w;
    std::vector<uint64_t> ord;
    PTX_TRY(check_read_pair_set(ctx, db, reads, cand, "strain_read_support", pair_off_out, pair_cap, hap, w, ord));
    const uint32_t S = db->S;
    if ((cand->cand_off[S] && !hap_out) || (S && !species_out) || (pair_off_out[S] && !pair_out))
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_read_support: null output array");
    return read_support_launch(ctx, db, reads, cand->cand_off, hap.data(), w.data(), ord.data(), pair_off_out, hap_out, species_out, pair_out);
}

int pantax_hip_fragment_mates(pantax_hip_ctx *ctx, uint64_t n, const uint64_t *key, const uint8_t *tag, uint32_t *mate_out, uint64_t *counts_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!counts_out || (n && (!key || !tag || !mate_out))) return fail(ctx, PANTAX_HIP_E_INVALID, "fragment_mates: null argument");
    if (n >= PANTAX_HIP_MATE_AMBIGUOUS) return fail(ctx, PANTAX_HIP_E_LIMIT, "fragment_mates: %llu reads exceed the 32-bit mate indices", (unsigned long long)n);
    for (uint64_t i = 0; i < n; ++i)
        if (tag[i] > 2) return fail(ctx, PANTAX_HIP_E_INVALID, "fragment_mates: tag %u of read %llu (0, 1 or 2)", (unsigned)tag[i], (unsigned long long)i);
    PTX_ENTER(ctx);
    counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
    if (n == 0) return 0;
    return fragment_mates_launch(ctx, n, key, tag, mate_out, counts_out);
}

int pantax_hip_strain_fragments(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand, const uint32_t *mate,
                                uint64_t *hap_out, uint64_t *species_out, int32_t *status_out, uint64_t *pair_off_out, uint64_t pair_cap, uint64_t *pair_out,
                                int32_t *frag_n_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !reads || !cand || !cand->cand_off || !pair_off_out || (reads->R && !mate)) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_fragments: null argument");
    PTX_ENTER(ctx);
    std::vector<uint32_t> hap;
    std::vector<double> w;
    std::vector<uint64_t> ord;
    PTX_TRY(check_read_strain_set(ctx, db, reads, cand, "strain_fragments", hap, w, ord));
    return fragments_launch(ctx, db, reads, cand->cand_off, hap.data(), w.data(), ord.data(), mate, hap_out, species_out, status_out, pair_off_out, pair_cap, pair_out,
                            frag_n_out);
}

int pantax_hip_strain_mosaic(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand, uint64_t *species_out,
                             uint64_t *extra_out, uint64_t *hap_out, uint64_t *pair_off_out, uint64_t pair_cap, uint64_t *pair_out, uint64_t junction_cap,
                             uint32_t *junction_out, uint64_t *junction_count_out, uint64_t *n_junctions_out, uint64_t *n_breaks_total_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !reads || !cand || !cand->cand_off || !pair_off_out || !n_junctions_out || !n_breaks_total_out)
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_mosaic: null argument");
    PTX_ENTER(ctx);
    std::vector<uint32_t> hap;
    std::vector<double> w;
    std::vector<uint64_t> ord;
    PTX_TRY(check_read_pair_set(ctx, db, reads, cand, "strain_mosaic", pair_off_out, pair_cap, hap, w, ord));
    const uint32_t S = db->S;
    if ((cand->cand_off[S] && !hap_out) || (S && (!species_out || !extra_out)) || (pair_off_out[S] && !pair_out) || (junction_cap && (!junction_out || !junction_count_out)))
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_mosaic: null output array");
    return mosaic_launch(ctx, db, reads, cand->cand_off, hap.data(), w.data(), ord.data(), pair_off_out, species_out, extra_out, hap_out, pair_out, junction_cap,
                         junction_out, junction_count_out, n_junctions_out, n_breaks_total_out);
}

int pantax_hip_strain_read_em(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_em_set *cand, uint64_t *species_out,
                              uint64_t *cls_off_out, uint64_t cls_cap, uint64_t *cls_mask_out, uint64_t *cls_q_out, double *x_out, uint32_t *iter_out,
                              int32_t *converged_out, double *delta_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !reads || !cand || !cand->cand_off || !cls_off_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_read_em: null argument");
    PTX_ENTER(ctx);
    if (cand->max_iter == 0 || !(cand->tol >= 0.0) || !std::isfinite(cand->tol))
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_read_em: max_iter %u, tol %g (at least one iteration; tol finite and >= 0)", cand->max_iter, cand->tol);
    // the set of the read passes with lengths in place of the weights: the same checks, the same canonical order
    const pantax_hip_read_strain_set set{cand->n_species, cand->cand_off, cand->cand_hap, nullptr};
    std::vector<uint32_t> hap;
    std::vector<double> w;
    std::vector<uint64_t> ord;
    PTX_TRY(check_read_strain_set(ctx, db, reads, &set, "strain_read_em", hap, w, ord, /*need_w=*/false));
    const uint32_t S = db->S;
    const uint64_t C = cand->cand_off[S];
    if (C && !cand->cand_len) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_read_em: null cand_len");
    if ((C && !x_out) || (S && (!species_out || !iter_out || !converged_out || !delta_out)) || (cls_cap && (!cls_mask_out || !cls_q_out)))
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_read_em: null output array");
    std::vector<uint64_t> len(C ? C : 1);
    for (uint64_t c = 0; c < C; ++c) len[c] = cand->cand_len[ord[c]];
    return read_em_launch(ctx, db, reads, cand->cand_off, hap.data(), len.data(), ord.data(), cand->max_iter, cand->tol, species_out, cls_off_out, cls_cap, cls_mask_out,
                          cls_q_out, x_out, iter_out, converged_out, delta_out);
}

// what the two node reports behind the coverage pass share: the db's species count (checked first, as before the window of the track), a selection of
// species-local haplotypes (in range, no repeats within a species) ...
static int check_species_count(pantax_hip_ctx *ctx, const pantax_hip_db *db, const char *what, uint32_t n_species) {
    return n_species == db->S ? 0 : fail(ctx, PANTAX_HIP_E_INVALID, "%s: the selection has %u species, the db %u", what, n_species, db->S);
}
static int check_hap_selection(pantax_hip_ctx *ctx, const pantax_hip_db *db, const char *what, const uint64_t *sel_off, const uint32_t *sel_hap) {
    const uint32_t S = db->S;
    if (db->d_path_nodes.p == nullptr || db->h_path_off.size() != db->H + 1)
        return fail(ctx, PANTAX_HIP_E_STATE, "%s: the db was uploaded without graphs (ranges only)", what);
    if (sel_off[0] != 0) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: sel_off[0] = %llu", what, (unsigned long long)sel_off[0]);
    for (uint32_t s = 0; s < S; ++s)
        if (sel_off[s + 1] < sel_off[s]) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: sel_off decreases at species %u", what, s);
    if (sel_off[S] && !sel_hap) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: null sel_hap", what);
    std::vector<uint8_t> seen;
    for (uint32_t s = 0; s < S; ++s) {
        const uint64_t nh = db->h_hap_off[s + 1] - db->h_hap_off[s];
        seen.assign(nh, 0);
        for (uint64_t c = sel_off[s]; c < sel_off[s + 1]; ++c) {
            const uint32_t h = sel_hap[c];
            if (h >= nh) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: species %u has %llu haplotypes, selected %u", what, s, (unsigned long long)nh, h);
            if (seen[h]) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: haplotype %u of species %u is selected twice", what, h, s);
            seen[h] = 1;
        }
    }
    return 0;
}
// ... and what their kernels read: bases_per_node in the coverage arena, node_base_cov in d_cov -- as the STAGE call leaves them
static int check_stage_coverage(pantax_hip_ctx *ctx, const pantax_hip_db *db, const char *what) {
    if (db->step_inflight) return fail(ctx, PANTAX_HIP_E_STATE, "%s: %d enqueued step(s) of this db have not been collected", what, db->step_inflight);
    if (!db->cov.stage_report_may_run() || db->d_cov.n < db->V || (db->V && (!db->d_cov.p || !db->d_bases.p)))
        return fail(ctx, PANTAX_HIP_E_STATE, "%s: the db holds no coverage result of pantax_hip_node_coverage%s; call pantax_hip_node_coverage first", what,
                    db->cov.resident_used_it() ? " (a resident step counts the covered bases in its own passes, keeps no node_base_cov and may have zeroed the coverage arena)" : "");
    return 0;
}

int pantax_hip_strain_cov_track(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_cov_track_set *sel, uint64_t *win_off_out, uint64_t cap,
                                uint32_t *n_nodes_out, uint64_t *len_out, uint64_t *covered_out, uint64_t *bases_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off || !win_off_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_cov_track: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_cov_track", sel->n_species));
    if (sel->window == 0) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_cov_track: window of 0 bases");
    PTX_TRY(check_hap_selection(ctx, db, "strain_cov_track", sel->sel_off, sel->sel_hap));
    PTX_TRY(check_stage_coverage(ctx, db, "strain_cov_track"));
    return cov_track_launch(ctx, db, sel->sel_off, sel->sel_hap, sel->window, win_off_out, cap, n_nodes_out, len_out, covered_out, bases_out);
}

int pantax_hip_strain_growth(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_cov_track_set *sel, uint64_t *win_off_out, uint64_t cap,
                             uint32_t *n_own_out, uint64_t *len_out, uint64_t *len_own_out, uint64_t *bases_own_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off || !win_off_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_growth: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_growth", sel->n_species));
    if (sel->window == 0) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_growth: window of 0 bases");
    PTX_TRY(check_hap_selection(ctx, db, "strain_growth", sel->sel_off, sel->sel_hap));
    PTX_TRY(check_stage_coverage(ctx, db, "strain_growth"));
    return growth_launch(ctx, db, sel->sel_off, sel->sel_hap, sel->window, win_off_out, cap, n_own_out, len_out, len_own_out, bases_own_out);
}

int pantax_hip_strain_segments(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_segment_set *sel, uint64_t *seg_off_out, uint64_t cap, uint64_t *hap_len_out,
                               uint64_t *n_runs_out, uint64_t *run_len_out, uint64_t *run_max_out, uint8_t *seg_class_out, uint64_t *seg_step_out,
                               uint32_t *seg_n_steps_out, uint64_t *seg_start_out, uint64_t *seg_len_out, uint64_t *seg_bases_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off || !seg_off_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_segments: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_segments", sel->n_species));
    if (sel->min_len == 0) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_segments: min_len of 0 bases");
    PTX_TRY(check_hap_selection(ctx, db, "strain_segments", sel->sel_off, sel->sel_hap));
    const uint64_t C = sel->sel_off[db->S];
    if (C && (!sel->peak_depth || !hap_len_out || !n_runs_out || !run_len_out || !run_max_out))
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_segments: null peak_depth or summary array");
    for (uint64_t c = 0; c < C; ++c)
        if (sel->peak_depth[c] > (1ull << 31))
            return fail(ctx, PANTAX_HIP_E_INVALID, "strain_segments: peak_depth %llu of entry %llu (at most 2^31)", (unsigned long long)sel->peak_depth[c], (unsigned long long)c);
    PTX_TRY(check_stage_coverage(ctx, db, "strain_segments"));
    return segments_launch(ctx, db, sel->sel_off, sel->sel_hap, sel->peak_depth, sel->min_len, seg_off_out, cap, hap_len_out, n_runs_out, run_len_out, run_max_out,
                           seg_class_out, seg_step_out, seg_n_steps_out, seg_start_out, seg_len_out, seg_bases_out);
}

int pantax_hip_strain_evidence(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel, uint64_t *hap_out, uint64_t *species_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_evidence: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_evidence", sel->n_species));
    PTX_TRY(check_hap_selection(ctx, db, "strain_evidence", sel->sel_off, sel->sel_hap));
    if ((sel->sel_off[db->S] && !hap_out) || (db->S && !species_out)) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_evidence: null output array");
    PTX_TRY(check_stage_coverage(ctx, db, "strain_evidence"));
    return evidence_launch(ctx, db, sel->sel_off, sel->sel_hap, hap_out, species_out);
}

int pantax_hip_strain_fit(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_fit_set *sel, uint64_t *hap_out, uint64_t *species_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_fit: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_fit", sel->n_species));
    PTX_TRY(check_hap_selection(ctx, db, "strain_fit", sel->sel_off, sel->sel_hap));
    const uint64_t C = sel->sel_off[db->S];
    if (C && !sel->sel_w) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_fit: null sel_w");
    for (uint64_t c = 0; c < C; ++c)
        if (!std::isfinite(sel->sel_w[c]) || sel->sel_w[c] < 0.0) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_fit: the weight of selection entry %llu is %g (finite and >= 0)", (unsigned long long)c, sel->sel_w[c]);
    if ((C && !hap_out) || (db->S && !species_out)) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_fit: null output array");
    PTX_TRY(check_stage_coverage(ctx, db, "strain_fit"));
    return fit_launch(ctx, db, sel->sel_off, sel->sel_hap, sel->sel_w, hap_out, species_out);
}

int pantax_hip_strain_bootstrap(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_bootstrap_set *sel, double *x_out, double *obj_out, uint64_t *rows_out,
                                int32_t *status_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_bootstrap: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_bootstrap", sel->n_species));
    PTX_TRY(check_hap_selection(ctx, db, "strain_bootstrap", sel->sel_off, sel->sel_hap));
    if (db->S && !sel->sp_key) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_bootstrap: null sp_key");
    if (sel->n_replicates == 0xFFFFFFFFu) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_bootstrap: %u replicates (at most 2^32 - 2)", sel->n_replicates);
    if ((sel->sel_off[db->S] && !x_out) || (db->S && (!obj_out || !rows_out || !status_out))) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_bootstrap: null output array");
    PTX_TRY(check_stage_coverage(ctx, db, "strain_bootstrap"));
    try {
        return bootstrap_launch(ctx, db, sel->sel_off, sel->sel_hap, sel->sp_key, sel->seed, sel->n_replicates, x_out, obj_out, rows_out, status_out);
    } catch (const std::bad_alloc &) {
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_bootstrap: out of host memory");
    }
}

int pantax_hip_strain_dropout(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel, double *x_out, double *obj_out, int32_t *status_out,
                              uint64_t *rows_out, uint64_t *count_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_dropout: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_dropout", sel->n_species));
    PTX_TRY(check_hap_selection(ctx, db, "strain_dropout", sel->sel_off, sel->sel_hap));
    if ((sel->sel_off[db->S] && !x_out) || (db->S && (!obj_out || !status_out || !rows_out || !count_out))) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_dropout: null output array");
    PTX_TRY(check_stage_coverage(ctx, db, "strain_dropout"));
    try {
        return dropout_launch(ctx, db, sel->sel_off, sel->sel_hap, x_out, obj_out, status_out, rows_out, count_out);
    } catch (const std::bad_alloc &) {
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_dropout: out of host memory");
    }
}

int pantax_hip_db_hap_pairs(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel, uint64_t *pair_off_out, uint64_t pair_cap, uint64_t *pair_out,
                            uint64_t *species_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off || !pair_off_out) return fail(ctx, PANTAX_HIP_E_INVALID, "db_hap_pairs: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "db_hap_pairs", sel->n_species));
    PTX_TRY(check_hap_selection(ctx, db, "db_hap_pairs", sel->sel_off, sel->sel_hap));
    // (no state beyond the uploaded graphs: the call reads node lengths, walks and the node -> haplotype words, and writes nothing of the db's)
    const uint32_t S = db->S, wide = hap_pairs_offsets(S, sel->sel_off, pair_off_out);
    if (wide != S)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "db_hap_pairs: species %u has %llu selected haplotypes, the call serves %llu", wide, (unsigned long long)(sel->sel_off[wide + 1] - sel->sel_off[wide]),
                    (unsigned long long)HAP_PAIRS_MAX_K);
    if (pair_off_out[S] > pair_cap)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "db_hap_pairs: %llu pair entries, the caller's array holds %llu", (unsigned long long)pair_off_out[S], (unsigned long long)pair_cap);
    if (pair_off_out[S] && !pair_out) return fail(ctx, PANTAX_HIP_E_INVALID, "db_hap_pairs: null output array");
    return hap_pairs_launch(ctx, db, sel->sel_off, sel->sel_hap, pair_off_out, pair_out, species_out);
}

int pantax_hip_strain_pair_evidence(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel, uint64_t *pair_off_out, uint64_t pair_cap, uint64_t *pair_out,
                                    uint64_t *species_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off || !pair_off_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_pair_evidence: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_pair_evidence", sel->n_species));
    PTX_TRY(check_hap_selection(ctx, db, "strain_pair_evidence", sel->sel_off, sel->sel_hap));
    const uint32_t S = db->S, wide = hap_pairs_offsets(S, sel->sel_off, pair_off_out);
    PTX_TRY(check_stage_coverage(ctx, db, "strain_pair_evidence"));   // (the sizing call too: it sizes the array of a call that can run)
    if (wide != S)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_pair_evidence: species %u has %llu selected haplotypes, the call serves %llu", wide,
                    (unsigned long long)(sel->sel_off[wide + 1] - sel->sel_off[wide]), (unsigned long long)HAP_PAIRS_MAX_K);
    if (pair_off_out[S] > pair_cap)
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_pair_evidence: %llu pair entries, the caller's array holds %llu", (unsigned long long)pair_off_out[S], (unsigned long long)pair_cap);
    if (pair_off_out[S] && !pair_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_pair_evidence: null output array");
    return pair_evidence_launch(ctx, db, sel->sel_off, sel->sel_hap, pair_off_out, pair_out, species_out);
}

int pantax_hip_strain_depth(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel, uint64_t *hap_out, uint64_t *species_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_depth: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_depth", sel->n_species));
    PTX_TRY(check_hap_selection(ctx, db, "strain_depth", sel->sel_off, sel->sel_hap));
    if (sel->sel_off[db->S] && !hap_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_depth: null output array");   // (species_out may be null: no species histograms)
    PTX_TRY(check_stage_coverage(ctx, db, "strain_depth"));
    return depth_launch(ctx, db, sel->sel_off, sel->sel_hap, hap_out, species_out);
}

// the argument checks that pantax_hip_strain_near_miss and pantax_hip_strain_addin share: both sets in range and free of repeats, and disjoint
static int check_near_miss_set(pantax_hip_ctx *ctx, const pantax_hip_db *db, const char *what, const pantax_hip_near_miss_set *sel) {
    PTX_TRY(check_species_count(ctx, db, what, sel->n_species));
    PTX_TRY(check_hap_selection(ctx, db, what, sel->sel_off, sel->sel_hap));
    PTX_TRY(check_hap_selection(ctx, db, (std::string(what) + " (candidates)").c_str(), sel->cand_off, sel->cand_hap));
    std::vector<uint8_t> reported;
    for (uint32_t s = 0; s < db->S; ++s) {
        reported.assign(db->h_hap_off[s + 1] - db->h_hap_off[s], 0);
        for (uint64_t c = sel->sel_off[s]; c < sel->sel_off[s + 1]; ++c) reported[sel->sel_hap[c]] = 1;
        for (uint64_t c = sel->cand_off[s]; c < sel->cand_off[s + 1]; ++c)
            if (reported[sel->cand_hap[c]]) return fail(ctx, PANTAX_HIP_E_INVALID, "%s: haplotype %u of species %u is reported and a candidate", what, sel->cand_hap[c], s);
    }
    return 0;
}

int pantax_hip_strain_near_miss(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_near_miss_set *sel, uint64_t *cand_out, uint64_t *species_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off || !sel->cand_off) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_near_miss: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_near_miss_set(ctx, db, "strain_near_miss", sel));
    if ((sel->cand_off[db->S] && !cand_out) || (db->S && !species_out)) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_near_miss: null output array");
    PTX_TRY(check_stage_coverage(ctx, db, "strain_near_miss"));
    return near_miss_launch(ctx, db, sel->sel_off, sel->sel_hap, sel->cand_off, sel->cand_hap, cand_out, species_out);
}

int pantax_hip_strain_read_rescue(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_near_miss_set *sel, uint64_t *species_out,
                                  uint64_t *step_out, uint64_t *cand_out, uint64_t *cand_steps_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !reads || !sel || !sel->sel_off || !sel->cand_off) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_read_rescue: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_near_miss_set(ctx, db, "strain_read_rescue", sel));
    PTX_TRY(check_read_pass_state(ctx, db, reads, "strain_read_rescue"));
    if ((sel->cand_off[db->S] && (!cand_out || !cand_steps_out)) || (db->S && (!species_out || !step_out)))
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_read_rescue: null output array");
    return rescue_launch(ctx, db, reads, sel->sel_off, sel->sel_hap, sel->cand_off, sel->cand_hap, species_out, step_out, cand_out, cand_steps_out);
}

int pantax_hip_strain_links(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *sel, uint64_t *species_out,
                            uint64_t *link_out, uint64_t *hap_out, uint64_t *brk_off_out, uint64_t cap, uint64_t *brk_step_out, uint64_t *brk_start_out,
                            uint32_t *brk_node_a_out, uint32_t *brk_node_b_out, uint64_t *brk_flank_out, uint64_t *brk_mask_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !reads || !sel || !sel->cand_off || !brk_off_out) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_links: null argument");
    PTX_ENTER(ctx);
    std::vector<uint32_t> hap;
    std::vector<double> w;
    std::vector<uint64_t> ord;
    PTX_TRY(check_read_strain_set(ctx, db, reads, sel, "strain_links", hap, w, ord, /*need_w=*/false));   // (the caller's order is kept: bit p = position p)
    PTX_TRY(check_stage_coverage(ctx, db, "strain_links"));
    const uint32_t S = db->S;
    if ((sel->cand_off[S] && !hap_out) || (S && (!species_out || !link_out))) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_links: null output array");
    return links_launch(ctx, db, reads, sel->cand_off, sel->cand_hap, species_out, link_out, hap_out, brk_off_out, cap, brk_step_out, brk_start_out,
                        brk_node_a_out, brk_node_b_out, brk_flank_out, brk_mask_out);
}

int pantax_hip_strain_rarefy(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_rarefy_set *sel, double *x_out, double *obj_out,
                             uint64_t *rows_out, int32_t *status_out, uint64_t *reads_out, uint64_t *member_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !reads || !sel || !sel->sel_off) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_rarefy: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_species_count(ctx, db, "strain_rarefy", sel->n_species));
    if (sel->n_levels == 0 || sel->n_levels > 16) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_rarefy: %u levels (1 .. 16)", sel->n_levels);
    if (sel->n_replicates == 0) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_rarefy: 0 replicates (at least one)");
    PTX_TRY(check_read_pass_state(ctx, db, reads, "strain_rarefy"));
    PTX_TRY(check_hap_selection(ctx, db, "strain_rarefy", sel->sel_off, sel->sel_hap));
    if ((sel->sel_off[db->S] && (!x_out || !member_out)) || (db->S && (!obj_out || !rows_out || !status_out || !reads_out)))
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_rarefy: null output array");
    PTX_TRY(check_stage_coverage(ctx, db, "strain_rarefy"));
    try {
        return rarefy_launch(ctx, db, reads, sel->sel_off, sel->sel_hap, sel->seed, sel->n_levels, sel->n_replicates, x_out, obj_out, rows_out, status_out, reads_out,
                             member_out);
    } catch (const std::bad_alloc &) {
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_rarefy: out of host memory");
    }
}

int pantax_hip_rarefy_node_bases(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, uint64_t seed, uint32_t replicate, uint32_t level,
                                 uint64_t *bases_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !reads || (db->V && !bases_out)) return fail(ctx, PANTAX_HIP_E_INVALID, "rarefy_node_bases: null argument");
    PTX_ENTER(ctx);
    if (level > 63) return fail(ctx, PANTAX_HIP_E_INVALID, "rarefy_node_bases: level %u (0 .. 63)", level);
    PTX_TRY(check_read_pass_state(ctx, db, reads, "rarefy_node_bases"));
    PTX_TRY(check_stage_coverage(ctx, db, "rarefy_node_bases"));
    return rarefy_node_bases_launch(ctx, db, reads, seed, replicate, level, bases_out);
}

int pantax_hip_strain_addin(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_near_miss_set *sel, double *x_out, double *obj_out, int32_t *status_out,
                            uint64_t *rows_out, uint64_t *count_out) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!db || !sel || !sel->sel_off || !sel->cand_off) return fail(ctx, PANTAX_HIP_E_INVALID, "strain_addin: null argument");
    PTX_ENTER(ctx);
    PTX_TRY(check_near_miss_set(ctx, db, "strain_addin", sel));
    // (x_out holds (J_s + 1) (K_s + J_s) doubles a species: none only when nothing is reported anywhere and there is no candidate)
    if (((sel->sel_off[db->S] || sel->cand_off[db->S]) && !x_out) || (db->S && (!obj_out || !status_out || !rows_out || !count_out)))
        return fail(ctx, PANTAX_HIP_E_INVALID, "strain_addin: null output array");
    PTX_TRY(check_stage_coverage(ctx, db, "strain_addin"));
    try {
        return addin_launch(ctx, db, sel->sel_off, sel->sel_hap, sel->cand_off, sel->cand_hap, x_out, obj_out, status_out, rows_out, count_out);
    } catch (const std::bad_alloc &) {
        return fail(ctx, PANTAX_HIP_E_LIMIT, "strain_addin: out of host memory");
    }
}

}  // extern "C"
