// stage_trio.hip -- a7: the unique-trio index (trio_nodes_info, profile.rs:658-740) on device: the build as named phases (trio_index_build), the export
// order, and the two entry points.
//
// Reference: every 3-window of every haplotype walk, canonicalised by swapping the ends when
// w[0] > w[2] (:672-678); count_per_trio counts every (hap, position) occurrence (:688-702); a
// trio is strain-specific ("unique") iff that count is exactly 1 (:708-716); its length is the
// sum of its three node lengths (:712).  The reference keeps a dense trio x hap presence matrix;
// a unique trio has exactly one owner, so an owner index per row carries the same information.
//
// The plan, as the files of the stage carry it out (trio_plan.hpp decides which of it runs; all species of the db in one batch, no sort):
//   uniqueness  Every occurrence of a window shares its MIDDLE node b, so count == 1 is a question about the visits of b.  By default the VISIT
//               TABLE answers it (stage_trio_tables.hip builds it at upload: the walks transposed, the interior positions node by node in groups
//               of 64 that no node straddles, a node's visits sorted by their pair of ends): one wave holds every visit of its group's nodes and
//               compares neighbouring lanes (trio_visit_kernel, stage_trio_uniq.hip).  A species that holds a node of more than 64 visits goes
//               by NODE BLOCKS of 64 ids, whose windows meet in an LDS hash table (trio_block_kernel).  A db the blocks cannot take (a species of
//               2^27 nodes among those, or trio_path=bucket) falls back to global BUCKETS per middle node (trio_count / fill / uniq kernels).
//   rows        A row is a unique window, NUMBERED IN FILING ORDER (stage_trio_rows.hip): the visit table's species in table order from the
//               visit kernel's records (trio_rows_kernel), behind them the other species by a pass over their walks (trio_lookup_kernel,
//               trio_canon_kernel); a node's rows are neighbours, sorted by their pair of ends, and its record carries {first row, #rows}.
//               A rebuild of a db whose group offsets are known decides and files in one pass over the table (trio_file_kernel).
//   export      The (species, hap, position) order the C ABI hands out is a permutation made on request (below); it replaces the reference's
//               FxHashSet iteration order, which is arbitrary: results are compared as keyed sets.
// History: round 1 counted windows per node, scattered them into buckets and compared inside each bucket, with rows numbered in (species, hap,
// position) order; that plan survives as the bucket fallback.
#include <algorithm>
#include <cstdlib>
#include "trio_device.hpp"

namespace ptx {

// ---- the export order: rows listed in (species, hap, position) order = ascending window start (the walks are one CSR over all haplotypes) ----
__global__ void __launch_bounds__(256) trio_iota_kernel(uint32_t n, uint32_t *__restrict__ v, const uint32_t *__restrict__ q, unsigned long long *__restrict__ key) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { v[i] = i; key[i] = q[i]; }
}
// export copies of the table in that order: canonical key (species-local), owner haplotype, length
__global__ void __launch_bounds__(256) trio_export_kernel(uint32_t n, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ q, const uint32_t *__restrict__ path_nodes,
                                                          const uint16_t *__restrict__ hap, const trio_len_t *__restrict__ len, uint32_t *__restrict__ abc_out,
                                                          uint32_t *__restrict__ hap_out, uint32_t *__restrict__ len_out) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint32_t row = perm[e], p = q[row];
    uint32_t a = path_nodes[p], b = path_nodes[p + 1], c = path_nodes[p + 2];
    if (a > c) { const uint32_t t = a; a = c; c = t; }                     // profile.rs:672-678
    if (abc_out) { abc_out[3ull * e] = a; abc_out[3ull * e + 1] = b; abc_out[3ull * e + 2] = c; }
#if TRIO_LH_PACK
    if (hap_out) hap_out[e] = len[row].y;
    if (len_out) len_out[e] = len[row].x;
#else
    if (hap_out) hap_out[e] = hap[row];
    if (len_out) len_out[e] = len[row];
#endif
}
__global__ void __launch_bounds__(256) gather_u64_kernel(uint32_t n, const uint32_t *__restrict__ perm, const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = src[perm[e]];
}

// ---- trio_index_build: the plan (trio_plan.hpp), then named phases in one enqueue order on ctx->stream ----
static TrioPlanIn trio_plan_in(const Ctx *ctx, const Db *db, bool with_keys) {
    const CtxConfig &c = ctx->cfg;
    const TrioScratch &ts = db->trio_scratch;
    TrioPlanIn in;
    in.P = db->P; in.V = db->V; in.H = (uint32_t)db->H; in.S = db->S;
    in.n_vgroups = db->n_vgroups; in.n_blocks = db->n_blocks;
    in.trio_visit_ok = db->trio_visit_ok; in.trio_block_ok = db->trio_block_ok;
    in.trio_sizes_known = db->trio_sizes_known; in.trio_layout_fast = db->trio_layout_fast;
    in.have_gprefix = ts.gprefix.p != nullptr; in.gprefix_for = ts.gprefix_for;
    in.with_keys = with_keys;
    in.trio_path = c.trio_path; in.trio_rows = c.trio_rows; in.trio_two_pass = c.trio_two_pass; in.uniq_hash = c.uniq_hash; in.flag_rank_chained = c.flag_rank_chained;
    in.tv_u = c.tv_u; in.tv_rounds = c.tv_rounds; in.tf_u = c.tf_u; in.tf_rounds = c.tf_rounds; in.rows_u = c.rows_u; in.tb_slots = c.tb_slots; in.trio_xcd = c.trio_xcd;
    return in;
}
// number of windows: every hap with len >= 3 contributes len-2
static uint64_t trio_window_count(const Db *db) {
    uint64_t n_win = 0;
    for (uint64_t h = 0; h < db->H; ++h) { uint64_t l = db->h_path_off[h + 1] - db->h_path_off[h]; if (l >= 3) n_win += l - 2; }
    return n_win;
}

// 1. scratch and clears.  One arena for what the path route needs cleared: uniq bits (one per path position) | first_cnt [| cnt | cursor].  The
// visit-table / node-block kernels STORE the count of every node that has a visit (the others read as zero through `d_node_visited`), the lookup
// pass counts them back down to zero in place of a cursor array; cnt / cursor belong to the bucket path.  The fast route clears nothing.
static int trio_scratch_prepare(Ctx *ctx, Db *db, const TrioPlan &pl) {
    TrioScratch &ts = db->trio_scratch;
    const uint64_t V = db->V;
    const uint32_t H = (uint32_t)db->H;
    const TrioArena &a = pl.arena;
    if (pl.path_route) {
        PTX_HIP(ctx, ts.zero_arena.alloc(a.zwords));
        ts.uniq_q.view(ts.zero_arena.p + a.off_uniq_q, a.zbits);
        ts.first_cnt.view(ts.zero_arena.p + a.off_first_cnt, V + 1);
        if (!pl.by_block) { ts.cnt.view(ts.zero_arena.p + a.off_cnt, V + 1); ts.cursor.view(ts.zero_arena.p + a.off_cursor, V + 1); }
        if (!pl.by_block) PTX_HIP(ctx, ts.bucket_off.alloc(V + 1));
        PTX_TRY(zero_fill(ctx, ts.zero_arena.p, a.clear * sizeof(uint32_t)));
        if (pl.by_block) PTX_HIP(ctx, hipMemsetAsync(ts.first_cnt.p + V, 0, sizeof(uint32_t), ctx->stream));   // the closing entry of the count scan
        PTX_HIP(ctx, db->d_trio_first.alloc(V + 1));
    }
    PTX_HIP(ctx, ts.scan_tmp.alloc(16));
    PTX_HIP(ctx, ts.d_tot.alloc(4));
    PTX_HIP(ctx, hipMemsetAsync(ts.d_tot.p, 0, 4 * sizeof(uint32_t), ctx->stream));   // {-, rows of the fast route, error word of the build kernels, rows of the path route}
    if (pl.run_rows) {
        PTX_HIP(ctx, ts.vis_uq.alloc(db->n_vgroups + 1)); PTX_HIP(ctx, ts.vis_rec.alloc((uint64_t)db->n_vgroups * VIS_REC));
        PTX_HIP(ctx, ts.gprefix.alloc(db->n_vgroups + 1));
        ts.gprefix_for = 0;
        PTX_HIP(ctx, hipMemsetAsync(ts.vis_uq.p + db->n_vgroups, 0, sizeof(uint64_t), ctx->stream));   // the closing entry of the count scan
    }
    if (pl.first_build) {
        PTX_HIP(ctx, ts.hap_cnt.alloc(H + 1));
        PTX_HIP(ctx, hipMemsetAsync(ts.hap_cnt.p, 0, ((size_t)H + 1) * sizeof(uint32_t), ctx->stream));
    }
    PTX_HIP(ctx, db->d_hap_trio_off.alloc(H + 1));
    return 0;
}

// 5. totals (first build only).  U is a function of the graphs alone: a rebuild (pantax_hip_db_reset) reuses the size learnt by the first build
static int trio_totals(Ctx *ctx, Db *db) {
    uint32_t tot[4] = {0, 0, 0, 0};
    PTX_TRY(download(ctx, tot, db->trio_scratch.d_tot.p, 4));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    db->U_known = (uint64_t)tot[1] + tot[3];
    if (db->U_known >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "trio_index: %llu unique trios exceed 32-bit rows", (unsigned long long)db->U_known);
    return 0;
}

// 6. row tables of db->U_known rows, and what filing a row writes into them
static int trio_row_tables(Ctx *ctx, Db *db, const TrioPlan &pl, RowOut &ro) {
    const uint32_t Utot = (uint32_t)db->U_known;
    PTX_HIP(ctx, db->d_trio_ent.alloc((size_t)Utot + 1)); PTX_HIP(ctx, db->d_trio_len.alloc(Utot));   // (+ 1: the coverage pass loads entries in pairs)
#if !TRIO_LH_PACK
    PTX_HIP(ctx, db->d_trio_hap.alloc(Utot));
#endif
    if (pl.with_keys) PTX_HIP(ctx, db->d_trio_q.alloc(Utot));
    if (pl.path_route) PTX_HIP(ctx, db->trio_scratch.row_q.alloc(Utot));
    ro = RowOut{db->d_node_len.p, db->d_path_off.p, db->d_hap_off.p, db->d_trio_ent.p, db->d_trio_len.p, const_cast<uint16_t *>(TRIO_HAP_PTR(db)), db->d_trio_q.p,
                db->trio_scratch.hap_cnt.p};
    return 0;
}

// 8. first-build epilogue: rows per haplotype -> hap_trio_off (the counts the first filter reads; the offsets of the export order), rows per
// species -> the chunk table of the per-haplotype statistics; the error word of the build kernels is read HERE, behind all of them
static int trio_first_build_epilogue(Ctx *ctx, Db *db, const TrioPlan &pl) {
    TrioScratch &ts = db->trio_scratch;
    const uint32_t H = (uint32_t)db->H, S = db->S;
    std::vector<uint32_t> hc(H + 1, 0);
    uint32_t err = 0;
    PTX_TRY(download(ctx, hc.data(), ts.hap_cnt.p, H));
    PTX_TRY(download(ctx, &err, ts.d_tot.p + 2, 1));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (err) return fail(ctx, PANTAX_HIP_E_LIMIT, "trio_index: %u problems in the build kernels: a node that heads 2^16 or more unique-trio rows, node blocks that could not be "
                                                  "resolved in LDS (trio_path=bucket), or visit groups out of order", err);
    db->h_hap_trio_off.assign(H + 1, 0);
    for (uint32_t h = 0; h < H; ++h) db->h_hap_trio_off[h + 1] = db->h_hap_trio_off[h] + hc[h];
    if (db->h_hap_trio_off[H] != db->U_known)
        return fail(ctx, PANTAX_HIP_E_STATE, "trio_index: %llu rows were filed but %llu counted", (unsigned long long)db->h_hap_trio_off[H], (unsigned long long)db->U_known);
    PTX_TRY(upload(ctx, db->d_hap_trio_off, db->h_hap_trio_off.data(), H + 1));
    // filing order of the species: those of the fast route first (in species order), then those of the path route
    db->h_sp_row_order.clear();
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t s = 0; s < S; ++s) {
            const bool fast = pl.rows_by_visit && !db->h_trio_slow[s];
            if (fast == (pass == 0)) db->h_sp_row_order.push_back(s);
        }
    {
        uint64_t at = 0;
        std::vector<uint64_t> first(S, 0), cnt(S, 0);
        for (uint32_t s : db->h_sp_row_order) {
            cnt[s] = db->h_hap_trio_off[db->h_hap_off[s + 1]] - db->h_hap_trio_off[db->h_hap_off[s]];
            first[s] = at; at += cnt[s];
        }
        PTX_TRY(hap_stats_layout(ctx, db, first.data(), cnt.data()));
    }
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    db->trio_sizes_known = true;
    db->trio_layout_fast = pl.rows_by_visit;
    // later builds file in one pass and need neither the records (16 B x 8 per group: 4.7 GB at 1e4 strains) nor the groups' ballots
    if (pl.release_records) { ts.vis_rec.release(); ts.vis_uq.release(); }
    return 0;
}

// The index of a db: uniqueness (visit table; node blocks or global buckets for what it does not cover), then the rows (stage_trio_rows.hip: fast
// route, path route, or the one-pass rebuild).  Which of it runs is the plan's; the order below is the order on the stream.
// with_keys: the window start of every row is kept as well (d_trio_q): what the exporters build the (species, hap, position) order from.
int trio_index_build(Ctx *ctx, Db *db, bool with_keys) {
    const bool same_rows = db->trio.built();   // (the exporters' rebuild with the window starts: a row keeps its number, a coverage result stays valid)
    db->trio.build_begun();
    if (db->P >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "trio_index: %llu path steps exceed 32-bit positions", (unsigned long long)db->P);
    TrioPlanIn in = trio_plan_in(ctx, db, with_keys);
    TrioPlan pl = trio_plan(in);
    if (pl.run_bucket) { in.n_win = trio_window_count(db); pl = trio_plan(in); }   // the bucket path alone asks how many windows there are: no rebuild walks h_path_off
    RowOut ro{};
    PTX_TRY(trio_scratch_prepare(ctx, db, pl));                                    // 1. scratch and clears
    if (pl.run_file) {                                                             // 2. fused filing (the size is known: the tables first)
        PTX_TRY(trio_row_tables(ctx, db, pl, ro));
        PTX_TRY(trio_file_launch(ctx, db, pl, ro));
    }
    if (pl.run_visit) PTX_TRY(trio_visit_launch(ctx, db, pl));                     // 3. uniqueness
    if (pl.run_block) PTX_TRY(trio_block_launch(ctx, db, pl));
    if (pl.run_bucket) PTX_TRY(trio_bucket_launch(ctx, db, pl));
    if (pl.prefix != TrioPrefix::none) PTX_TRY(trio_group_prefix(ctx, db, pl));    // 4. sizes: the first row of every group (fast route) ...
    if (pl.head_scan != TrioHeadScan::none) PTX_TRY(trio_head_scan(ctx, db, pl));  //    ... and of every node (path route)
    if (pl.first_build) PTX_TRY(trio_totals(ctx, db));                             // 5. totals
    db->U = (uint32_t)db->U_known;
    if (!pl.run_file) PTX_TRY(trio_row_tables(ctx, db, pl, ro));                   // 6. row tables
    if (pl.run_rows) PTX_TRY(trio_rows_launch(ctx, db, pl, ro));                   // 7. rows
    if (pl.path_route) PTX_TRY(trio_path_rows_launch(ctx, db, pl, ro));
    PTX_HIP(ctx, hipGetLastError());
    if (pl.first_build) PTX_TRY(trio_first_build_epilogue(ctx, db, pl));           // 8. first-build epilogue
    db->trio.build_finished(with_keys);
    if (!same_rows) db->cov.invalidated();
    return 0;
}

// the window start of every row is wanted (the exporters): rebuild with it unless it is there
int trio_keys_ensure(Ctx *ctx, Db *db) {
    if (db->trio.has_keys()) return 0;
    if (db->step_inflight) return fail(ctx, PANTAX_HIP_E_STATE, "trio tables: %d enqueued step(s) of this db have not been collected", db->step_inflight);
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream2));   // a step's rebuild on the side stream is over before the tables are replaced
    return trio_index_build(ctx, db, true);
}

// d_trio_perm[e] = the row of the e-th window in (species, hap, position) order: the rows sorted by their window start (the walks of all
// haplotypes are one CSR in that order).  Off the step's path: only pantax_hip_trio_get and the trio_bases of pantax_hip_node_coverage ask.
int trio_export_ensure(Ctx *ctx, Db *db) {
    PTX_TRY(trio_keys_ensure(ctx, db));
    if (db->trio.export_order_valid()) return 0;
    const uint64_t U = db->U;
    PTX_HIP(ctx, db->d_trio_perm.alloc(U ? U : 1));
    if (U) {
        DevBuf<uint64_t> ka, kb;
        DevBuf<uint32_t> vb, table, tmp;
        PTX_HIP(ctx, ka.alloc(U)); PTX_HIP(ctx, kb.alloc(U)); PTX_HIP(ctx, vb.alloc(U)); PTX_HIP(ctx, table.alloc(sort_table_elems(U))); PTX_HIP(ctx, tmp.alloc(16));
        hipLaunchKernelGGL(trio_iota_kernel, dim3((uint32_t)((U + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t)U, db->d_trio_perm.p, (const uint32_t *)db->d_trio_q.p,
                           reinterpret_cast<unsigned long long *>(ka.p));
        SortBufs A, B;
        A.nw = B.nw = 1; A.k[0] = ka.p; B.k[0] = kb.p; A.v = db->d_trio_perm.p; B.v = vb.p;
        std::vector<SortPass> passes;
        add_passes(passes, 0, 0, bits_for(db->P ? db->P : 1));
        bool in_b = false;
        PTX_TRY(radix_sort(ctx, A, B, U, passes.data(), (int)passes.size(), table.p, tmp.p, &in_b, nullptr));
        if (in_b) PTX_HIP(ctx, hipMemcpyAsync(db->d_trio_perm.p, vb.p, U * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the sort's buffers go out of scope
    }
    db->trio.export_order_made();
    return 0;
}

// rows in export order: out[e] = src[row of e] (trio_bases of pantax_hip_node_coverage)
int trio_export_u64(Ctx *ctx, Db *db, const unsigned long long *d_src, unsigned long long *d_dst) {
    PTX_TRY(trio_export_ensure(ctx, db));
    if (db->U) hipLaunchKernelGGL(gather_u64_kernel, dim3((uint32_t)((db->U + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t)db->U, (const uint32_t *)db->d_trio_perm.p, d_src, d_dst);
    PTX_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace ptx

using namespace ptx;
extern "C" {

int pantax_hip_trio_index(pantax_hip_ctx *ctx, pantax_hip_db *db, uint64_t *n_unique_total_out) {
    if (!ctx || !db) return PANTAX_HIP_E_INVALID;
    PTX_ENTER(ctx);
    if (!db->trio.built()) {
        const bool rebuild = db->trio_sizes_known;
        PTX_TRY(trio_index_build(ctx, db));
        // a db's FIRST build reads the error word of its kernels itself; a rebuild (after pantax_hip_db_reset) leaves it for the pipelined step to
        // fetch with its results.  A stage caller consumes the index right away (trio_get, node_coverage): the word is read here, behind the build
        if (rebuild && db->trio_scratch.d_tot.p) {
            uint32_t err = 0;
            PTX_TRY(download(ctx, &err, db->trio_scratch.d_tot.p + 2, 1));
            PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (err) {
                db->index_invalidate();
                return fail(ctx, PANTAX_HIP_E_LIMIT, "trio_index: %u problems in the rebuild's kernels: visit groups out of order / offsets that are not this table's, or a node "
                                                     "that heads 2^16 or more unique-trio rows", err);
            }
        }
    }
    if (n_unique_total_out) *n_unique_total_out = db->U;
    return 0;
}

int pantax_hip_trio_get(pantax_hip_ctx *ctx, const pantax_hip_db *cdb, uint32_t *abc_out, uint32_t *hap_out, int64_t *len_out,
                        uint64_t *hap_trio_off_out) {
    if (!ctx || !cdb) return PANTAX_HIP_E_INVALID;
    pantax_hip_db *db = const_cast<pantax_hip_db *>(cdb);
    if (!db->trio.built()) return fail(ctx, PANTAX_HIP_E_STATE, "trio_get: call pantax_hip_trio_index first");
    PTX_ENTER(ctx);
    const uint64_t U = db->U;
    if ((abc_out || hap_out || len_out) && U) {
        // the table in (species, hap, position) order is an export: the rows are permuted on the device (the last build may have been a
        // step's, without the window starts: the same index is built again with them)
        PTX_TRY(trio_export_ensure(ctx, db));
        DevBuf<uint32_t> d_abc, d_hap, d_len;
        if (abc_out) PTX_HIP(ctx, d_abc.alloc(3 * U));
        if (hap_out) PTX_HIP(ctx, d_hap.alloc(U));
        if (len_out) PTX_HIP(ctx, d_len.alloc(U));
        hipLaunchKernelGGL(trio_export_kernel, dim3((uint32_t)((U + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t)U, (const uint32_t *)db->d_trio_perm.p,
                           (const uint32_t *)db->d_trio_q.p, (const uint32_t *)db->d_path_nodes.p, TRIO_HAP_PTR(db), (const trio_len_t *)db->d_trio_len.p,
                           abc_out ? d_abc.p : (uint32_t *)nullptr, hap_out ? d_hap.p : (uint32_t *)nullptr, len_out ? d_len.p : (uint32_t *)nullptr);
        PTX_HIP(ctx, hipGetLastError());
        std::vector<uint32_t> len32;
        if (abc_out) PTX_TRY(download(ctx, abc_out, d_abc.p, 3 * U));
        if (hap_out) PTX_TRY(download(ctx, hap_out, d_hap.p, U));
        if (len_out) { len32.resize(U); PTX_TRY(download(ctx, len32.data(), d_len.p, U)); }
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (len_out) for (uint64_t u = 0; u < U; ++u) len_out[u] = len32[u];
    }
    if (hap_trio_off_out) for (uint64_t h = 0; h <= db->H; ++h) hap_trio_off_out[h] = db->h_hap_trio_off[h];
    return 0;
}
}
