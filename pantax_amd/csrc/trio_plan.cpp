// trio_plan.cpp -- the unique-trio index's host-side decisions (trio_plan.hpp).  Nothing here touches the device.
#include "trio_plan.hpp"
#include <algorithm>

namespace ptx {

// u x rounds groups per wave, four waves per workgroup; `xcd`: the workgroups go to the XCDs round-robin and XCD x is given the x-th contiguous
// eighth of the chunks, so the grid is a multiple of eight and the kernel is told how many chunks hold groups
static TrioGroupGrid group_grid(uint32_t n_groups, int u_opt, int rounds_opt, bool xcd) {
    TrioGroupGrid g;
    g.u = u_opt == 2 ? 2u : u_opt == 8 ? 8u : 4u;
    g.rounds = (uint32_t)std::max(1, rounds_opt);
    g.chunks = (n_groups + 4u * g.u * g.rounds - 1u) / (4u * g.u * g.rounds);
    g.grid = xcd ? ((g.chunks + 7u) / 8u) * 8u : g.chunks;
    g.xcd_chunks = xcd ? g.chunks : 0u;
    return g;
}

TrioPlan trio_plan(const TrioPlanIn &in) {
    TrioPlan p;
    const uint64_t P = in.P, V = in.V;
    // which uniqueness path: the visit table (default; species with a node of more than 64 visits: by node block), or through global buckets
    // for the whole db (a species of >= 2^27 nodes among those left to the node-block kernel, or forced)
    p.by_block = in.trio_block_ok && (in.trio_visit_ok || in.n_blocks) && in.trio_path != "bucket";
    p.rows_by_visit = p.by_block && P && in.n_vgroups && in.trio_rows != "path";
    p.path_route = P && (!p.rows_by_visit || in.n_blocks != 0);
    p.mixed = p.rows_by_visit && p.path_route;
    // first build of a db -- or the first one that files the species in another order (the options trio_rows / trio_path changed between two
    // builds: tests)
    p.first_build = !in.trio_sizes_known || in.trio_layout_fast != p.rows_by_visit;
    // a rebuild of a db whose group offsets are known: uniqueness and filing of the visit table's species in one pass (trio_file_kernel)
    p.fused = p.rows_by_visit && !p.first_build && in.have_gprefix && in.gprefix_for == in.n_vgroups && !in.trio_two_pass;
    p.with_keys = in.with_keys;
    p.n_win = in.n_win;

    p.run_file = p.fused;
    p.run_visit = P && p.by_block && in.n_vgroups && !p.fused;
    p.run_block = P && p.by_block && in.n_blocks;
    p.run_bucket = P && !p.by_block;
    p.run_uniq = p.run_bucket && in.n_win;
    // mean bucket size decides: short buckets (few haplotypes per node) compare through shuffles, long ones hash
    // (measured: 7 windows per node -> shuffles 0.050 vs hash 0.058 ms; 34 per node -> 4.66 vs 1.69 ms)
    p.uniq_hashed = p.run_uniq && (in.uniq_hash >= 0 ? in.uniq_hash == 1 : in.n_win > 16 * V);
    p.run_rows = p.rows_by_visit && !p.fused;
    if (p.run_rows) p.prefix = in.flag_rank_chained ? TrioPrefix::chained : TrioPrefix::tiles;
    if (p.path_route) p.head_scan = p.mixed ? TrioHeadScan::slow_first : TrioHeadScan::trio_first;
    p.release_records = p.first_build && p.rows_by_visit && !in.trio_two_pass;

    // trio_xcd: bit 0 the visit / file kernel, bit 1 the rows kernel take their workgroups in XCD-contiguous chunks (measurements)
    const uint32_t xcd = (uint32_t)in.trio_xcd;
    p.visit = group_grid(in.n_vgroups, in.tv_u, in.tv_rounds, xcd & 1u);
    p.file = group_grid(in.n_vgroups, in.tf_u, in.tf_rounds, xcd & 1u);
    p.rows.u = in.rows_u == 2 ? 2u : in.rows_u == 4 ? 4u : 1u;
    p.rows.rchunks = (in.n_vgroups + 32 * p.rows.u - 1) / (32 * p.rows.u);
    // a first build counts the rows per haplotype: 64 chunks per workgroup share one set of LDS counters (no XCD chunking there)
    p.rows.iters = p.first_build ? 64u : 1u;
    p.rows.rxcd = (xcd & 2u) && !p.first_build;
    p.rows.grid = p.first_build ? (p.rows.rchunks + p.rows.iters - 1) / p.rows.iters : p.rows.rxcd ? ((p.rows.rchunks + 7u) / 8u) * 8u : p.rows.rchunks;
    p.rows.xcd_chunks = p.rows.rxcd ? p.rows.rchunks : 0u;
    p.tb_slots = in.tb_slots == 512 ? 512 : in.tb_slots == 128 ? 128 : 256;

    TrioArena &a = p.arena;
    a.zbits = (size_t)((P + 31) / 32 + 1);
    if (p.path_route) {
        a.zwords = a.zbits + (size_t)(V + 1) + (p.by_block ? 0 : 2 * (size_t)(V + 1));
        a.clear = p.by_block ? a.zbits : a.zwords;
        a.off_first_cnt = a.zbits;
        if (!p.by_block) { a.off_cnt = a.zbits + (size_t)(V + 1); a.off_cursor = a.zbits + 2 * (size_t)(V + 1); }
    }
    return p;
}

TrioBlockTable trio_block_table(const std::vector<uint64_t> &node_off, const std::vector<uint8_t> &slow) {
    TrioBlockTable t;
    const size_t S = slow.size();
    t.blk_base.assign(S + 1, 0);
    for (size_t s = 0; s < S; ++s) {
        const uint64_t Vs = slow[s] ? node_off[s + 1] - node_off[s] : 0;   // blocks only where the visit table leaves a species to this path
        if (Vs >= (1ull << 27)) return t;             // the packed LDS key holds 27-bit local ids: such a db keeps the bucket path
        const uint64_t nb = (uint64_t)t.blk_base[s] + ((Vs + TRIO_BLK - 1) >> TRIO_BLK_SHIFT);
        if (nb >= 0x7FFFFFFFull) return t;
        t.blk_base[s + 1] = (uint32_t)nb;
    }
    t.n_blocks = t.blk_base[S];
    t.ok = true;
    return t;
}

std::vector<TrioVisitChunk> trio_visit_chunks(const std::vector<uint64_t> &node_off, const std::vector<uint32_t> &slow, bool force_block) {
    std::vector<TrioVisitChunk> chunks;
    if (force_block) return chunks;
    for (size_t s = 0; s < slow.size(); ++s) {
        if (slow[s]) continue;
        for (uint64_t v = node_off[s]; v < node_off[s + 1]; v += (1u << VIS_CHUNK_SHIFT))
            chunks.push_back({(uint32_t)v, (uint32_t)std::min<uint64_t>(v + (1u << VIS_CHUNK_SHIFT), node_off[s + 1]), (uint32_t)node_off[s], (uint32_t)s});
    }
    return chunks;
}

}  // namespace ptx
