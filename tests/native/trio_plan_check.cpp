// trio_plan_check.cpp -- the unique-trio index's host-side decisions (pantax_amd/csrc/trio_plan.hpp) at their edges.  A program of its own:
// tests/test_trio_plan.py compiles it with trio_plan.cpp by the host compiler under -fsanitize=address,undefined and runs it; it returns non-zero at
// the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "trio_plan.hpp"

using namespace ptx;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "trio_plan_check:%d: %s\n", __LINE__, #cond);    \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

// a db the visit table covers whole: 1000 groups, no blocks, nothing built yet, default options
static TrioPlanIn narrow_db() {
    TrioPlanIn in;
    in.P = 100000; in.V = 5000; in.H = 20; in.S = 4;
    in.n_vgroups = 1000; in.n_blocks = 0;
    in.trio_visit_ok = true; in.trio_block_ok = true;
    return in;
}
// the same db after its first build by the fast route
static TrioPlanIn narrow_db_built() {
    TrioPlanIn in = narrow_db();
    in.trio_sizes_known = true; in.trio_layout_fast = true; in.have_gprefix = true; in.gprefix_for = in.n_vgroups;
    return in;
}
static TrioPlanIn mixed_db() {
    TrioPlanIn in = narrow_db();
    in.n_blocks = 37;
    return in;
}
// brackets that launch kernels
static int n_brackets(const TrioPlan &p) {
    return (int)p.run_file + p.run_visit + p.run_block + p.run_bucket + p.run_uniq + (p.prefix != TrioPrefix::none) + p.run_rows + (p.head_scan != TrioHeadScan::none) +
           p.path_route;
}

static void routes() {
    {   // visit table and no blocks, first build: visit + prefix + rows
        const TrioPlan p = trio_plan(narrow_db());
        CHECK(p.by_block && p.rows_by_visit && !p.path_route && !p.mixed && p.first_build && !p.fused);
        CHECK(p.run_visit && p.prefix == TrioPrefix::tiles && p.run_rows);
        CHECK(!p.run_file && !p.run_block && !p.run_bucket && !p.run_uniq && p.head_scan == TrioHeadScan::none);
        CHECK(n_brackets(p) == 3 && p.release_records);
        CHECK(p.arena.zwords == 0 && p.arena.clear == 0);       // the fast route clears nothing
    }
    {   // the same db, sizes known, the offsets are this table's: one pass
        const TrioPlan p = trio_plan(narrow_db_built());
        CHECK(p.rows_by_visit && !p.first_build && p.fused && p.run_file);
        CHECK(n_brackets(p) == 1 && !p.release_records);
        TrioPlanIn in = narrow_db_built();
        in.gprefix_for = in.n_vgroups - 1;                      // offsets of another table
        TrioPlan q = trio_plan(in);
        CHECK(!q.fused && !q.run_file && !q.first_build && q.run_visit && q.prefix == TrioPrefix::tiles && q.run_rows && n_brackets(q) == 3);
        in = narrow_db_built();
        in.have_gprefix = false;
        q = trio_plan(in);
        CHECK(!q.fused && q.run_visit && q.run_rows);
        in = narrow_db_built();
        in.trio_two_pass = true;
        q = trio_plan(in);
        CHECK(!q.fused && !q.run_file && !q.first_build && q.run_visit && q.prefix == TrioPrefix::tiles && q.run_rows && n_brackets(q) == 3);
        in.flag_rank_chained = true;
        CHECK(trio_plan(in).prefix == TrioPrefix::chained);
    }
    {   // the layout the sizes were learnt by differs from the route: a first build again
        TrioPlanIn in = narrow_db_built();
        in.trio_layout_fast = false;
        TrioPlan p = trio_plan(in);
        CHECK(p.rows_by_visit && p.first_build && !p.fused && p.run_visit && p.run_rows);
        in = narrow_db_built();
        in.trio_rows = "path";
        p = trio_plan(in);
        CHECK(!p.rows_by_visit && p.first_build && !p.fused);
    }
    {   // blocks and visit groups together: mixed, the block species' heads behind the fast rows
        TrioPlan p = trio_plan(mixed_db());
        CHECK(p.by_block && p.rows_by_visit && p.path_route && p.mixed && p.first_build);
        CHECK(p.run_visit && p.run_block && p.prefix == TrioPrefix::tiles && p.run_rows && p.head_scan == TrioHeadScan::slow_first);
        CHECK(!p.run_file && !p.run_bucket && n_brackets(p) == 6);
        CHECK(p.arena.zbits == (100000 + 31) / 32 + 1 && p.arena.zwords == p.arena.zbits + 5001 && p.arena.clear == p.arena.zbits);
        CHECK(p.arena.off_uniq_q == 0 && p.arena.off_first_cnt == p.arena.zbits);
        TrioPlanIn in = mixed_db();                             // its rebuild: the fast species in one pass, the others as before
        in.trio_sizes_known = true; in.trio_layout_fast = true; in.have_gprefix = true; in.gprefix_for = in.n_vgroups;
        p = trio_plan(in);
        CHECK(p.fused && p.mixed && p.run_file && !p.run_visit && p.run_block && p.prefix == TrioPrefix::none && !p.run_rows);
        CHECK(p.head_scan == TrioHeadScan::slow_first && p.path_route && n_brackets(p) == 4);
    }
    {   // blocks only, or trio_rows=path: one route, every node's head
        TrioPlanIn in = mixed_db();
        in.n_vgroups = 0;
        TrioPlan p = trio_plan(in);
        CHECK(p.by_block && !p.rows_by_visit && p.path_route && !p.mixed && !p.run_visit && p.run_block && p.head_scan == TrioHeadScan::trio_first);
        CHECK(p.prefix == TrioPrefix::none && !p.run_rows && n_brackets(p) == 3);
        in = mixed_db();
        in.trio_rows = "path";
        p = trio_plan(in);
        CHECK(p.by_block && !p.rows_by_visit && p.path_route && !p.mixed && p.run_visit && p.run_block && p.head_scan == TrioHeadScan::trio_first);
        CHECK(p.prefix == TrioPrefix::none && !p.run_rows && n_brackets(p) == 4);
        in = narrow_db();
        in.trio_rows = "path";
        p = trio_plan(in);
        CHECK(!p.mixed && p.run_visit && !p.run_block && p.head_scan == TrioHeadScan::trio_first && n_brackets(p) == 3);
    }
    {   // trio_visit_ok == false with blocks: the block path
        TrioPlanIn in = mixed_db();
        in.trio_visit_ok = false; in.n_vgroups = 0;
        const TrioPlan p = trio_plan(in);
        CHECK(p.by_block && !p.rows_by_visit && p.run_block && !p.run_visit && !p.run_bucket && p.head_scan == TrioHeadScan::trio_first);
        in.n_blocks = 0;                                        // neither table
        CHECK(!trio_plan(in).by_block && trio_plan(in).run_bucket);
    }
}

static void buckets() {
    TrioPlanIn in = narrow_db();
    in.trio_path = "bucket";
    in.n_win = 16 * in.V;
    TrioPlan p = trio_plan(in);
    CHECK(!p.by_block && !p.rows_by_visit && p.path_route && !p.mixed && p.first_build && !p.fused);
    CHECK(p.run_bucket && p.run_uniq && !p.run_visit && !p.run_block && !p.run_file && p.head_scan == TrioHeadScan::trio_first);
    CHECK(p.prefix == TrioPrefix::none && !p.run_rows && !p.release_records);
    // cnt and cursor in the arena, all of it cleared
    const size_t zb = (100000 + 31) / 32 + 1, v1 = 5001;
    CHECK(p.arena.zbits == zb && p.arena.zwords == zb + 3 * v1 && p.arena.clear == p.arena.zwords);
    CHECK(p.arena.off_uniq_q == 0 && p.arena.off_first_cnt == zb && p.arena.off_cnt == zb + v1 && p.arena.off_cursor == zb + 2 * v1);
    // the hashed test from more than 16 windows per node
    CHECK(!p.uniq_hashed && p.n_win == 16 * in.V);
    in.n_win = 16 * in.V + 1;
    CHECK(trio_plan(in).uniq_hashed);
    in.uniq_hash = 0;
    CHECK(!trio_plan(in).uniq_hashed);
    in.n_win = 16 * in.V; in.uniq_hash = 1;
    CHECK(trio_plan(in).uniq_hashed);
    in.n_win = 0;                                               // no windows: nothing to test, whatever the option says
    p = trio_plan(in);
    CHECK(p.run_bucket && !p.run_uniq && !p.uniq_hashed);
    // !trio_block_ok and no override: buckets
    in = mixed_db();
    in.trio_block_ok = false;
    p = trio_plan(in);
    CHECK(!p.by_block && p.run_bucket && !p.run_visit && !p.run_block && !p.rows_by_visit && p.arena.clear == p.arena.zwords && p.arena.zwords == zb + 3 * v1);
    // a rebuild on the bucket path learns nothing again
    in = narrow_db();
    in.trio_path = "bucket"; in.trio_sizes_known = true; in.trio_layout_fast = false;
    p = trio_plan(in);
    CHECK(!p.first_build && p.run_bucket && !p.fused);
}

static void empty_db() {
    TrioPlanIn in;
    in.P = 0; in.V = 0; in.trio_visit_ok = false; in.trio_block_ok = false;
    TrioPlan p = trio_plan(in);
    CHECK(n_brackets(p) == 0 && !p.path_route && !p.rows_by_visit && !p.fused && p.first_build);
    CHECK(p.arena.zbits == 1 && p.arena.zwords == 0 && p.arena.clear == 0);
    in = narrow_db();
    in.P = 0;                                                   // tables of a db without path steps
    p = trio_plan(in);
    CHECK(n_brackets(p) == 0 && !p.path_route && !p.rows_by_visit);
    in.trio_path = "bucket";
    CHECK(n_brackets(trio_plan(in)) == 0);
}

static void shapes() {
    TrioPlanIn in = narrow_db();
    TrioPlan p = trio_plan(in);
    CHECK(p.visit.u == 4 && p.visit.rounds == 4 && p.file.u == 8 && p.file.rounds == 1 && p.rows.u == 1 && p.tb_slots == 256);   // the defaults
    for (int u : {2, 4, 8}) { in.tv_u = u; in.tf_u = u; p = trio_plan(in); CHECK(p.visit.u == (uint32_t)u && p.file.u == (uint32_t)u); }
    for (int u : {3, 0, -1, 16}) { in.tv_u = u; in.tf_u = u; p = trio_plan(in); CHECK(p.visit.u == 4 && p.file.u == 4); }
    for (int r : {0, -3}) { in.tv_rounds = r; in.tf_rounds = r; p = trio_plan(in); CHECK(p.visit.rounds == 1 && p.file.rounds == 1); }
    in.tv_rounds = 3; in.tf_rounds = 5;
    p = trio_plan(in);
    CHECK(p.visit.rounds == 3 && p.file.rounds == 5);
    for (int u : {1, 2, 4}) { in.rows_u = u; CHECK(trio_plan(in).rows.u == (uint32_t)u); }
    for (int u : {3, 0, 8}) { in.rows_u = u; CHECK(trio_plan(in).rows.u == 1); }
    for (int s : {128, 256, 512}) { in.tb_slots = s; CHECK(trio_plan(in).tb_slots == s); }
    for (int s : {100, 0, 1024}) { in.tb_slots = s; CHECK(trio_plan(in).tb_slots == 256); }
    CHECK(trio_plan(in).with_keys);
    in.with_keys = false;
    CHECK(!trio_plan(in).with_keys);
}

static void grids() {
    // visit and file kernel: a workgroup takes 4 * u * rounds groups
    for (int xcd = 0; xcd < 2; ++xcd) {
        TrioPlanIn in = narrow_db();
        in.trio_xcd = xcd;
        in.tv_u = 2; in.tv_rounds = 3; in.tf_u = 8; in.tf_rounds = 2;
        const uint32_t per_v = 4 * 2 * 3, per_f = 4 * 8 * 2;
        const struct { uint32_t ng, chunks_v, chunks_f; } t[] = {{1, 1, 1}, {per_v, 1, 1}, {per_v + 1, 2, 1}, {per_f, 3, 1}, {per_f + 1, 3, 2}, {9 * per_f, 24, 9}};
        for (const auto &c : t) {
            in.n_vgroups = c.ng;
            const TrioPlan p = trio_plan(in);
            CHECK(p.visit.chunks == c.chunks_v && p.file.chunks == c.chunks_f);
            if (xcd) {      // a multiple of eight workgroups, and the kernel is told how many hold groups
                CHECK(p.visit.grid == (c.chunks_v + 7) / 8 * 8 && p.visit.xcd_chunks == c.chunks_v);
                CHECK(p.file.grid == (c.chunks_f + 7) / 8 * 8 && p.file.xcd_chunks == c.chunks_f);
            } else {
                CHECK(p.visit.grid == c.chunks_v && p.visit.xcd_chunks == 0 && p.file.grid == c.chunks_f && p.file.xcd_chunks == 0);
            }
        }
    }
    {   // trio_xcd bit 1 alone does not touch them
        TrioPlanIn in = narrow_db();
        in.trio_xcd = 2;
        CHECK(trio_plan(in).visit.xcd_chunks == 0 && trio_plan(in).visit.grid == trio_plan(in).visit.chunks);
    }
    {   // rows kernel, first build: 64 chunks of 32 * u groups per workgroup, no XCD chunking whatever the option says
        TrioPlanIn in = narrow_db();
        in.trio_xcd = 3; in.n_vgroups = 32 * 64 + 1;
        TrioPlan p = trio_plan(in);
        CHECK(p.first_build && p.rows.u == 1 && p.rows.rchunks == 65 && p.rows.iters == 64 && !p.rows.rxcd && p.rows.grid == 2 && p.rows.xcd_chunks == 0);
        in.n_vgroups = 32 * 64;
        p = trio_plan(in);
        CHECK(p.rows.rchunks == 64 && p.rows.grid == 1);
        in.rows_u = 4; in.n_vgroups = 129;
        p = trio_plan(in);
        CHECK(p.rows.rchunks == 2 && p.rows.grid == 1 && p.rows.iters == 64);
    }
    {   // rows kernel on a rebuild (trio_two_pass): one chunk per workgroup, XCD chunking under bit 1
        TrioPlanIn in = narrow_db_built();
        in.trio_two_pass = true; in.n_vgroups = in.gprefix_for = 32 * 9 + 1;
        in.trio_xcd = 2;
        TrioPlan p = trio_plan(in);
        CHECK(!p.first_build && p.run_rows && p.rows.rchunks == 10 && p.rows.iters == 1 && p.rows.rxcd && p.rows.grid == 16 && p.rows.xcd_chunks == 10);
        in.trio_xcd = 1;
        p = trio_plan(in);
        CHECK(!p.rows.rxcd && p.rows.grid == 10 && p.rows.xcd_chunks == 0 && p.rows.iters == 1);
        in.trio_xcd = 3; in.rows_u = 2;
        p = trio_plan(in);
        CHECK(p.rows.rxcd && p.rows.rchunks == 5 && p.rows.grid == 8 && p.rows.xcd_chunks == 5);
    }
}

static void block_table() {
    using U64s = std::vector<uint64_t>;
    using U8s = std::vector<uint8_t>;
    const uint64_t big = 1ull << 27;
    {   // every species goes through the visit table: ok, zero blocks
        const TrioBlockTable t = trio_block_table(U64s{0, 100, 300, 301}, U8s{0, 0, 0});
        CHECK(t.ok && t.n_blocks == 0 && t.blk_base == std::vector<uint32_t>({0, 0, 0, 0}));
    }
    {   // blocks of 64 nodes for the slow species only; the last block of a species is short
        const TrioBlockTable t = trio_block_table(U64s{0, 64, 64 + 65, 64 + 65 + 1000, 64 + 65 + 1000 + 1}, U8s{1, 1, 0, 1});
        CHECK(t.ok && t.n_blocks == 4 && t.blk_base == std::vector<uint32_t>({0, 1, 3, 3, 4}));
    }
    {   // 2^27 - 1 nodes fit the packed key, 2^27 do not
        TrioBlockTable t = trio_block_table(U64s{0, 10, 10 + big - 1}, U8s{0, 1});
        CHECK(t.ok && t.n_blocks == (1u << 21) && t.blk_base[1] == 0);
        t = trio_block_table(U64s{0, 10, 10 + big}, U8s{0, 1});
        CHECK(!t.ok && t.n_blocks == 0);
        t = trio_block_table(U64s{0, 10, 10 + big}, U8s{1, 0});          // that large but not slow: no blocks for it
        CHECK(t.ok && t.n_blocks == 1);
        t = trio_block_table(U64s{0, 10 + 4 * big, 20 + 4 * big}, U8s{0, 0});
        CHECK(t.ok && t.n_blocks == 0);
    }
    {   // 2^31 - 1 blocks and more: not ok.  1024 species of 2^27 - 64 nodes have 2^31 - 1024 blocks; a species of 1022 * 64 nodes more is the most that fits
        U64s off{0};
        for (int s = 0; s < 1024; ++s) off.push_back(off.back() + big - 64);
        U8s slow(1024, 1);
        TrioBlockTable t = trio_block_table(off, slow);
        CHECK(t.ok && t.n_blocks == 0x80000000u - 1024u);
        off.push_back(off.back() + 1022 * 64); slow.push_back(1);
        t = trio_block_table(off, slow);
        CHECK(t.ok && t.n_blocks == 0x7FFFFFFEu);
        off.back() += 1;                                                 // one node more: one block more, 2^31 - 1
        t = trio_block_table(off, slow);
        CHECK(!t.ok);
    }
    {   // no species
        const TrioBlockTable t = trio_block_table(U64s{0}, U8s{});
        CHECK(t.ok && t.n_blocks == 0 && t.blk_base.size() == 1);
    }
}

static bool chunk_is(const TrioVisitChunk &c, uint32_t first, uint32_t end, uint32_t base, uint32_t species) {
    return c.first == first && c.end == end && c.base == base && c.species == species;
}
static void visit_chunks() {
    static_assert(sizeof(TrioVisitChunk) == 16, "four words");
    const std::vector<uint64_t> off{0, 1, 257, 514, 600};            // species of 1, 256, 257 and 86 nodes
    std::vector<TrioVisitChunk> c = trio_visit_chunks(off, {0, 0, 0, 0}, false);
    CHECK(c.size() == 5);
    CHECK(chunk_is(c[0], 0, 1, 0, 0) && chunk_is(c[1], 1, 257, 1, 1) && chunk_is(c[2], 257, 513, 257, 2) && chunk_is(c[3], 513, 514, 257, 2));
    CHECK(chunk_is(c[4], 514, 600, 514, 3));
    c = trio_visit_chunks(off, {0, 1, 0, 7}, false);                 // the slow species have none
    CHECK(c.size() == 3 && chunk_is(c[0], 0, 1, 0, 0) && chunk_is(c[1], 257, 513, 257, 2) && chunk_is(c[2], 513, 514, 257, 2));
    CHECK(trio_visit_chunks(off, {0, 0, 0, 0}, true).empty());       // force_block: every species is the node-block kernel's
    CHECK(trio_visit_chunks(off, {1, 1, 1, 1}, false).empty());
    CHECK(trio_visit_chunks({0}, {}, false).empty());
    CHECK(trio_visit_chunks({0, 0, 5}, {0, 0}, false).size() == 1);  // a species without nodes
}

int main() {
    routes();
    buckets();
    empty_db();
    shapes();
    grids();
    block_table();
    visit_chunks();
    std::printf("trio_plan_check: ok\n");
    return 0;
}
