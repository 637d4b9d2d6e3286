// trio_plan.hpp -- the host-side decisions of the unique-trio index (a7) as pure functions of plain values: which route a build takes, which of its
// brackets run and in which shape (trio_plan), which node blocks the species left to the node-block kernel get (trio_block_table) and which 256-node
// chunks the visit table is packed by (trio_visit_chunks).  trio_index_build (stage_trio.hip) and the two upload-time builders
// (stage_trio_tables.hip) follow them; nothing else decodes a trio option or spells a route predicate.  Standard headers only:
// tests/native/trio_plan_check.cpp compiles this with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ptx {

constexpr int TRIO_BLK_SHIFT = 6, TRIO_BLK = 1 << TRIO_BLK_SHIFT;   // nodes per block of the node-block kernel
constexpr int VIS_CHUNK_SHIFT = 8;                                  // nodes per layout chunk of the visit table (a chunk starts on a group border)

struct TrioPlanIn {
    uint64_t P = 0, V = 0;                       // path steps, nodes
    uint32_t H = 0, S = 0;
    uint32_t n_vgroups = 0, n_blocks = 0;        // groups of the visit table, blocks of the node-block kernel
    uint64_t n_win = 0;                          // windows of the db: read on the bucket path only (the caller counts them only for a plan that says buckets)
    bool trio_visit_ok = false, trio_block_ok = false;
    bool trio_sizes_known = false, trio_layout_fast = false;
    bool have_gprefix = false;                   // the groups' first rows of an earlier build are there ...
    uint32_t gprefix_for = 0;                    // ... for this many groups
    bool with_keys = true;
    // options
    std::string trio_path, trio_rows;
    bool trio_two_pass = false, flag_rank_chained = false;
    int uniq_hash = -1;
    int tv_u = 4, tv_rounds = 4, tf_u = 8, tf_rounds = 1, rows_u = 1, tb_slots = 256, trio_xcd = 3;
};

// trio_visit_kernel<U, ..> / trio_file_kernel<U, ..>: every wave takes u x rounds consecutive groups, a workgroup (four waves) one chunk
struct TrioGroupGrid {
    uint32_t u = 4, rounds = 1;
    uint32_t chunks = 0;         // workgroups that have groups
    uint32_t grid = 0;           // workgroups launched: `chunks`, rounded up to eight where the XCDs take contiguous eighths
    uint32_t xcd_chunks = 0;     // the kernel's argument: `chunks` under XCD chunking, else 0
};
// trio_rows_kernel<.., .., U>: a wave takes u batches of eight groups; a first build's workgroup takes `iters` chunks (one set of LDS counters)
struct TrioRowsGrid {
    uint32_t u = 1, rchunks = 0, iters = 1, grid = 0, xcd_chunks = 0;
    bool rxcd = false;
};
// One arena for what the path route needs cleared: uniq bits (one per path position) | first_cnt [| cnt | cursor]; offsets and sizes in u32 words.
// cnt / cursor belong to the bucket path, which clears all of it (`clear` = zwords); the other builds clear the bits alone.
struct TrioArena {
    size_t zbits = 0, zwords = 0, clear = 0;
    size_t off_uniq_q = 0, off_first_cnt = 0, off_cnt = 0, off_cursor = 0;
};
enum class TrioPrefix { none, tiles, chained };              // the groups' first rows: three plain launches, or one chained scan (flag_rank_chained)
enum class TrioHeadScan { none, trio_first, slow_first };    // the nodes' first rows on the path route: every node, or (mixed) the node-block species behind the fast rows

struct TrioPlan {
    // the route
    bool by_block = false;        // uniqueness by visit table / node block (false: global buckets for the whole db)
    bool rows_by_visit = false;   // the visit table's species are filed from the visit kernel's records (fast route)
    bool path_route = false;      // some (or all) rows are filed by the pass over the walks
    bool mixed = false;           // both: the path route's rows follow the fast route's
    bool first_build = false;     // sizes, rows per haplotype and the statistics' chunk table are (re)learnt
    bool fused = false;           // a rebuild that decides and files the visit table's species in one pass
    // the brackets
    bool run_file = false, run_visit = false, run_block = false, run_bucket = false;
    bool run_uniq = false, uniq_hashed = false;        // bucket path: there are windows to test; through the LDS hash table
    TrioPrefix prefix = TrioPrefix::none;
    bool run_rows = false;
    TrioHeadScan head_scan = TrioHeadScan::none;
    bool release_records = false; // first build: later builds file in one pass and need neither the records nor the groups' ballots
    // the shapes, normalised: u in {2, 4, 8}, rounds >= 1, rows.u in {1, 2, 4}, tb_slots in {128, 256, 512}
    TrioGroupGrid visit, file;
    TrioRowsGrid rows;
    int tb_slots = 256;
    bool with_keys = true;
    uint64_t n_win = 0;
    TrioArena arena;
};
TrioPlan trio_plan(const TrioPlanIn &in);

// Blocks of TRIO_BLK consecutive local node ids for the species the visit table leaves to the node-block kernel (slow[s] != 0); node_off: [S + 1].
// ok = false: the db keeps the bucket path (a species of >= 2^27 nodes among them -- the packed LDS key holds 27-bit local ids -- or 2^31 - 1
// blocks and more).  ok with n_blocks == 0: every species goes through the visit table.
struct TrioBlockTable {
    bool ok = false;
    uint32_t n_blocks = 0;
    std::vector<uint32_t> blk_base;      // [S + 1] first block of every species
};
TrioBlockTable trio_block_table(const std::vector<uint64_t> &node_off, const std::vector<uint8_t> &slow);

// The 256-node chunks of the species the visit table covers (slow[s] == 0; none under force_block), in species order
struct TrioVisitChunk { uint32_t first, end, base, species; };   // {first node, end node, node base of the species, species}
std::vector<TrioVisitChunk> trio_visit_chunks(const std::vector<uint64_t> &node_off, const std::vector<uint32_t> &slow, bool force_block);

}  // namespace ptx
