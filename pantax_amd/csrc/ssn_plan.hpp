// ssn_plan.hpp -- the host-side decisions of the node-order row sort (sample_sort_nodes.hip) as one pure function of plain values: how many
// partition workgroups a segment gets and how many tiles each walks, the grid of the tie fills, and where every region of the sort's u32
// workspace lies.  sample_sort_nodes_ws_elems() sizes the workspace by this plan and sample_sort_nodes() binds its pointers from the same one;
// nothing else spells the layout.  The constants the host shares with the kernels (ssn_device.hpp) are here as well.  Standard headers only:
// tests/native/ssn_plan_check.cpp compiles this with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ptx {

#ifndef SN_LEVELS
#define SN_LEVELS 10                             // levels of the splitter tree (-DSN_LEVELS=9: measurements)
#endif
constexpr int SN_SAMPLE = 4096;
constexpr int SN_NLEAF = 1 << SN_LEVELS;         // 1024
constexpr int SN_NBUCKET = 2 * SN_NLEAF;         // 2048 ids (the last odd one stays empty)
#ifndef SN_ITEMS_N
#define SN_ITEMS_N 8
#endif
constexpr int SN_ITEMS = SN_ITEMS_N;                      // nodes per thread and tile
constexpr int SN_TILE = 256 * SN_ITEMS;
constexpr uint32_t SN_TARGET_WGS = 8192;         // workgroups of the two partition kernels over all segments
constexpr uint32_t SN_TIE_ROWS = 8192;           // consecutive output rows of a segment that one workgroup of ssn_ties_kernel fills
#ifndef SN_HEAD_PAIRS
#define SN_HEAD_PAIRS 64                          // bucket pairs a wave of ssn_heads_kernel looks at (round 6: 16 and 4 measured slower or equal)
#endif
constexpr int SN_HP = SN_HEAD_PAIRS, SN_NWH = SN_NLEAF / SN_HP;   // ... and the waves per segment
constexpr bool SSN_TIES_ASYNC_AUTO = false;      // option ssn_ties_async = -1 (ssn_ties_async() below).  Off: at cfg4 the step gained 0.13 .. 0.2 ms, but in the plain bench
                                                 // series the ranges of the runs with and without it overlap; not measured on the smaller workloads
constexpr uint64_t SSN_MAX_SEG = 1ull << 26;   // nodes of one segment (buckets grow with the segment: beyond 4096 rows they are sorted through memory)

// per-segment workspace (u32 words), SN_WS_WORDS apart (a multiple of four: the tree's 16-byte nodes stay aligned)
constexpr size_t SN_OFF_FLAGS = 0;                                  // [0] small segment, [1] #buckets left to the workgroup-wide sort, [2] # left to the second wave kernel, [3] rows
constexpr size_t SN_OFF_TREE = 4;                                   // {m, a} [SN_NLEAF], node k's children 2k and 2k+1 (node 0 unused)
constexpr size_t SN_OFF_SAMP = SN_OFF_TREE + 4 * SN_NLEAF;          // u64 [2][4096]
constexpr size_t SN_OFF_START = SN_OFF_SAMP + 2 * 2 * SN_SAMPLE;    // [SN_NBUCKET + 1]
constexpr size_t SN_OFF_MED = SN_OFF_START + SN_NBUCKET + 4;        // [SN_NBUCKET] buckets the first wave kernel leaves to the second
constexpr size_t SN_OFF_BIG = SN_OFF_MED + SN_NBUCKET;              // [SN_NBUCKET] buckets of more than SN_WAVE_CAP2 rows
constexpr size_t SN_WS_WORDS = SN_OFF_BIG + SN_NBUCKET;
static_assert(SN_WS_WORDS % 4 == 0, "16-byte tree nodes");

constexpr size_t SN_NODE_PARTIAL_WORDS = 8;     // u32 words of a NodePartial (primitives.hpp; ssn_device.hpp asserts it)

// The workspace, in u32 words from its base.  The base is at least 16-byte aligned (every DevBuf allocation is): the per-segment blocks and the
// count matrix are read in 16-byte steps, and the two regions of 8-byte elements (c0p, npart) start at EVEN word offsets -- alignment is decided
// here, not by looking at a pointer.
struct SsnPlan {
    uint32_t G = 1, per = 1;     // partition workgroups per segment, tiles each of them walks: G * per >= the tiles of the largest segment
    uint32_t tie_grid = 1;       // grid.x of ssn_ties_kernel: SN_TIE_ROWS rows of the largest segment each
    size_t ws = 0;               // [S][SN_WS_WORDS] flags, splitter tree, samples, bucket starts, the two bucket lists
    size_t cntm = 0;             // [S x G][SN_NBUCKET] count matrix
    size_t stage_cnt = 0;        // [S x G] rows a partition workgroup staged
    size_t c0p = 0;              // [S x G] double (even)
    size_t seg_n = 0;            // [S]
    size_t seg_out = 0;          // [S + 1]
    size_t sub_k = 0;            // [S][SN_NWH] patterns found by each wave of ssn_heads_kernel
    size_t ids = 0;              // [V] u16 bucket ids of the staged rows
    size_t npart = 0;            // [S x G] NodePartial (even)
    size_t total_words = 0;
};
SsnPlan ssn_plan(uint32_t S, uint64_t seg_bound, uint64_t V);

// Which rows of the sort's output get their key words (Sn::keys_all), from option ssn_keys and whether the sort forms the pattern tables itself.  With the
// tables the rows' keys have one reader, ssn_heads_kernel, which looks at the mixed bucket pairs only (sn_pair_mixed) and the step keeps the abundances
// alone; without them (pantax_hip_sort_rows) the keys ARE the result.  1: all, 0: the needed ones, -1: an unknown value, or "needed" without the tables.
int ssn_keys_all(const char *option, bool has_patterns);
// Where node_rows_kernel takes a node's bit-vector words from (options node_bits, node_bits_words): 0 every node gathers them ("gather"), 1 / 2 an item's
// stretch of the bit vector is loaded whole, that many words a lane ("" / "range"; words 0 = the default, SSN_NODE_BITS_WORDS).  -1: an unknown value.
constexpr int SSN_NODE_BITS_WORDS = 2;
int ssn_node_bits(const char *option, int words);
// The tie fill on the side stream (option ssn_ties_async; -1 = what the measurements of DESIGN.md section 4 decided).  Never while every launch is being
// clocked (a bracket on the side stream would time the overlap, and the per-kernel table wants the fill's own time), and never from the side stream itself.
bool ssn_ties_async(int option, bool clocked, bool on_side_stream, bool have_side_stream);

}  // namespace ptx
