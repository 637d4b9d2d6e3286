// cov_plan.hpp -- the host-side decisions of the coverage pass (a8) as pure functions of plain values: which of its three kernels a pass launches and in
// which shape (cov_plan), which work items a db of SOME of the species launches (cov_item_select), where the result arena keeps its parts
// (cov_arena_layout), and whether a graph counts its covered bases by the long-node scheme (long_node_shape).  coverage_launch and coverage_prepare
// (stage_cov.hip) follow them; nothing else decodes a shape code or picks a kernel.  Standard headers only: tests/native/cov_plan_check.cpp compiles
// this with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ptx {

// coverage_fast_kernel<.., U, PASSES, WIN>: groups in flight per wave, rounds per workgroup, nodes in the LDS window
struct CovFastShape { int u, passes, win; };
// coverage_fast_kernel<.., U, 1, WIN, LONG> over plain cuts of the stream: groups per workgroup, nodes the window begins in front of the first live step
struct CovLongShape { int u, win; uint32_t chunk_groups, win_back; };
// coverage_step_kernel<.., U, PASSES>
struct CovStepShape { int u, passes; };

struct CovPlan {
    bool run_fast = false, run_long = false, run_step = false;
    CovFastShape fast{2, 4, 2048};
    CovLongShape lng{2, 3072, 8, 0};
    CovStepShape step{1, 4};
    bool only_long = true;     // long / step kernel: groups without a step of a walk of more than 64 steps are the short-read kernel's (false: cov_general, every group)
    uint32_t xcd_map = 0;      // step kernel: every XCD walks one contiguous eighth of the stream
};

// Shape codes (options covf_shape, covl_shape, cov_shape; measurements and tests).  An unknown code decodes to the shape named last in each table.
//   fast: <U><PASSES><window / 1024>, or <U><PASSES><window / 256 as two digits - 70> for windows between 2048 and 3072 nodes
//   long: four digits <U><G><W><B> or five <U><GG><W><B>: G * 8 groups per workgroup (at least 8), a window of W * 1024 nodes that begins B * 256 nodes
//         in front of the first live step
//   step: <U><PASSES>
CovFastShape cov_fast_shape(int code);
CovLongShape cov_long_shape(int code);
CovStepShape cov_step_shape(int code);
constexpr int COVF_SHAPE_DEFAULT = 2423, COVF_SHAPE_DEFAULT_BIG = 2823;   // the second on streams of 2^28 steps and more
constexpr int COVL_SHAPE_DEFAULT = 2834;                                  // 2 groups in flight, 64 groups per workgroup, 3072-node window, 1024 nodes back
constexpr int COVS_SHAPE_DEFAULT = 14, COVS_SHAPE_DEFAULT_BIG = 18;       // the second on streams of 2^25 steps and more

// Which kernels a coverage pass over these reads launches.  T_pad: steps of the padded stream; n_long / n_slots: walks of more than 64 steps / all walks
// that own a slot; n_items: work items of the short-read kernel; R: reads.  Shape options <= 0: the default.
CovPlan cov_plan(uint64_t T_pad, uint32_t n_long, uint32_t n_slots, uint32_t n_items, uint64_t R, bool cov_general, const std::string &cov_long,
                 int covf_shape, int covl_shape, int cov_shape, int cov_xcd);

// The work items of the short-read kernel that can hold reads of a db's species: item_block[i] is the node block (first node id >> blk_shift) of the first
// read of item i, ascending; range_start / range_end are the species' id ranges.  `sel` is the ascending list without duplicates, kept only where the
// indirection pays (sel.size() * 9/8 < items; otherwise empty, n_sel = every item, on = false).  on: the kernel takes the list -- also when it is empty
// (n_sel = 0: nothing to launch).
struct CovItemSel {
    uint32_t n_sel = 0;
    std::vector<uint32_t> sel;
    bool on = false;
};
CovItemSel cov_item_select(const std::vector<uint32_t> &item_block, int blk_shift, const std::vector<int64_t> &range_start, const std::vector<int64_t> &range_end);

// One arena, one memset: [bases V u64][trio_bases max(U, 1) u64][abort u64][bitmap words u32, 16-byte aligned][full-node flags: 1 bit per node, padded by
// the largest LDS window].  Byte offsets; U = 0 without the unique-trio table.
struct CovArenaLayout {
    uint64_t words, fwords, n_trio;     // u32 words of the bit vector / of the flags, u64 entries of trio_bases
    size_t off_trio, off_abort, off_bm, off_full, total;
};
CovArenaLayout cov_arena_layout(uint64_t V, uint64_t U, uint64_t L);

// long nodes on average (chunk graphs of single-genome species among them): covered bases are counted from a per-stretch prefix in LDS
// (popcount_long_kernel, node_cov_stats_kernel<.., LONGN>), and the fused node pass is closed to the db
inline bool long_node_shape(uint64_t L, uint64_t V, int ncs_prefix_min, bool ncs_no_prefix) {
    return V != 0 && L / V >= (uint64_t)ncs_prefix_min && !ncs_no_prefix;
}

}  // namespace ptx
