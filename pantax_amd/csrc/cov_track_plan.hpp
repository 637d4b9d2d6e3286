// cov_track_plan.hpp -- the host side that the windowed passes along selected walks share (stage_cov_track.hip, stage_growth.hip): the tiles of the
// selected walks, the length pass over them and the host scan of its sums, up to the accumulation kernel of the caller.  Include from .hip files only.
#pragma once
#include <vector>
#include "common.hpp"
#include "cov_track_tile.hpp"

namespace ptx {

// what cov_track_plan (stage_cov_track.hip) leaves for the accumulation kernel of its caller: the tiles and their output records on the device, and on
// the host the first tile of every selection entry (tile_first [C+1])
struct CtPlan {
    uint32_t n_tiles = 0;
    std::vector<uint64_t> tile_first;
    DevBuf<CtTile> d_tiles;
    DevBuf<CtTileOut> d_touts;   // filled only when the windows fit the caller's cap
};
int cov_track_plan(Ctx *ctx, Db *db, const char *who, const uint64_t *sel_off, const uint32_t *sel_hap, uint64_t W, uint64_t *win_off_out, uint64_t cap, CtPlan &pl);

}  // namespace ptx
