// walk_masks.hip -- the compact node masks of chosen walks (WalkMasks, member_device.hpp): the tile list and the pass over it.
#include <algorithm>
#include "member_device.hpp"
#include "primitives.hpp"

namespace ptx {

namespace {

// a wave per tile of one chosen walk; bit k of the walk's word on every node the stretch visits
__global__ void __launch_bounds__(256) read_strain_mask_kernel(uint32_t n_tiles, const WalkMaskTile *__restrict__ tiles, const uint32_t *__restrict__ path_nodes,
                                                               unsigned long long *__restrict__ mask) {
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * 4) {
        const WalkMaskTile tl = tiles[t];
        const unsigned long long bit = 1ull << (tl.k & 63u);
        const uint64_t wb = tl.word0 + (tl.k >> 6);
        for (uint64_t p = tl.p0 + (uint64_t)lane; p < tl.p1; p += 64) atomicOr(&mask[wb + (uint64_t)path_nodes[p] * tl.nw], bit);
    }
}

}  // namespace

MemberRow WalkMasks::row(const Db *db, uint32_t s, bool by_node, const uint32_t *haps, uint64_t K) {
    MemberRow r = member_row(by_node, db->h_hap_off[s + 1] - db->h_hap_off[s], (uint32_t)db->h_node_off[s], haps, K);
    if (r.route == 2u) r.mask_base = add_species(db, s, haps, K);
    return r;
}
// the words of every node of the species behind what the arena holds so far (bit k = the walk of haps[k]), and the tiles of those K walks ...
uint64_t WalkMasks::add_species(const Db *db, uint32_t s, const uint32_t *haps, uint64_t K) {
    const uint64_t base = words;
    const uint32_t nw = (uint32_t)member_words(K);
    words += (db->h_node_off[s + 1] - db->h_node_off[s]) * nw;
    for (uint64_t k = 0; k < K; ++k) {
        const uint64_t h = db->h_hap_off[s] + haps[k];
        for (uint64_t p = db->h_path_off[h]; p < db->h_path_off[h + 1]; p += WALK_MASK_TILE)
            tiles.push_back(WalkMaskTile{p, std::min(p + WALK_MASK_TILE, db->h_path_off[h + 1]), base, nw, (uint32_t)k});
    }
    return base;
}
// ... and the pass over them: the arena zero-filled, then one 64-bit atomic OR per visit (the result does not depend on their order)
int WalkMasks::build(Ctx *ctx, const Db *db) {
    PTX_HIP(ctx, d_mask.alloc(words ? words : 1));
    if (words) PTX_TRY(zero_fill(ctx, d_mask.p, words * sizeof(unsigned long long)));
    if (tiles.empty()) return 0;
    if (tiles.size() >= 0xFFFFFFFFull) return fail(ctx, PANTAX_HIP_E_LIMIT, "walk masks: %llu tiles of selected walks exceed 32-bit positions", (unsigned long long)tiles.size());
    PTX_TRY(upload(ctx, d_tiles, tiles.data(), tiles.size()));
    KTimer tm(ctx, "read_strain_mask_kernel");
    hipLaunchKernelGGL(read_strain_mask_kernel, dim3(grid_for(tiles.size(), 4, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, (uint32_t)tiles.size(), d_tiles.p,
                       db->d_path_nodes.p, d_mask.p);
    return 0;
}

int MemberPass::open(Ctx *ctx, const Db *db, size_t n) {
    PTX_HIP(ctx, d_out.alloc(n));
    PTX_TRY(zero_fill(ctx, d_out.p, n * sizeof(unsigned long long)));
    return wm.build(ctx, db);
}
int MemberPass::close(Ctx *ctx, uint64_t *a, size_t n_a, uint64_t *b, size_t n_b) {
    PTX_HIP(ctx, hipGetLastError());
    if (n_a) PTX_TRY(download(ctx, (unsigned long long *)a, d_out.p, n_a));
    if (n_b) PTX_TRY(download(ctx, (unsigned long long *)b, d_out.p + n_a, n_b));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host arrays are filled, the caller's temporaries are released on its return
    return 0;
}

}  // namespace ptx
