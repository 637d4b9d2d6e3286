// member_device.hpp -- what the .hip files of the strain reports share beside the plan (member_plan.hpp): the compact node masks of route 2 and, on the
// device, a node's row in them and the four-sum accumulator of the node evidence and near-miss kernels.  How a kernel consumes its words is its own design
// and stays in its file.  Include from .hip files only.
#pragma once
#include "common.hpp"
#include "member_plan.hpp"
#include "wave.hpp"

namespace ptx {

// Route 2: node membership in chosen walks as a compact arena -- member_words(K) words per node of a species over its K chosen haplotypes only (bit k = the
// k-th of them), filled by read_strain_mask_kernel (walk_masks.hip).  Its eight users: read_strains_launch and read_support_launch (through rs_table_build),
// evidence_launch, depth_launch, near_miss_launch (over Sel ++ Cand), hap_pairs_launch, fit_launch, growth_launch.  The object owns the device buffers: it outlives the kernels that read d_mask.
constexpr uint64_t WALK_MASK_TILE = 4096;   // walk positions per tile of the mask pass (one wave)
struct WalkMaskTile { uint64_t p0, p1, word0; uint32_t nw, k; };   // walk positions [p0, p1) of chosen walk k; its words start at word0 (+ local node * nw)
struct WalkMasks {
    std::vector<WalkMaskTile> tiles;
    uint64_t words = 0;
    DevBuf<WalkMaskTile> d_tiles;
    DevBuf<unsigned long long> d_mask;
    MemberRow row(const Db *db, uint32_t s, bool by_node, const uint32_t *haps, uint64_t K);   // member_row of species s; on route 2 its masks join the arena
    uint64_t add_species(const Db *db, uint32_t s, const uint32_t *haps, uint64_t K);          // -> first word of the species' node masks
    int build(Ctx *ctx, const Db *db);   // after the last row / add_species: zero fill + the pass over the tiles, on ctx->stream
};
// What the launchers of the five node passes (evidence, depth, near miss, hap pairs, fit) hold on the device around their kernel: the masks, and one output block [a | b]
struct MemberPass {
    WalkMasks wm;
    DevBuf<unsigned long long> d_out;
    int open(Ctx *ctx, const Db *db, size_t n);                                   // d_out: n words, zero-filled; the masks built
    int close(Ctx *ctx, uint64_t *a, size_t n_a, uint64_t *b, size_t n_b);        // behind the kernel: the block's two parts -> the host arrays, then the stream's end
};
// first mask word of global node v of the row's species (the row by value: by reference the node kernels' register allocation comes out differently)
__device__ __forceinline__ uint64_t member_mask_row(const MemberRow r, uint32_t v) { return r.mask_base + (uint64_t)(v - r.node_base) * r.nw; }

// The per-wave LDS counters of the evidence and fit node passes change hands between the wave's lanes (lane 0 adds, every lane zeroes and flushes its own
// bit): order the accesses inside the wave
__device__ __forceinline__ void member_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

struct MemberQ { unsigned long long n, len, cov, bases; };
__device__ __forceinline__ void mq_add(MemberQ &a, bool on, uint32_t len, uint32_t cov, unsigned long long bases) {
    a.n += on ? 1ull : 0ull; a.len += on ? (unsigned long long)len : 0ull; a.cov += on ? (unsigned long long)cov : 0ull; a.bases += on ? bases : 0ull;
}
__device__ __forceinline__ MemberQ mq_wave_sum(const MemberQ &a) {
    const auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
    return MemberQ{wave_reduce(a.n, add), wave_reduce(a.len, add), wave_reduce(a.cov, add), wave_reduce(a.bases, add)};
}
__device__ __forceinline__ void mq_flush(unsigned long long *__restrict__ dst, const MemberQ &a) {   // one 64-bit atomicAdd per non-zero sum
    if (a.n) atomicAdd(dst, a.n);
    if (a.len) atomicAdd(dst + 1, a.len);
    if (a.cov) atomicAdd(dst + 2, a.cov);
    if (a.bases) atomicAdd(dst + 3, a.bases);
}

}  // namespace ptx
