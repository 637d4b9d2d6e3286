// cov_device.hpp -- what the kernels of the coverage pass share (stage_cov.hip, stage_cov_step.hip) and what the upload-time read layout
// (stage_read_layout.hip) writes for them: the LDS windows, the step codes of the grouped stream, the votes, the full-node flags.
#pragma once
#include "common.hpp"
#include "wave.hpp"

namespace ptx {

constexpr int COV_BLOCK = 256;

// The test-before-set must see other CUs' ORs to be worth anything: the ORs execute below the
// per-CU L1 (which is never refreshed by them), so the probe is an agent-scope load (sc1: L1
// bypass, served by L2).  A stale 0 only costs a redundant OR; bits never clear, so it is safe.
__device__ __forceinline__ uint32_t bm_peek(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Bits [g0,g1) of the coverage bit vector are marked through the workgroup's LDS bit window (words
// [bw0, bw0 + COV_BWIN) of the global vector); words outside the window take the global test-then-OR path.  The window is ORed into memory once per workgroup.
constexpr uint32_t COV_BWIN = 2048;   // 32-bit words: 64 kbit of graph bases
constexpr int COV_WIN = 2048;         // nodes in the LDS window of `bases` (a multiple of 64 nodes from a multiple of 64: the full-node flags flush as ballots);
                                      // 2048 steps of 1e7 reads over 3.2e7 nodes span ~1000 nodes: 1024 overflowed on most chunks
// the LDS windows of the coverage kernel live at file scope: helpers that received them as (generic) pointer arguments
// made this compiler emit an illegal null check of the shared-memory aperture
// One dynamic LDS block per workgroup: [WIN u32 `bases` window][COV_BWIN u32 bit window][WIN u8 full-node flags: a step covered the
// whole node, its bits are not marked one by one (popcount_kernel takes the length)].  WIN is a launch parameter of the
// short-read kernel (a multiple of 256 nodes) and COV_WIN in the general one; helpers address the block by offsets.
extern __shared__ uint32_t s_cov[];
#define S_WIN(i) s_cov[(i)]
#define S_BM(bmo, i) s_cov[(bmo) + (i)]
#define S_FULL(bmo, i) reinterpret_cast<uint8_t *>(s_cov + (bmo) + COV_BWIN)[(i)]
__host__ __device__ constexpr size_t cov_lds_bytes(int win) { return (size_t)win * 4 + COV_BWIN * 4 + (size_t)win; }
__device__ __forceinline__ void lds_or(uint32_t *__restrict__ bm, uint32_t bmo, uint64_t bw0, uint32_t bwn, uint64_t w, uint32_t m) {
    const uint64_t off = w - bw0;     // unsigned wrap: words below the window are out of range too
    if (off < bwn) {
        if ((S_BM(bmo, off) & m) != m) atomicOr(&S_BM(bmo, off), m);
    } else if ((bm_peek(&bm[w]) & m) != m) atomicOr(&bm[w], m);
}
__device__ __forceinline__ void mark_range(uint32_t *__restrict__ bm, uint32_t bmo, uint64_t bw0, uint32_t bwn, uint64_t g0, uint64_t g1) {
    if (g1 <= g0) return;
    uint64_t w0 = g0 >> 5, w1 = (g1 - 1) >> 5;
    uint32_t m0 = 0xFFFFFFFFu << (g0 & 31);
    uint32_t m1 = 0xFFFFFFFFu >> (31 - (uint32_t)((g1 - 1) & 31));
    if (w0 == w1) lds_or(bm, bmo, bw0, bwn, w0, m0 & m1);
    else {
        lds_or(bm, bmo, bw0, bwn, w0, m0);
        for (uint64_t w = w0 + 1; w < w1; ++w) lds_or(bm, bmo, bw0, bwn, w, 0xFFFFFFFFu);
        lds_or(bm, bmo, bw0, bwn, w1, m1);
    }
}
// the same for a range that lies inside the LDS bit window: 32-bit positions relative to the window, LDS only
__device__ __forceinline__ void win_or(uint32_t bmo, uint32_t w, uint32_t m) { if ((S_BM(bmo, w) & m) != m) atomicOr(&S_BM(bmo, w), m); }
__device__ __forceinline__ void mark_window(uint32_t bmo, uint32_t r0, uint32_t r1) {
    if (r1 <= r0) return;
    const uint32_t w0 = r0 >> 5, w1 = (r1 - 1) >> 5;
    const uint32_t m0 = 0xFFFFFFFFu << (r0 & 31), m1 = 0xFFFFFFFFu >> (31 - ((r1 - 1) & 31));
    if (w0 == w1) win_or(bmo, w0, m0 & m1);
    else {
        win_or(bmo, w0, m0);
        for (uint32_t w = w0 + 1; w < w1; ++w) win_or(bmo, w, 0xFFFFFFFFu);
        win_or(bmo, w1, m1);
    }
}

// Step codes (g_step_dup): walks of <= 64 steps carry the distance back to the first occurrence of the step's node in
// the walk (0 = none); longer walks carry STEP_LONG | (1 if the node occurred earlier in the walk).  Where the first
// occurrence sits matters only through "is it step 0" (profile.rs:853-856 vs :860-862), i.e. id == id of step 0.
constexpr uint32_t STEP_LONG = 0x80u;
// ... and, both kinds, STEP_START on the first step of a walk; pad steps carry STEP_PAD.  The slots of the grouped copy follow
// the stream (build_step_read lays the walks out in slot order), so a step's slot is not stored per step: group_slot[g] names
// the read that owns the first step of the 64-step group g, and every later walk start in the group advances it by one.
constexpr uint32_t STEP_START = 0x40u, STEP_PAD = 0xFFu, STEP_DIST = 0x3Fu;
// ballots / votes of a bool WITHOUT the detour through an int predicate (__ballot(int) costs a v_cndmask + v_cmp per call: the kernel is bound by VALU issue)
__device__ __forceinline__ unsigned long long ballot1(bool b) { return __builtin_amdgcn_ballot_w64(b); }
__device__ __forceinline__ bool any1(bool b) { return __builtin_amdgcn_ballot_w64(b) != 0ull; }
__device__ __forceinline__ bool none1(bool b) { return __builtin_amdgcn_ballot_w64(b) == 0ull; }
__device__ __forceinline__ uint32_t slot_in_group(uint32_t group_first_slot, uint32_t code, int lane) {
    const unsigned long long starts = ballot1((code != STEP_PAD) & ((code & STEP_START) != 0u)) & ~1ull;   // lane 0's walk is group_first_slot itself
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(starts >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)starts, 0u));   // starts in lower lanes
    return group_first_slot + below + (uint32_t)((starts >> lane) & 1ull);
}

// read_nodes_len of position j (never the last position) of a long walk: the length aligned at the node's FIRST
// occurrence in the read (profile.rs:879-882)
__device__ __forceinline__ uint32_t rl_from_memory(uint32_t j, uint32_t b, const uint32_t *__restrict__ node_id, const uint8_t *__restrict__ step_dup,
                                                   uint32_t delta, const uint4 *__restrict__ node_rec, uint32_t len0, uint32_t ps) {
    const uint32_t idj = node_id[b + j];
    if (j == 0 || ((step_dup[b + j] & 1u) && idj == node_id[b])) return len0 - ps;
    return node_rec[idj + delta].z;
}

// -DCOV_ABLATE builds (never the product library: make OUT=../lib_prof EXTRA=-DCOV_ABLATE, loaded through PANTAX_HIP_LIB) read
// PANTAX_COV_ABLATE: bit 0 no bit / flag marking, bit 1 no `bases`, bit 2 no unique-trio lookups -- wrong results, for timing only
#ifdef COV_ABLATE
#define ABL(bit) (ablate & (bit))
#else
#define ABL(bit) false
#endif
constexpr int COV_WIN_BACK = 128; // window starts (at least) this many nodes before the node of the chunk's first live step
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;

__device__ __forceinline__ void add_bases(unsigned long long *__restrict__ bases, uint32_t wlo, uint32_t win_n, uint32_t v, uint32_t aln) {
    const uint32_t off = v - wlo;   // unsigned wrap puts nodes below the window out of range too
    if (off < win_n && aln < (1u << 18)) atomicAdd(&S_WIN(off), aln);   // <= 8192 steps x 2^18 < 2^32
    else atomicAdd(&bases[v], (unsigned long long)aln);
}
// The full-node flag of node v (v = NO_FULL: none) -- called by ALL 64 lanes of a wave.  Inside the LDS window: plain byte stores of the
// same value (no atomic, nothing to lose).  Outside: the steps of a long walk are neighbouring nodes, so dozens of lanes would OR
// into the SAME 32-bit word -- memory-side atomics on one address run one after the other (1.0 of the kernel's 2.6 ms at cfg5's share);
// the lanes of one word combine their bits first (DPP reduction) and the first of them issues ONE atomic per distinct word.
constexpr uint32_t NO_FULL = 0xFFFFFFFFu;
__device__ __forceinline__ void mark_full_wave(uint32_t *__restrict__ full, uint32_t wlo, uint32_t win_n, uint32_t v) {
    const uint32_t off = v - wlo;
    const bool have = v != NO_FULL;
    if (have && off < win_n) S_FULL(COV_WIN, off) = 1;
    const bool out = have && off >= win_n;
    unsigned long long todo = __ballot(out);
    const uint32_t w = v >> 5, bit = 1u << (v & 31);
    const int lane = threadIdx.x & 63;
    while (todo) {                                 // (wave-uniform) one round per distinct word: two to four for a stretch of a walk
        const int leader = __builtin_ctzll(todo);
        const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane((int)w, leader);
        const bool mine = out && w == wl;
        const uint32_t orv = wave_reduce(mine ? bit : 0u, [](uint32_t x, uint32_t y) { return x | y; });
        if (lane == leader) atomicOr(&full[wl], orv);   // no test-before-set: the probe is a dependent round trip, the OR is fire-and-forget
        todo &= ~__ballot(mine);
    }
}

// Work items of the short-read kernel (build_step_read cuts them, coverage_fast_kernel takes one per workgroup): up to COV_ITEM_GROUPS consecutive groups
// whose reads all start inside one block of 2^COV_BLK_SHIFT node ids.
constexpr uint32_t COV_ITEM_GROUPS = 128;     // (64 until the end of round 5: a block of 2048 ids holds ~80 groups at 1e8 reads, cut as 64 + 17; whole blocks as ONE item: 5.2 -> 5.0 ms)
struct __attribute__((packed, aligned(4))) EntPair { uint32_t a, b, c, d; };     // two neighbouring lookup entries {smaller end, larger end}
constexpr int COV_BLK_SHIFT = 11;

template <int WIN>
__device__ __forceinline__ void mark_full_out_wave(uint32_t *__restrict__ full, bool out, uint32_t v) {
    // the steps of a long walk are neighbouring nodes: dozens of lanes would OR into the SAME word, and memory-side atomics on one address run one
    // after the other -- the lanes of a word combine their bits first and ONE of them issues the atomic (wave-uniform loop, called by all 64 lanes)
    unsigned long long todo = ballot1(out);
    const uint32_t w = v >> 5, bit = 1u << (v & 31);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane((int)w, leader);
        const bool mine = out & (w == wl);
        const uint32_t orv = wave_reduce(mine ? bit : 0u, [](uint32_t x, uint32_t y) { return x | y; });
        if (lane == leader) atomicOr(&full[wl], orv);
        todo &= ~ballot1(mine);
    }
}

}  // namespace ptx
