// stage_read_layout.hip -- the upload-time layout of resident reads: the locus-grouped, wave-padded copy of the walks with its step codes, slot records
// and work items (build_step_read, reads_group).  A function of the reads alone: it runs at upload, never in a step.
#include <algorithm>
#include <atomic>
#include <vector>
#include "common.hpp"
#include "primitives.hpp"
#include "wave.hpp"
#include "cov_device.hpp"

namespace ptx {

// ---------------------------------------------------------------------------------------------
// Resident layout of the packed reads: grouped by the locus of their first node and padded so that
// a walk of <= 64 steps never straddles a 64-step boundary.  Key = first node id >> shift (ids are
// globally ordered by species and position, sort_range.rs:25-33).  Counting sort of the reads into
// slots (histogram -> scan -> scatter), then one thread per bucket lays its walks out (start moved to
// the next multiple of 64 when the walk would straddle one; bucket sizes rounded up to 64), a scan of
// the bucket sizes, and the fill.  Done once per upload: it depends on the reads only, not on the
// binning.  Slot order inside a bucket is arbitrary; every output of the path is an order-independent
// integer sum, so results stay bit-exact.  Reads with an empty walk own no slot (profile.rs:794-796).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) group_count_kernel(uint64_t R, const uint32_t *__restrict__ step_off, const uint32_t *__restrict__ node_id,
                                                          int shift, uint32_t *__restrict__ cnt_r) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 256) {
        const uint32_t b = step_off[r], k = step_off[r + 1] - b;
        if (k) atomicAdd(&cnt_r[node_id[b] >> shift], 1u);
    }
}
__global__ void __launch_bounds__(256) group_slot_kernel(uint64_t R, const uint32_t *__restrict__ step_off, const uint32_t *__restrict__ node_id,
                                                         const uint32_t *__restrict__ pstart, const uint32_t *__restrict__ pend, const uint32_t *__restrict__ qlen,
                                                         const uint8_t *__restrict__ mapq, int shift, const uint32_t *__restrict__ base_r, uint32_t *__restrict__ cur_r,
                                                         uint32_t *__restrict__ slot_of, uint4 *__restrict__ g_read_rec, uint2 *__restrict__ g_qm,
                                                         uint32_t *__restrict__ n_long) {
    // The per-read columns are read HERE, in file order (coalesced), and leave as the slot's two records -- {first step of the walk in
    // the source columns (group_fill_kernel replaces it by the walk's place in the grouped stream), #steps, pstart, pend} and {read
    // length, MAPQ}: the fill pass then reads one coalesced record per slot.  (Round 3 kept {#steps, read} per slot and let the fill
    // pass gather six columns at random: 46 GB fetched for 4 GB of payload at 1e8 reads.)
    uint32_t mine = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (uint64_t)gridDim.x * 256) {
        const uint32_t b = step_off[r], k = step_off[r + 1] - b;
        uint32_t slot = NO_SLOT;
        if (k) {
            const uint32_t key = node_id[b] >> shift;
            slot = base_r[key] + atomicAdd(&cur_r[key], 1u);
            g_read_rec[slot] = make_uint4(b, k, pstart[r], pend[r]);
            g_qm[slot] = make_uint2(qlen[r], (uint32_t)mapq[r]);    // slot-order copies for the binning pass
            mine += k > 64 ? 1u : 0u;
        }
        slot_of[r] = slot;
    }
    if (__any(mine != 0)) {
        mine = wave_reduce(mine, [](uint32_t x, uint32_t y) { return x + y; });
        if ((threadIdx.x & 63) == 0) atomicAdd(n_long, mine);
    }
}
// One thread lays out a UNIT of 2^g consecutive buckets; only units are rounded up to 64 steps.  (Rounding every 32-node
// bucket cost 32 pad steps per bucket on average: with ten reads per bucket -- 1e7 reads over 3.2e7 nodes -- the padded
// stream was 1.45 x the walk steps, and the coverage kernel spends a lane on every pad.)
// A thread lays out ONE unit (its reads one after the other: a walk of <= 64 steps never straddles a 64-step border).  A workgroup of 64 threads takes 64
// consecutive units -- their reads are one stretch of slots --, loads the reads' step counts into LDS coalesced, lets every thread walk its unit there,
// and writes the places back coalesced.  (The first version had every thread read its reads' 16-byte records from memory, far from its neighbours':
// 10.7 GB of sector traffic for 1.6 GB of records at 1e8 reads, 4.8 ms.)  A stretch of more reads than the LDS holds takes the plain loop.
constexpr uint32_t GL_UNITS = 64, GL_CAP = 24576;
__global__ void __launch_bounds__(64) group_layout_kernel(uint32_t NB, int g, const uint32_t *__restrict__ base_r /*[NB+1]*/,
                                                          const uint4 *__restrict__ g_read_rec, uint32_t *__restrict__ slot_rel,
                                                          uint32_t *__restrict__ size_s) {
    __shared__ uint32_t s_k[GL_CAP];
    const uint32_t NU = (NB + (1u << g) - 1) >> g;
    const uint32_t u0 = blockIdx.x * GL_UNITS, key = u0 + threadIdx.x;
    const uint32_t kb = min(NB, u0 << g), ke = min(NB, (u0 + GL_UNITS) << g);
    const uint32_t s_begin = base_r[kb], n_wg = base_r[ke] - s_begin;                    // (workgroup-uniform)
    const bool staged = n_wg <= GL_CAP;
    if (staged) {
        for (uint32_t i = threadIdx.x; i < n_wg; i += GL_UNITS) s_k[i] = g_read_rec[s_begin + i].y;
        __syncthreads();
    }
    if (key < NU) {
        const uint32_t k0 = key << g, k1 = min(NB, (key + 1) << g);
        uint32_t pos = 0;
        for (uint32_t s = base_r[k0], e = base_r[k1]; s < e; ++s) {
            const uint32_t k = staged ? s_k[s - s_begin] : g_read_rec[s].y;
            if (k <= 64 && (pos & 63) + k > 64) pos = (pos + 63) & ~63u;
            if (staged) s_k[s - s_begin] = pos; else slot_rel[s] = pos;
            pos += k;
        }
        size_s[key] = (pos + 63) & ~63u;
    }
    if (staged) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_wg; i += GL_UNITS) slot_rel[s_begin + i] = s_k[i];
    }
}
// In SLOT order, one WAVE per 64 consecutive slots: the lanes first file their slot's records (coalesced), then hand the steps
// of the 64 walks out flat over the wave -- lane = step of the output stream, which the slots follow in order, so node ids and
// step codes are written as dense runs and the short source walks are gathered.  (Thread per read in file order scattered
// single dwords and bytes over the whole stream: 72 GB written for 4 GB of payload at 1e8 reads, 46 ms; thread per slot with
// a private loop over its steps still re-read every walk k times for the first-occurrence codes: 41 ms.)  The code of a step
// -- distance back to the first occurrence of its node in the walk -- comes from the lanes below (and, where a walk began in
// the round before, from that round's ids).
__global__ void __launch_bounds__(256) group_fill_kernel(uint32_t n_slots, const uint32_t *__restrict__ node_id, int shift,
                                                         const uint32_t *__restrict__ base_s, const uint32_t *__restrict__ slot_rel, uint4 *__restrict__ g_read_rec,
                                                         uint32_t *__restrict__ g_node_id, uint32_t *__restrict__ g_group_slot,
                                                         uint8_t *__restrict__ g_step_dup, uint2 *__restrict__ g_mm) {
    __shared__ uint32_t s_excl[4][65], s_b[4][64], s_sb[4][64];
    __shared__ uint2 s_mm[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n_waves = (n_slots + 63) / 64;
    for (uint32_t w = blockIdx.x * 4 + wave; w < n_waves; w += gridDim.x * 4) {
        const uint32_t slot = w * 64 + lane;
        uint32_t b = 0, k = 0, sb = 0;
        if (slot < n_slots) {
            uint4 rec = g_read_rec[slot];                            // {first step in the source columns, #steps, pstart, pend}: group_slot_kernel
            b = rec.x; k = rec.y;
            sb = base_s[node_id[b] >> shift] + slot_rel[slot];
            rec.x = sb;
            g_read_rec[slot] = rec;
            if (k > 64) { k = 0; s_mm[wave][lane] = make_uint2(0xFFFFFFFFu, 0u); }   // laid out by group_fill_long_kernel, one workgroup per walk (min / max: its atomics)
            else if ((sb & 63u) == 0u) g_group_slot[sb >> 6] = slot; // a walk of <= 64 steps lies inside one 64-step group
        }
        const uint32_t incl = wave_incl_scan_dpp(k);
        const uint32_t total = __shfl(incl, 63);
        s_excl[wave][lane] = incl - k; s_b[wave][lane] = b; s_sb[wave][lane] = sb;
        if (lane == 0) s_excl[wave][64] = total;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        uint32_t prev_id = 0;
        for (uint32_t f0 = 0; f0 < total; f0 += 64) {
            const uint32_t f = f0 + (uint32_t)lane;
            const bool on = f < total;
            uint32_t o = 0;                                          // owner: the last slot whose first flat step is <= f (walks of 0 steps own none)
            if (on) {
                uint32_t lo = 0, hi = 63;
                while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (s_excl[wave][mid] <= f) lo = mid; else hi = mid - 1; }
                o = lo;
            }
            const uint32_t i = on ? f - s_excl[wave][o] : 0u;
            const uint32_t id = on ? node_id[s_b[wave][o] + i] : 0u;
            // first occurrence of my node among the i earlier steps of my walk: they sit in the lanes below, or in the round before
            uint32_t dup = 0, mn = id, mx = id;                      // smallest / largest id of my walk up to my step: complete in the lane of its last step
            const uint32_t imax = wave_reduce(i, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
            for (uint32_t d = 1; d <= imax; ++d) {
                const uint32_t cur = __shfl(id, (lane - (int)d) & 63), old = __shfl(prev_id, (lane - (int)d) & 63);
                const uint32_t other = (int)d <= lane ? cur : old;
                if (d <= i && other == id) dup = d;                   // the largest such distance = the first occurrence
                const uint32_t mine = d <= i ? other : id;
                mn = min(mn, mine); mx = max(mx, mine);
            }
            if (on) {
                const uint32_t dst = s_sb[wave][o] + i;
                g_node_id[dst] = id;
                g_step_dup[dst] = (uint8_t)(dup | (i == 0 ? STEP_START : 0u));
                if (i + 1 == s_excl[wave][o + 1] - s_excl[wave][o]) s_mm[wave][o] = make_uint2(mn, mx);   // the walk's last step (the owner of a flat step holds at least one)
            }
            prev_id = id;
        }
        // {min id, max id} of the 64 walks, one coalesced store (a slot holds a walk of at least one step: every row of s_mm was written)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        if (slot < n_slots) g_mm[slot] = s_mm[wave][lane];
        __builtin_amdgcn_wave_barrier();                             // the LDS rows are reused by this wave's next 64 slots
    }
}

// Walks of more than 64 steps: one workgroup copies the walk (coalesced) and decides for every step whether its node
// occurred earlier in the walk -- an LDS hash of (node id -> smallest position) for walks of up to LONG_HASH/2 steps,
// a plain scan of the earlier steps above that.  The copy loop, which every walk takes, also forms the walk's smallest and largest id
// for the binning pass (group_fill_kernel, which runs first, left the neutral pair in the slot's place): one atomic pair per wave.
constexpr uint32_t LONG_HASH = 8192;
__global__ void __launch_bounds__(256) group_fill_long_kernel(uint64_t R, const uint32_t *__restrict__ step_off, const uint32_t *__restrict__ node_id,
                                                              int shift, const uint32_t *__restrict__ base_s, const uint32_t *__restrict__ slot_of,
                                                              const uint32_t *__restrict__ slot_rel, uint32_t *__restrict__ g_node_id,
                                                              uint32_t *__restrict__ g_group_slot, uint8_t *__restrict__ g_step_dup,
                                                              uint2 *__restrict__ g_mm) {
    __shared__ uint32_t h_key[LONG_HASH], h_pos[LONG_HASH];
    constexpr uint32_t EMPTY = 0xFFFFFFFFu;
    for (uint64_t r = blockIdx.x; r < R; r += gridDim.x) {
        const uint32_t b = step_off[r], k = step_off[r + 1] - b;
        if (k <= 64) continue;
        const uint32_t slot = slot_of[r];
        const uint32_t sb = base_s[node_id[b] >> shift] + slot_rel[slot];
        uint32_t mn = 0xFFFFFFFFu, mx = 0;
        for (uint32_t i = threadIdx.x; i < k; i += 256) {
            const uint32_t id = node_id[b + i];
            g_node_id[sb + i] = id;
            mn = min(mn, id); mx = max(mx, id);
            if (((sb + i) & 63u) == 0u) g_group_slot[(sb + i) >> 6] = slot;   // every group this walk's steps begin
        }
        mn = wave_reduce(mn, [](uint32_t x, uint32_t y) { return x < y ? x : y; });
        mx = wave_reduce(mx, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
        if ((threadIdx.x & 63) == 0) {
            uint32_t *mm = reinterpret_cast<uint32_t *>(g_mm + slot);
            atomicMin(mm, mn); atomicMax(mm + 1, mx);
        }
        if (k <= LONG_HASH / 2) {
            for (uint32_t i = threadIdx.x; i < LONG_HASH; i += 256) { h_key[i] = EMPTY; h_pos[i] = EMPTY; }
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < k; i += 256) {
                const uint32_t id = node_id[b + i];
                uint32_t h = (id * 2654435761u) >> 19;             // 13 bits
                for (;;) {
                    const uint32_t old = atomicCAS(&h_key[h], EMPTY, id);
                    if (old == EMPTY || old == id) { atomicMin(&h_pos[h], i); break; }
                    h = (h + 1) & (LONG_HASH - 1);
                }
            }
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < k; i += 256) {
                const uint32_t id = node_id[b + i];
                uint32_t h = (id * 2654435761u) >> 19;
                while (h_key[h] != id) h = (h + 1) & (LONG_HASH - 1);
                g_step_dup[sb + i] = (uint8_t)(STEP_LONG | (h_pos[h] < i ? 1u : 0u) | (i == 0 ? STEP_START : 0u));
            }
            __syncthreads();
        } else {
            for (uint32_t i = threadIdx.x; i < k; i += 256) {
                const uint32_t id = node_id[b + i];
                uint32_t dup = 0;
                for (uint32_t j = 0; j < i; ++j) if (node_id[b + j] == id) { dup = 1; break; }
                g_step_dup[sb + i] = (uint8_t)(STEP_LONG | dup | (i == 0 ? STEP_START : 0u));
            }
        }
    }
}

// first group of every node block: the smallest group whose first step is the first step of a read that starts in the block (a group
// that continues a longer walk, or holds only pads, starts no read)
__global__ void __launch_bounds__(256) group_block_kernel(uint32_t n_groups, const uint32_t *__restrict__ group_slot, const uint32_t *__restrict__ g_node_id,
                                                          const uint8_t *__restrict__ step_code, int bshift, uint32_t *__restrict__ first_g) {
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < n_groups; g += gridDim.x * 256) {
        if (group_slot[g] == NO_SLOT) continue;
        const uint32_t code = step_code[(uint64_t)g * 64];
        if (code == STEP_PAD || !(code & STEP_START)) continue;
        atomicMin(&first_g[g_node_id[(uint64_t)g * 64] >> bshift], g);
    }
}

static int step_read_layout(Ctx *ctx, Reads *rd, uint32_t max_node_id) {
    static std::atomic<uint64_t> next_layout{1};
    rd->layout_id = next_layout.fetch_add(1);       // (what a db's list of work items is made for)
    rd->T_pad = 0;
    rd->n_long = 0;
    rd->n_slots = 0;
    rd->n_items = 0;
    PTX_HIP(ctx, rd->d_slot_of.alloc(rd->R ? rd->R : 1));
    PTX_HIP(ctx, rd->d_g_slot_rec.alloc(rd->R ? rd->R : 1));
    PTX_HIP(ctx, rd->d_g_qm.alloc(rd->R ? rd->R : 1));
    PTX_HIP(ctx, rd->d_g_mm.alloc(rd->R ? rd->R : 1));
    if (rd->R == 0) return 0;
    if (rd->T == 0) {
        PTX_HIP(ctx, hipMemsetAsync(rd->d_slot_of.p, 0xFF, rd->R * sizeof(uint32_t), ctx->stream));
        return 0;
    }
    int shift = 5;
    // buckets of 32 node ids up to 5e8 ids (round 4; 2^20 buckets before: 512-id buckets at 3e8 ids, whose reads are in no particular order --
    // the coverage pass gathers node records along the stream, and neighbours in the stream should be neighbours in the graph)
    int bucket_cap_bits = 24;
    if (ctx->cfg.group_bucket_bits) bucket_cap_bits = std::max(10, std::min(26, ctx->cfg.group_bucket_bits));
    while (((uint64_t)max_node_id >> shift) + 1 > (1ull << bucket_cap_bits)) ++shift;
    const uint32_t NB = (uint32_t)(max_node_id >> shift) + 1;
    DevBuf<uint32_t> cnt, scan_tmp, slot_rel;
    PTX_HIP(ctx, cnt.alloc(4ull * (NB + 1) + 8));
    uint32_t *cnt_r = cnt.p, *base_r = cnt_r + (NB + 1), *size_s = base_r + (NB + 1), *base_s = size_s + (NB + 1);
    PTX_HIP(ctx, scan_tmp.alloc(scan_tmp_elems(NB + 1)));
    PTX_HIP(ctx, slot_rel.alloc(rd->R));
    PTX_HIP(ctx, rd->d_g_read_rec.alloc(rd->R));
    PTX_TRY(zero_fill(ctx, cnt_r, (NB + 1) * sizeof(uint32_t)));
    int gridR = grid_for(rd->R, 256, ctx->n_cu * 8);
    hipLaunchKernelGGL(group_count_kernel, dim3(gridR), dim3(256), 0, ctx->stream, rd->R, rd->d_step_off.p, rd->d_node_id.p, shift, cnt_r);
    PTX_TRY(exclusive_scan_u32(ctx, cnt_r, base_r, NB + 1, scan_tmp.p, nullptr));
    PTX_TRY(zero_fill(ctx, cnt_r, (NB + 1) * sizeof(uint32_t)));   // reused as cursors
    uint32_t *d_total = (uint32_t *)ctx->d_scalars.p, *d_n_long = d_total + 1;
    PTX_HIP(ctx, hipMemsetAsync(d_n_long, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(group_slot_kernel, dim3(gridR), dim3(256), 0, ctx->stream, rd->R, rd->d_step_off.p, rd->d_node_id.p, rd->d_pstart.p, rd->d_pend.p,
                       rd->d_qlen.p, rd->d_mapq.p, shift, base_r, cnt_r, rd->d_slot_of.p, rd->d_g_read_rec.p, rd->d_g_qm.p, d_n_long);
    // layout units: 2^g buckets each, about 2048 walk steps per unit (the rounding of a unit to 64 steps then costs ~1.5 %)
    int g = 0;
    while (g < 12 && ((double)rd->T / (double)NB) * (double)(1u << g) < 2048.0) ++g;
    const uint32_t NU = (NB + (1u << g) - 1) >> g;
    hipLaunchKernelGGL(group_layout_kernel, dim3((NU + GL_UNITS - 1) / GL_UNITS), dim3(GL_UNITS), 0, ctx->stream, NB, g, base_r, rd->d_g_read_rec.p, slot_rel.p, size_s);
    PTX_TRY(exclusive_scan_u32(ctx, size_s, base_s, NU, scan_tmp.p, d_total));
    const int ushift = shift + g;   // unit of a read = its first node id >> ushift
    uint32_t h_tot[2] = {0, 0}, h_slots = 0;
    PTX_TRY(download(ctx, h_tot, d_total, 2));
    PTX_TRY(download(ctx, &h_slots, base_r + NB, 1));   // reads that own a slot (non-empty walk)
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t h_total = h_tot[0];
    rd->n_long = h_tot[1];
    rd->n_slots = h_slots;
    if ((uint64_t)h_total < rd->T) return fail(ctx, PANTAX_HIP_E_LIMIT, "reads_upload: padded step stream exceeds 32-bit positions");
    rd->T_pad = h_total;
    PTX_HIP(ctx, rd->d_g_node_id.alloc(rd->T_pad)); PTX_HIP(ctx, rd->d_g_group_slot.alloc(rd->T_pad / 64 + 1)); PTX_HIP(ctx, rd->d_g_step_dup.alloc(rd->T_pad));
    PTX_TRY(byte_fill(ctx, rd->d_g_node_id.p, 0, rd->T_pad * sizeof(uint32_t)));
    PTX_TRY(byte_fill(ctx, rd->d_g_group_slot.p, 0xFF, (rd->T_pad / 64 + 1) * sizeof(uint32_t)));
    PTX_TRY(byte_fill(ctx, rd->d_g_step_dup.p, 0xFF, rd->T_pad));                                            // STEP_PAD
    if (rd->n_slots)
        hipLaunchKernelGGL(group_fill_kernel, dim3(grid_for(rd->n_slots, 256, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, rd->n_slots, rd->d_node_id.p, ushift,
                           base_s, slot_rel.p, rd->d_g_read_rec.p, rd->d_g_node_id.p, rd->d_g_group_slot.p, rd->d_g_step_dup.p, rd->d_g_mm.p);
    if (rd->n_long) {
        const uint32_t gridL = (uint32_t)std::min<uint64_t>(rd->R, (uint64_t)ctx->n_cu * 64);
        hipLaunchKernelGGL(group_fill_long_kernel, dim3(gridL), dim3(256), 0, ctx->stream, rd->R, rd->d_step_off.p, rd->d_node_id.p, ushift, base_s,
                           rd->d_slot_of.p, slot_rel.p, rd->d_g_node_id.p, rd->d_g_group_slot.p, rd->d_g_step_dup.p, rd->d_g_mm.p);
        PTX_HIP(ctx, rd->d_long_sum.alloc(rd->R));
        PTX_HIP(ctx, rd->d_long_len0.alloc(rd->R));
    }
    PTX_HIP(ctx, hipGetLastError());
    // work items of the short-read coverage kernel: the groups cut at the borders of 2048-id node blocks (the stream is in the order of
    // the reads' first nodes, bucket by bucket), a block's groups cut into items of COV_ITEM_GROUPS
    {
        const uint32_t n_groups = (uint32_t)(rd->T_pad / 64);
        const int bshift = std::max(COV_BLK_SHIFT, shift);
        const uint32_t NBLK = (uint32_t)(max_node_id >> bshift) + 1;
        DevBuf<uint32_t> first_g;
        PTX_HIP(ctx, first_g.alloc(NBLK + 1));
        PTX_HIP(ctx, hipMemsetAsync(first_g.p, 0xFF, ((size_t)NBLK + 1) * sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(group_block_kernel, dim3(grid_for(n_groups, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, n_groups, rd->d_g_group_slot.p, rd->d_g_node_id.p,
                           rd->d_g_step_dup.p, bshift, first_g.p);
        std::vector<uint32_t> fg((size_t)NBLK + 1);
        PTX_TRY(download(ctx, fg.data(), first_g.p, (size_t)NBLK + 1));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        fg[NBLK] = n_groups;
        bool monotone = true;
        for (uint32_t b = NBLK; b-- > 0;) { if (fg[b] == 0xFFFFFFFFu) fg[b] = fg[b + 1]; else if (fg[b] > fg[b + 1]) monotone = false; }
        fg[0] = 0;                                                  // groups in front of the first live one (pads) belong to the first block
        std::vector<uint2> items;
        rd->h_item_block.clear();
        // at most 256 groups: the LDS `bases` window sums an item's 32-bit lengths, 256 x 64 steps x (2^18 - 1) < 2^32 (S_WIN in coverage_fast_kernel, stage_cov.hip)
        const uint32_t cap = ctx->cfg.cov_item_groups > 0 ? (uint32_t)std::min(ctx->cfg.cov_item_groups, 256) : COV_ITEM_GROUPS;
        if (monotone)
            for (uint32_t b = 0; b < NBLK; ++b)
            {   // a block's groups in EQUAL items of at most `cap` groups (81 groups: 41 + 40, not 64 + 17 -- a workgroup zeroes and flushes its LDS windows once per item)
                const uint32_t n = fg[b + 1] - fg[b];
                if (!n) continue;
                const uint32_t k = (n + cap - 1) / cap, per = (n + k - 1) / k;
                for (uint32_t g = fg[b]; g < fg[b + 1]; g += per) { items.push_back(make_uint2(g, std::min(fg[b + 1], g + per))); rd->h_item_block.push_back(b); }
            }
        else   // cannot happen with the counting sort above; never silent: plain cuts of the stream
            for (uint32_t g = 0; g < n_groups; g += COV_ITEM_GROUPS) items.push_back(make_uint2(g, std::min(n_groups, g + COV_ITEM_GROUPS)));
        rd->n_items = (uint32_t)items.size();
        rd->item_blk_shift = monotone ? bshift : 0;
        PTX_TRY(upload(ctx, rd->d_g_items, items.data(), items.size()));
    }
    PTX_HIP(ctx, hipGetLastError());
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // temporaries are released on return
    return 0;
}

// "grouped" holds only from the finished build on; the build voids the binning (the species of a read now live in its slot record: the next binning pass
// writes them), the file-order species array and the slot-order flags
int build_step_read(Ctx *ctx, Reads *rd, uint32_t max_node_id) {
    rd->state.layout_begun();
    PTX_TRY(step_read_layout(ctx, rd, max_node_id));
    rd->state.layout_finished();
    return 0;
}

int reads_group(Ctx *ctx, Reads *rd) {
    if (rd->state.grouped()) return 0;
    return build_step_read(ctx, rd, rd->max_node_id);
}

}  // namespace ptx
