// stage_trio_tables.hip -- the upload-time layout tables of the unique-trio index (a7): the visit table (trio_visits_build) and the node-block run
// table (trio_runs_build).  Both are functions of the graphs alone, built once at the end of db upload like the tile table; which species go where
// (trio_visit_chunks, trio_block_table) is trio_plan.hpp's.
#include <algorithm>
#include <cstdlib>
#include "trio_device.hpp"

namespace ptx {

// ---- the visit table (upload time; a function of the graphs alone) ----
// interior visits per node (a position with a neighbour on either side inside its walk is the middle of one window)
__global__ void __launch_bounds__(256) visit_count_kernel(TRIO_GRAPH_ARGS, uint32_t *__restrict__ cnt) {
    TILE_LOOP(q, h, qend) {
        if (q > path_off[h] && q + 1 < qend) atomicAdd(&cnt[node_base[hap_species[h]] + path_nodes[q]], 1u);
    }
}
// visited[v] = the node has a visit (its count is stored by every build; the others read as zero), slow[s] = the species holds a
// node with more than VIS_MAX visits
__global__ void __launch_bounds__(256) visit_flags_kernel(uint64_t V, uint32_t S, const uint32_t *__restrict__ node_base, const uint32_t *__restrict__ cnt,
                                                          uint32_t *__restrict__ visited, uint32_t *__restrict__ slow) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = v < V ? cnt[v] : 0u;
    const unsigned long long bal = __ballot(c != 0u);
    if ((threadIdx.x & 31) == 0 && v < V + 32) visited[v >> 5] = (uint32_t)(bal >> (threadIdx.x & 32));
    if (c > (uint32_t)VIS_MAX) {
        uint32_t lo = 0, hi = S;                                             // last s with node_base[s] <= v
        while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)node_base[mid] <= v) lo = mid; else hi = mid; }
        slow[lo] = 1u;
    }
}
// one thread packs the nodes of a chunk {first node, end node, node base of the species, species} into groups of 64 visits that no node
// straddles: FIRST FIT over a few open groups (round 5; rounds 4's next-fit closed a group as soon as the next node did not fit -- one
// 50-visit node per group at fifty strains per species, 22 % pads; 7 % at ten).  The order of the nodes inside a chunk is then the order of
// their placement, not of their ids: nothing depends on it (a node's visits stay one stretch of one group, its rows one block).
constexpr int VIS_OPEN = 4;
struct VisPack {
    uint32_t fill[VIS_OPEN], gidx[VIS_OPEN], n_groups;
    unsigned long long heads[VIS_OPEN];                  // head lanes of the open groups (bit = a node's first visit)
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < VIS_OPEN; ++j) { fill[j] = 64u; gidx[j] = 0xFFFFFFFFu; heads[j] = 0ull; }
        n_groups = 0u;
    }
    // -> slot of the node's first visit, relative to the chunk's first group.  A group that is closed to make room is handed to `closed`
    // (group index relative to the chunk, its head mask): a group belongs to ONE chunk, so its mask is a plain store of the packing thread
    template <class Closed>
    __device__ __forceinline__ uint32_t place(uint32_t k, Closed &&closed) {
        int best = -1;
#pragma unroll
        for (int j = VIS_OPEN - 1; j >= 0; --j) if (fill[j] + k <= 64u) best = j;       // the first open group it fits
        if (best < 0) {                                                                 // none: the fullest one is closed, a new group opened in its place
            best = 0;
#pragma unroll
            for (int j = 1; j < VIS_OPEN; ++j) if (fill[j] > fill[best]) best = j;
#pragma unroll
            for (int j = 0; j < VIS_OPEN; ++j) if (j == best) { if (gidx[j] != 0xFFFFFFFFu) closed(gidx[j], heads[j]); fill[j] = 0u; gidx[j] = n_groups; heads[j] = 0ull; }
            ++n_groups;
        }
        uint32_t slot = 0;
#pragma unroll
        for (int j = 0; j < VIS_OPEN; ++j) if (j == best) { slot = gidx[j] * 64u + fill[j]; heads[j] |= 1ull << fill[j]; fill[j] += k; }
        return slot;
    }
    template <class Closed>
    __device__ __forceinline__ void finish(Closed &&closed) {
#pragma unroll
        for (int j = 0; j < VIS_OPEN; ++j) if (gidx[j] != 0xFFFFFFFFu) closed(gidx[j], heads[j]);
    }
};
// PLACE = false: the number of groups every chunk needs (-> scan -> first group of every chunk); PLACE = true: the nodes' slots, the groups' head
// masks / node bases / species.  A workgroup of 64 threads takes 64 consecutive chunks: the wave loads their nodes' counts into LDS (coalesced; a
// count of the visit table's species is at most 64: a byte), every thread then packs ITS chunk from LDS, and the wave writes the slots back
// coalesced.  (Round 4-5's first version had every thread read its chunk's counts from memory, 1 KB apart from its neighbour's: 81 + 37 GB of
// sector traffic for 1.3 GB of counts at 1e4 strains, 22 + 4.5 ms.)
constexpr int VP_CHUNKS = 64, VP_CNT_STRIDE = 260 /* bytes */, VP_SLOT_STRIDE = 258 /* u16: 129 words -> the threads' rows start on different banks */;
template <bool PLACE>
__global__ void __launch_bounds__(64) visit_pack_kernel(uint32_t NC, const uint4 *__restrict__ chunks, const uint32_t *__restrict__ cnt, uint32_t *__restrict__ chunk_groups,
                                                        const uint32_t *__restrict__ chunk_gbase, uint32_t *__restrict__ vslot, unsigned long long *__restrict__ head,
                                                        uint32_t *__restrict__ gnbase, uint32_t *__restrict__ gsp) {
    __shared__ uint8_t s_cnt[VP_CHUNKS * VP_CNT_STRIDE];
    __shared__ uint16_t s_slot[PLACE ? VP_CHUNKS * VP_SLOT_STRIDE : 1];
    const uint32_t c0 = blockIdx.x * VP_CHUNKS, lane = threadIdx.x;
    const uint32_t nj = min((uint32_t)VP_CHUNKS, NC - c0);
    for (uint32_t j = 0; j < nj; ++j) {
        const uint4 ch = chunks[c0 + j];                                         // (workgroup-uniform)
        for (uint32_t i = lane; i < ch.y - ch.x; i += 64) s_cnt[j * VP_CNT_STRIDE + i] = (uint8_t)min(cnt[ch.x + i], 255u);
    }
    __syncthreads();
    {
        uint32_t n = 0;
        if (lane < nj) { const uint4 ch = chunks[c0 + lane]; n = ch.y - ch.x; }
        VisPack pk;
        pk.init();
        // a group's head mask: one plain 8-byte store by the packing thread when the group is closed (the first version issued one memory-side
        // atomicOr per NODE: 3.2e8 at 1e4 strains, 15 of the kernel's 17 ms)
        const uint32_t gb = (PLACE && lane < nj) ? chunk_gbase[c0 + lane] : 0u;
        auto closed = [&](uint32_t g, unsigned long long m) { if (PLACE) head[gb + g] = m; };
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t k = s_cnt[lane * VP_CNT_STRIDE + i];
            if (!k) continue;
            const uint32_t slot = pk.place(k, closed);                           // relative to the chunk's first group: below 256 groups x 64
            if (PLACE) s_slot[lane * VP_SLOT_STRIDE + i] = (uint16_t)slot;
        }
        pk.finish(closed);
        if (!PLACE) { if (lane < nj) chunk_groups[c0 + lane] = pk.n_groups; return; }
    }
    __syncthreads();
    for (uint32_t j = 0; j < nj; ++j) {
        const uint4 ch = chunks[c0 + j];
        const uint32_t gbase = chunk_gbase[c0 + j], base = gbase << 6, ng = chunk_gbase[c0 + j + 1] - gbase;
        for (uint32_t i = lane; i < ch.y - ch.x; i += 64)
            if (s_cnt[j * VP_CNT_STRIDE + i]) vslot[ch.x + i] = base + s_slot[j * VP_SLOT_STRIDE + i];
        for (uint32_t g = lane; g < ng; g += 64) { gnbase[gbase + g] = ch.z; gsp[gbase + g] = ch.w; }   // the chunk's groups: its species' node base / species
    }
}
__global__ void __launch_bounds__(256) visit_fill_kernel(TRIO_GRAPH_ARGS, const uint32_t *__restrict__ slow, const uint32_t *__restrict__ vslot,
                                                         uint32_t *__restrict__ cnt /* counted back down to zero */, uint32_t *__restrict__ vis_pos) {
    TILE_LOOP(q, h, qend) {
        const uint32_t sp = hap_species[h];
        if (slow[sp] || !(q > path_off[h] && q + 1 < qend)) continue;
        const uint32_t g = node_base[sp] + path_nodes[q];
        vis_pos[vslot[g] + atomicSub(&cnt[g], 1u) - 1u] = (uint32_t)q;
    }
}
// the visits of every node sorted by (smaller end, larger end, position) of their window (the fill's atomics left them in arrival
// order): equal windows become neighbours, which is what trio_visit_kernel's two-neighbour test relies on -- and checks -- and the
// table is the same on every upload.  One wave per group, ranks by shuffles inside the node's stretch.
__global__ void __launch_bounds__(256) visit_sort_kernel(uint32_t NG, uint32_t *__restrict__ vis_pos, const uint64_t *__restrict__ vis_head,
                                                         const uint32_t *__restrict__ path_nodes) {
    const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= NG) return;
    const int lane = threadIdx.x & 63;
    const uint32_t q = vis_pos[(uint64_t)g * 64 + lane];
    const bool valid = q != VIS_PAD;
    uint32_t lo = 0, hi = 0;
    if (valid) { const U32x3 w = *reinterpret_cast<const U32x3 *>(path_nodes + (q - 1u)); lo = min(w.x, w.z); hi = max(w.x, w.z); }
    const unsigned long long vmask = __ballot(valid), hd = vis_head[g] & vmask;
    const unsigned long long he = hd | (~vmask & (vmask + 1ull));
    const unsigned long long upto = hd & ((2ull << lane) - 1ull), above = he & ~((2ull << lane) - 1ull);
    const int start = upto ? 63 - __builtin_clzll(upto) : lane, end = above ? __builtin_ctzll(above) : 64;
    // LONG stretches (a node of dozens of visits: fifty strains per species): the ranks below cost a round per distance, 49 of them -- the whole wave
    // is sorted instead by (stretch, smaller end, larger end, position) in a bitonic network of 21 exchanges, pads (stretch 64) last: a lane's
    // sorted place IS its slot, because the stretches are the wave's lanes in order (115 -> 70 ms per db of 2.8e9 path steps)
    if (__builtin_amdgcn_ballot_w64(valid && end - start > 24) != 0ull) {
        uint32_t k0 = valid ? (uint32_t)start : 64u, k1 = lo, k2 = hi, k3 = q;
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const int partner = lane ^ j;
                const uint32_t p0 = __shfl(k0, partner), p1 = __shfl(k1, partner), p2 = __shfl(k2, partner), p3 = __shfl(k3, partner);
                const bool p_less = p0 < k0 || (p0 == k0 && (p1 < k1 || (p1 == k1 && (p2 < k2 || (p2 == k2 && p3 < k3)))));
                const bool keep_min = ((lane & k) == 0) == (lane < partner);     // ascending blocks keep the smaller key in the lower lane
                const bool take = keep_min ? p_less : !p_less;                   // (keys are distinct: positions differ; pads equal each other -- either stays)
                if (take && !(p0 == k0 && p1 == k1 && p2 == k2 && p3 == k3)) { k0 = p0; k1 = p1; k2 = p2; k3 = p3; }
            }
        if (k0 != 64u) vis_pos[(uint64_t)g * 64 + lane] = k3;
        return;
    }
    int rank = 0;
    // every pair of a stretch is compared ONCE, by its upper lane (positions are distinct: the order is total and strict); the lower lane reads the
    // outcome from the ballot -- three shuffles per distance instead of six (28.8 ms at 1e4 strains, 213 ms per db at fifty strains per species before)
    for (int d = 1; d < 64; ++d) {
        const bool dn = valid && lane - d >= start;
        if (!__any(dn)) break;
        const int ld = (lane - d) & 63;
        const uint32_t alo = __shfl(lo, ld), ahi = __shfl(hi, ld), aq = __shfl(q, ld);
        const bool below_first = alo < lo || (alo == lo && (ahi < hi || (ahi == hi && aq < q)));
        const unsigned long long mine_first = __ballot(dn && !below_first);      // bit l: lane l sorts before its partner l - d
        if (dn && below_first) ++rank;
        if (valid && lane + d < end && ((mine_first >> ((lane + d) & 63)) & 1ull)) ++rank;
    }
    if (valid) vis_pos[(uint64_t)g * 64 + start + rank] = q;   // every lane holds its value already: the stretch is rewritten in place
}

// The run table (upload time, depends on the graphs only): heads = positions whose node lies in another block than their
// predecessor's (or that start a walk); counted per block, scanned, then every head measures its run and files it.
__global__ void __launch_bounds__(256) run_count_kernel(TRIO_GRAPH_ARGS, const uint32_t *__restrict__ slow, const uint32_t *__restrict__ blk_base, uint32_t *__restrict__ blk_cnt) {
    TILE_LOOP(q, h, qend) {
        const uint32_t sp = hap_species[h], x = path_nodes[q];
        if (!slow[sp]) continue;                       // the visit table's species
        const bool head = q == path_off[h] || (path_nodes[q - 1] >> TRIO_BLK_SHIFT) != (x >> TRIO_BLK_SHIFT);
        if (head) atomicAdd(&blk_cnt[blk_base[sp] + (x >> TRIO_BLK_SHIFT)], 1u);
    }
}
__global__ void __launch_bounds__(256) run_fill_kernel(TRIO_GRAPH_ARGS, const uint32_t *__restrict__ slow, const uint32_t *__restrict__ blk_base, const uint32_t *__restrict__ blk_run_off,
                                                       uint32_t *__restrict__ cursor, uint4 *__restrict__ runs) {
    TILE_LOOP(q, h, qend) {
        const uint32_t sp = hap_species[h], x = path_nodes[q], bx = x >> TRIO_BLK_SHIFT;
        if (!slow[sp]) continue;
        const uint64_t qb = path_off[h];
        const bool head = q == qb || (path_nodes[q - 1] >> TRIO_BLK_SHIFT) != bx;
        if (!head) continue;
        uint64_t e = q + 1;
        while (e < qend && (path_nodes[e] >> TRIO_BLK_SHIFT) == bx) ++e;
        const uint32_t gb = blk_base[sp] + bx;
        runs[blk_run_off[gb] + atomicAdd(&cursor[gb], 1u)] = make_uint4((uint32_t)q, (uint32_t)(e - q), (uint32_t)qb, (uint32_t)qend);
    }
}

// The visit table (end of db upload).  Counting sort of the interior positions by their node: count -> which species stay
// with the node-block kernel -> greedy packing of every 256-node chunk into groups of 64 visits (one thread per chunk; a
// chunk starts on a group border, so the chunks pack independently) -> scan of the chunk sizes -> place -> fill -> sort.
int trio_visits_build(Ctx *ctx, Db *db) {
    db->trio_visit_ok = false;
    db->n_vgroups = 0;
    db->h_trio_slow.assign(db->S, 1);          // until shown otherwise every species is the node-block kernel's
    const bool force_block = ctx->cfg.trio_path == "block";   // every species through the node-block kernel (tests, measurements)
    PTX_HIP(ctx, db->d_trio_slow.alloc(db->S ? db->S : 1));
    PTX_HIP(ctx, hipMemsetAsync(db->d_trio_slow.p, 0, (db->S ? db->S : 1) * sizeof(uint32_t), ctx->stream));
    PTX_HIP(ctx, db->d_node_visited.alloc(db->V / 32 + 2));
    PTX_HIP(ctx, hipMemsetAsync(db->d_node_visited.p, 0, (db->V / 32 + 2) * sizeof(uint32_t), ctx->stream));
    auto all_slow = [&]() -> int {
        std::vector<uint32_t> ones(db->S ? db->S : 1, 1u);
        PTX_TRY(upload(ctx, db->d_trio_slow, ones.data(), ones.size()));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return 0;
    };
    if (db->P == 0 || db->P >= 0xFFFFFFFFull || db->V == 0 || db->S == 0) return all_slow();
    DevBuf<uint32_t> cnt, vslot, chunk_groups, chunk_gbase, scan_tmp, tot;
    PTX_HIP(ctx, cnt.alloc(db->V + 1));
    PTX_TRY(zero_fill(ctx, cnt.p, (db->V + 1) * sizeof(uint32_t)));
    const dim3 tgrid((uint32_t)db->n_tiles);
    hipLaunchKernelGGL(visit_count_kernel, tgrid, dim3(256), 0, ctx->stream, TRIO_GRAPH(db), cnt.p);
    hipLaunchKernelGGL(visit_flags_kernel, dim3((uint32_t)((db->V + 256) / 256)), dim3(256), 0, ctx->stream, db->V, db->S, db->d_node_base.p, cnt.p,
                       db->d_node_visited.p, db->d_trio_slow.p);
    std::vector<uint32_t> slow(db->S);
    PTX_TRY(download(ctx, slow.data(), db->d_trio_slow.p, db->S));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    static_assert(sizeof(TrioVisitChunk) == sizeof(uint4), "a chunk record is the uint4 visit_pack_kernel reads");
    const std::vector<TrioVisitChunk> chunks = trio_visit_chunks(db->h_node_off, slow, force_block);
    const uint32_t NC = (uint32_t)chunks.size();
    if (NC == 0) return all_slow();
    DevBuf<uint4> d_chunks;
    PTX_TRY(upload(ctx, d_chunks, reinterpret_cast<const uint4 *>(chunks.data()), chunks.size()));
    PTX_HIP(ctx, chunk_groups.alloc(NC + 1)); PTX_HIP(ctx, chunk_gbase.alloc(NC + 1));
    PTX_HIP(ctx, scan_tmp.alloc(scan_tmp_elems(NC + 1))); PTX_HIP(ctx, tot.alloc(1));
    PTX_HIP(ctx, hipMemsetAsync(chunk_groups.p + NC, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(visit_pack_kernel<false>, dim3((NC + VP_CHUNKS - 1) / VP_CHUNKS), dim3(64), 0, ctx->stream, NC, d_chunks.p, cnt.p, chunk_groups.p, (const uint32_t *)nullptr,
                       (uint32_t *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr);
    PTX_TRY(exclusive_scan_u32(ctx, chunk_groups.p, chunk_gbase.p, (uint64_t)NC + 1, scan_tmp.p, tot.p));
    uint32_t NG = 0;
    PTX_TRY(download(ctx, &NG, tot.p, 1));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((uint64_t)NG * 64 >= 0xFFFFFFFFull) return all_slow();   // slots are 32-bit
    if (NG) {
        PTX_HIP(ctx, db->d_vis_pos.alloc((uint64_t)NG * 64)); PTX_HIP(ctx, db->d_vis_head.alloc(NG)); PTX_HIP(ctx, db->d_vis_nbase.alloc(NG)); PTX_HIP(ctx, db->d_vis_sp.alloc(NG));
        PTX_HIP(ctx, vslot.alloc(db->V));
        PTX_TRY(byte_fill(ctx, db->d_vis_pos.p, 0xFF, (uint64_t)NG * 64 * sizeof(uint32_t)));
        PTX_TRY(byte_fill(ctx, db->d_vis_head.p, 0, (uint64_t)NG * sizeof(uint64_t)));
        PTX_TRY(byte_fill(ctx, db->d_vis_nbase.p, 0, (uint64_t)NG * sizeof(uint32_t)));
        PTX_TRY(byte_fill(ctx, db->d_vis_sp.p, 0, (uint64_t)NG * sizeof(uint32_t)));
        PTX_TRY(upload(ctx, db->d_trio_slow, slow.data(), slow.size()));
        hipLaunchKernelGGL(visit_pack_kernel<true>, dim3((NC + VP_CHUNKS - 1) / VP_CHUNKS), dim3(64), 0, ctx->stream, NC, d_chunks.p, cnt.p, (uint32_t *)nullptr,
                           (const uint32_t *)chunk_gbase.p, vslot.p, reinterpret_cast<unsigned long long *>(db->d_vis_head.p), db->d_vis_nbase.p, db->d_vis_sp.p);
        hipLaunchKernelGGL(visit_fill_kernel, tgrid, dim3(256), 0, ctx->stream, TRIO_GRAPH(db), db->d_trio_slow.p, vslot.p, cnt.p, db->d_vis_pos.p);
        hipLaunchKernelGGL(visit_sort_kernel, dim3((NG + 3) / 4), dim3(256), 0, ctx->stream, NG, db->d_vis_pos.p, db->d_vis_head.p, db->d_path_nodes.p);
    } else PTX_TRY(upload(ctx, db->d_trio_slow, slow.data(), slow.size()));
    PTX_HIP(ctx, hipGetLastError());
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the temporaries (and `slow`, `chunks`) go out of scope
    for (uint32_t s = 0; s < db->S; ++s) db->h_trio_slow[s] = slow[s] ? 1 : 0;
    db->n_vgroups = NG;
    db->trio_visit_ok = true;
    return 0;
}

int trio_runs_build(Ctx *ctx, Db *db) {
    db->trio_block_ok = false;
    db->n_blocks = 0; db->n_runs = 0;
    if (db->P == 0 || db->P >= 0xFFFFFFFFull) return 0;
    const TrioBlockTable bt = trio_block_table(db->h_node_off, db->h_trio_slow);
    if (!bt.ok) return 0;                             // such a db keeps the bucket path
    const std::vector<uint32_t> &blk_base = bt.blk_base;
    const uint32_t NB = bt.n_blocks;
    db->trio_block_ok = true;
    if (NB == 0) return 0;                            // every species goes through the visit table
    db->trio_block_ok = false;
    std::vector<uint32_t> blk_species(NB);
    for (uint32_t s = 0; s < db->S; ++s) std::fill(blk_species.begin() + blk_base[s], blk_species.begin() + blk_base[s + 1], s);
    PTX_TRY(upload(ctx, db->d_blk_base, blk_base.data(), db->S + 1));
    PTX_TRY(upload(ctx, db->d_blk_species, blk_species.data(), NB));
    DevBuf<uint32_t> cnt, scan_tmp, tot;
    PTX_HIP(ctx, cnt.alloc(2ull * (NB + 1)));
    PTX_HIP(ctx, scan_tmp.alloc(scan_tmp_elems(NB + 1)));
    PTX_HIP(ctx, tot.alloc(1));
    PTX_HIP(ctx, db->d_blk_run_off.alloc(NB + 1));
    PTX_HIP(ctx, hipMemsetAsync(cnt.p, 0, 2ull * (NB + 1) * sizeof(uint32_t), ctx->stream));
    const dim3 tgrid((uint32_t)db->n_tiles);
    hipLaunchKernelGGL(run_count_kernel, tgrid, dim3(256), 0, ctx->stream, TRIO_GRAPH(db), db->d_trio_slow.p, db->d_blk_base.p, cnt.p);
    PTX_TRY(exclusive_scan_u32(ctx, cnt.p, db->d_blk_run_off.p, (uint64_t)NB + 1, scan_tmp.p, tot.p));
    uint32_t h_tot = 0;
    PTX_TRY(download(ctx, &h_tot, tot.p, 1));
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PTX_HIP(ctx, db->d_runs.alloc(h_tot ? h_tot : 1));
    hipLaunchKernelGGL(run_fill_kernel, tgrid, dim3(256), 0, ctx->stream, TRIO_GRAPH(db), db->d_trio_slow.p, db->d_blk_base.p, db->d_blk_run_off.p, cnt.p + (NB + 1), db->d_runs.p);
    PTX_HIP(ctx, hipGetLastError());
    PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the temporaries go out of scope
    {   // one record per block for the build kernel: {first run, end run, global first node, species-local first node}
        std::vector<uint32_t> run_off(NB + 1);
        PTX_TRY(download(ctx, run_off.data(), db->d_blk_run_off.p, (size_t)NB + 1));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<uint4> rec(NB + 1);
        for (uint32_t s = 0; s < db->S; ++s)
            for (uint32_t gb = blk_base[s]; gb < blk_base[s + 1]; ++gb) {
                const uint32_t n0 = (gb - blk_base[s]) << TRIO_BLK_SHIFT;
                const uint32_t nn = (uint32_t)std::min<uint64_t>(TRIO_BLK, db->h_node_off[s + 1] - db->h_node_off[s] - n0);
                rec[gb] = make_uint4(run_off[gb], run_off[gb + 1], (uint32_t)db->h_node_off[s] + n0, (gb - blk_base[s]) | (nn << 24));   // < 2^21 blocks per species (2^27 nodes)
            }
        rec[NB] = make_uint4(h_tot, h_tot, (uint32_t)db->V, 0u);
        PTX_TRY(upload(ctx, db->d_blk_rec, rec.data(), rec.size()));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    db->n_blocks = NB;
    db->n_runs = h_tot;
    db->trio_block_ok = true;
    return 0;
}

}  // namespace ptx
