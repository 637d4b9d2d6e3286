// ssn_partition.hip -- node-order row sort, stages 3 and 4: column sums of the count matrix -> bucket starts, the matrix rewritten as every
// workgroup's first slot in every bucket; rows per segment -> first output row of every segment, total row count; then the staged rows into their
// buckets as 16-byte records, and the tie buckets written as fills of the output.
#include "ssn_device.hpp"

namespace ptx {

namespace {
// bucket starts of a segment; the count matrix becomes the first slot of every workgroup in every bucket
__global__ void __launch_bounds__(256) ssn_offsets_kernel(Sn sn) {
    __shared__ uint32_t s_wave[4];
    const uint32_t s = blockIdx.x, n = sn.node_base[s + 1] - sn.node_base[s];
    uint32_t *w = sn.w(s);
    if (n == 0 || w[SN_OFF_FLAGS] != 0) return;          // (a small segment's row count is the sample kernel's)
    uint32_t *cm = sn.cntm + (size_t)s * sn.G * SN_NBUCKET;
    const uint32_t nt = (n + SN_TILE - 1) / SN_TILE, ng = (nt + sn.per - 1) / sn.per;   // workgroups that hold tiles
    constexpr int BPT = SN_NBUCKET / 256;                 // consecutive buckets per thread (a multiple of four)
    static_assert(BPT % 4 == 0 && BPT >= 4, "16-byte steps");
    const uint32_t b0 = threadIdx.x * BPT;
    uint32_t tot[BPT], sum = 0;
#pragma unroll
    for (int i = 0; i < BPT; ++i) tot[i] = 0;
    for (uint32_t g = 0; g < ng; ++g) {
#pragma unroll
        for (int q = 0; q < BPT; q += 4) {
            const uint4 c = *reinterpret_cast<const uint4 *>(cm + (size_t)g * SN_NBUCKET + b0 + q);
            tot[q] += c.x; tot[q + 1] += c.y; tot[q + 2] += c.z; tot[q + 3] += c.w;
        }
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) sum += tot[i];
    uint32_t total;
    uint32_t off = block_excl_scan<256>(sum, s_wave, &total);
    uint32_t run[BPT];
#pragma unroll
    for (int i = 0; i < BPT; ++i) { run[i] = off; w[SN_OFF_START + b0 + i] = off; off += tot[i]; }
    if (threadIdx.x == 255) w[SN_OFF_START + SN_NBUCKET] = off;
    for (uint32_t g = 0; g < ng; ++g) {
        uint32_t *p = cm + (size_t)g * SN_NBUCKET + b0;
#pragma unroll
        for (int q = 0; q < BPT; q += 4) {
            const uint4 c = *reinterpret_cast<const uint4 *>(p + q);
            *reinterpret_cast<uint4 *>(p + q) = make_uint4(run[q], run[q + 1], run[q + 2], run[q + 3]);
            run[q] += c.x; run[q + 1] += c.y; run[q + 2] += c.z; run[q + 3] += c.w;
        }
    }
    if (threadIdx.x == 0) {
        sn.seg_n[s] = total; w[SN_OFF_FLAGS + 3] = total;
        if (sn.c0) { double t = 0.0; for (uint32_t g = 0; g < ng; ++g) t += sn.c0p[(size_t)s * sn.G + g]; sn.c0[s] = t; }   // in workgroup order
    }
}
// first output row of every segment (the rows of all segments lie back to back), and the total
__global__ void __launch_bounds__(1024) ssn_segscan_kernel(uint32_t S, const uint32_t *__restrict__ seg_n, uint32_t *__restrict__ seg_out, uint32_t *__restrict__ d_n) {
    __shared__ uint32_t s_wave[16];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < S; base += 1024) {
        const uint32_t i = base + threadIdx.x, v = i < S ? seg_n[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan<1024>(v, s_wave, &tot);
        if (i < S) seg_out[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) { seg_out[S] = carry; *d_n = carry; }
}

__global__ void __launch_bounds__(256) ssn_scatter_kernel(Sn sn) {
    __shared__ uint32_t s_slot[SN_NBUCKET];
    const uint32_t s = blockIdx.y, g = blockIdx.x, o = sn.node_base[s], n = sn.node_base[s + 1] - o;
    const uint32_t *w = sn.w(s);
    if (n == 0 || w[SN_OFF_FLAGS] != 0) return;
    uint32_t t0, t1;
    sn_tiles(sn, n, g, t0, t1);
    if (t0 >= t1) return;
    const uint32_t cnt = sn.stage_cnt[(size_t)s * sn.G + g];
    if (cnt == 0) return;
    const uint32_t *row = sn.cntm + ((size_t)s * sn.G + g) * SN_NBUCKET;
    for (int i = threadIdx.x; i < SN_NBUCKET; i += 256) s_slot[i] = row[i];
    __syncthreads();
    // the staged rows of this workgroup (ssn_hist_kernel): the even buckets' rows only -- a row equal to a splitter does not travel at
    // all, its bucket holds copies of ONE key and ssn_ties_kernel writes it as a plain fill (cfg4: 64 % of the rows; long reads, whose
    // coverage values are small integers: nearly all)
    const ulonglong2 *st = sn.stage + o + t0 * SN_TILE;
    const uint16_t *sid = sn.ids + o + t0 * SN_TILE;
    for (uint32_t k0 = 0; k0 < cnt; k0 += 256 * SN_ITEMS) {
        ulonglong2 rec[SN_ITEMS];
        uint32_t id[SN_ITEMS];
#pragma unroll
        for (int r = 0; r < SN_ITEMS; ++r) {
            const uint32_t k = k0 + (uint32_t)r * 256u + threadIdx.x;
            id[r] = SN_NO_ROW; rec[r] = make_ulonglong2(0ull, 0ull);
            if (k < cnt) { id[r] = sid[k]; rec[r] = st[k]; }
        }
#pragma unroll
        for (int r = 0; r < SN_ITEMS; ++r) {
            if (id[r] == SN_NO_ROW) continue;
            const uint32_t pos = atomicAdd(&s_slot[id[r]], 1u);
            sn.rows[o + pos] = rec[r];
        }
    }
}

// The tie buckets (2j + 1: the rows equal to splitter j) as fills of the output: a workgroup takes SN_TIE_ROWS consecutive rows of its
// segment's output and walks the buckets that overlap them (a few large buckets hold most of the rows: by rows, not by buckets)
__global__ void __launch_bounds__(256) ssn_ties_kernel(Sn sn) {
    __shared__ uint32_t s_start[SN_NBUCKET + 1];
    const uint32_t s = blockIdx.y, o = sn.node_base[s], nn = sn.node_base[s + 1] - o;
    const uint32_t *w = sn.w(s);
    if (nn == 0 || w[SN_OFF_FLAGS] != 0) return;
    const uint32_t n = w[SN_OFF_FLAGS + 3], r0 = blockIdx.x * SN_TIE_ROWS;
    if (r0 >= n) return;
    const uint32_t r1 = min(n, r0 + SN_TIE_ROWS);
    for (uint32_t i = threadIdx.x; i <= (uint32_t)SN_NBUCKET; i += 256) s_start[i] = w[SN_OFF_START + i];
    __syncthreads();
    uint32_t lo = 0, hi = SN_NBUCKET;                            // first bucket that ends behind r0
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_start[mid + 1] <= r0) lo = mid + 1; else hi = mid; }
    const ulonglong2 *tree = reinterpret_cast<const ulonglong2 *>(w + SN_OFF_TREE);
    const uint32_t out = sn.seg_out[s];
    // 256 buckets at a time: the keys of their tie buckets are fetched by all threads at once (a dependent 16-byte load per bucket inside
    // the walk cost 0.1 of the 0.75 ms at cfg4), then the walk writes
    __shared__ ulonglong2 s_key[128];
    for (uint32_t qb = lo & ~1u; qb < (uint32_t)SN_NBUCKET && s_start[qb] < r1; qb += 256) {
        __syncthreads();
        if (threadIdx.x < 128u) {
            const uint32_t q = qb + 2u * threadIdx.x + 1u;       // odd bucket: splitter q >> 1
            if (q < (uint32_t)SN_NBUCKET - 1u && s_start[q + 1] > s_start[q]) s_key[threadIdx.x] = tree[tree_node(q >> 1)];
        }
        __syncthreads();
        for (uint32_t q = qb + 1u; q < qb + 256u && q < (uint32_t)SN_NBUCKET && s_start[q] < r1; q += 2) {
            const uint32_t a = max(s_start[q], r0), e = min(s_start[q + 1], r1);
            if (e <= a) continue;                                // (workgroup-uniform; a non-empty odd bucket has j < SN_NSPLIT)
            const ulonglong2 key = s_key[(q - qb) >> 1];
            // (keys_all == 0: `a` alone -- of a tie bucket ssn_heads_kernel wants the first row's mask at most, and takes it from the splitter tree)
            if (sn.keys_all) for (uint32_t i = a + threadIdx.x; i < e; i += 256) sn.put(s, out + i, key.x, key.y);
            else for (uint32_t i = a + threadIdx.x; i < e; i += 256) sn.ka[out + i] = key.y;
        }
    }
}
}  // namespace

void ssn_offsets_launch(Ctx *ctx, const Sn &sn, uint32_t S, uint32_t *d_n) {
    hipLaunchKernelGGL(ssn_offsets_kernel, dim3(S), dim3(256), 0, ctx->stream, sn);
    hipLaunchKernelGGL(ssn_segscan_kernel, dim3(1), dim3(1024), 0, ctx->stream, S, (const uint32_t *)sn.seg_n, sn.seg_out, d_n);
}

void ssn_scatter_launch(Ctx *ctx, const Sn &sn, uint32_t S) {
    hipLaunchKernelGGL(ssn_scatter_kernel, dim3(sn.G, S), dim3(256), 0, ctx->stream, sn);
}

void ssn_ties_launch(Ctx *ctx, const Sn &sn, uint32_t S, uint32_t tie_grid) {
    hipLaunchKernelGGL(ssn_ties_kernel, dim3(tie_grid, S), dim3(256), 0, ctx->stream, sn);
}

}  // namespace ptx
