// ssn_local.hip -- node-order row sort, stage 5: the sorts inside a bucket.  A wave per even bucket sorts up to 512 rows IN REGISTERS (eight per
// lane: a bitonic network whose cross-lane steps are ds_bpermute swaps and whose in-lane steps are plain selects -- no LDS memory, no barriers); the
// buckets of 513 .. 1024 rows go through a second kernel with sixteen rows per lane, so that its registers do not cost the first one its waves in
// flight (2.2 -> 3.1 ms when it was one); the rare larger ones through an LDS network, above 4096 rows in place through memory.
#include "ssn_device.hpp"

namespace ptx {

namespace {
// ---------------------------------------------------------------------------------------------
// A wave's register network: 64 * L keys, lane l holds elements l * L .. l * L + L - 1 of the sequence being sorted.
// Step (k, j) of the bitonic network pairs element i with i ^ j; j >= L: the partner sits in lane l ^ (j / L), same register
// -- one ds_bpermute per 32-bit half, then the lane keeps the smaller or the larger key; j < L: both in this lane.
// TWO: keys are (m, a); otherwise `a` alone moves (a bucket between two splitters of one mask).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t lane_xor64(uint64_t v, int addr /* (partner lane) << 2 */) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
template <bool TWO>
__device__ __forceinline__ void cmp_swap(uint64_t &m0, uint64_t &a0, uint64_t &m1, uint64_t &a1, bool up) {
    // up: afterwards key0 <= key1; otherwise key0 >= key1.  ONE comparison: equal keys may swap, which changes nothing
    const bool lt10 = TWO ? less2(Key2{m1, a1}, Key2{m0, a0}) : (a1 < a0);
    const bool sw = up == lt10;
    const uint64_t ta = sw ? a1 : a0, tb = sw ? a0 : a1;
    a0 = ta; a1 = tb;
    if (TWO) { const uint64_t tm = sw ? m1 : m0, tn = sw ? m0 : m1; m0 = tm; m1 = tn; }
}
template <int L, bool TWO>
__device__ __forceinline__ void wave_sort_regs(uint64_t (&m)[L], uint64_t (&a)[L]) {
    const uint32_t lane = threadIdx.x & 63;
    // stages whose direction depends on the element's place inside the lane (k < L)
#pragma unroll
    for (int k = 2; k < L; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int e = 0; e < L; ++e)
                if ((e & j) == 0) cmp_swap<TWO>(m[e], a[e], m[e | j], a[e | j], (e & k) == 0);
    // stages k = L .. 64 L: the direction is the lane's
    for (uint32_t kl = 1; kl <= 64; kl <<= 1) {          // kl = k / L
        const bool up = (lane & kl) == 0;
        for (uint32_t jl = kl >> 1; jl > 0; jl >>= 1) {  // cross-lane steps: partner lane ^ jl
            const int addr = (int)((lane ^ jl) << 2);
            const bool keep_min = up == ((lane & jl) == 0);
#pragma unroll
            for (int e = 0; e < L; ++e) {
                const uint64_t oa = lane_xor64(a[e], addr);
                uint64_t om = 0;
                if (TWO) om = lane_xor64(m[e], addr);
                const bool o_lt = TWO ? less2(Key2{om, oa}, Key2{m[e], a[e]}) : (oa < a[e]);
                const bool take = keep_min == o_lt;               // (keeping the larger one: an equal key may be taken, which changes nothing)
                a[e] = take ? oa : a[e];
                if (TWO) m[e] = take ? om : m[e];
            }
        }
#pragma unroll
        for (int j = L >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int e = 0; e < L; ++e)
                if ((e & j) == 0) cmp_swap<TWO>(m[e], a[e], m[e | j], a[e | j], up);
    }
}
// one bucket of n <= 64 L rows: src (16-byte records) -> sorted -> the segment's output at dst
template <int L, bool TWO>
__device__ __forceinline__ void wave_sort_bucket(const Sn &sn, uint32_t s, const ulonglong2 *__restrict__ src, uint32_t n, uint32_t dst, uint64_t mv) {
    // TWO = the pair is mixed (sn_pair_mixed): its rows keep their key words in every mode
    const uint32_t lane = threadIdx.x & 63;
    uint64_t m[L], a[L];
#pragma unroll
    for (int e = 0; e < L; ++e) {                 // any assignment of rows to elements will do: coalesced loads
        const uint32_t i = (uint32_t)e * 64u + lane;
        m[e] = ~0ull; a[e] = ~0ull;               // pads sort behind every row
        if (i < n) { const ulonglong2 r = src[i]; m[e] = r.x; a[e] = r.y; }
    }
    wave_sort_regs<L, TWO>(m, a);
#pragma unroll
    for (int e = 0; e < L; ++e) {
        const uint32_t i = lane * (uint32_t)L + (uint32_t)e;
        if (i < n) sn.put_if(TWO, s, dst + i, TWO ? m[e] : mv, a[e]);
    }
}

// A wave per even bucket 2j, sorted in registers (more than SN_WAVE_CAP rows: left on the segment's list for the second kernel).
__global__ void __launch_bounds__(256) ssn_local_wave_kernel(Sn sn) {
    // (flat grids whose waves / workgroups walk several (segment, bucket) items were measured in round 6 for this kernel and the tie fills: 1.10 -> 1.32 ms here at
    // cfg4, +0.2 ms a step at the reference-DB shape with its 2.3 million mostly idle workgroups -- starting workgroups that find nothing is not the cost)
    const uint32_t s = blockIdx.y, o = sn.node_base[s], nn = sn.node_base[s + 1] - o;
    uint32_t *w = sn.w(s);
    if (nn == 0 || w[SN_OFF_FLAGS] != 0) return;
    const uint32_t *bucket_start = w + SN_OFF_START;
    const ulonglong2 *tree = reinterpret_cast<const ulonglong2 *>(w + SN_OFF_TREE);
    const uint32_t lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);   // grid.x * 4 = SN_NLEAF pairs
    const uint32_t out = sn.seg_out[s];
    const uint32_t st = bucket_start[2 * j], st1 = bucket_start[2 * j + 1];   // (the tie bucket 2j + 1 went to the output in the scatter pass)
    const uint32_t m = st1 - st;
    if (m == 0) return;
    const ulonglong2 *src = sn.rows + o + st;
    if (m > (uint32_t)SN_WAVE_CAP) { if (lane == 0) w[SN_OFF_MED + atomicAdd(&w[SN_OFF_FLAGS + 2], 1u)] = 2 * j; return; }
    // between two splitters with the same mask every row has that mask: only `a` moves through the network
    uint64_t mv = 0;
    const bool one = !sn_pair_mixed(tree, j, &mv);
    if (m == 1) { if (lane == 0) { const ulonglong2 r = src[0]; sn.put_if(!one, s, out + st, r.x, r.y); } return; }
    const uint32_t dst = out + st;
    if (one) {
        if (m <= 64) wave_sort_bucket<1, false>(sn, s, src, m, dst, mv);
        else if (m <= 128) wave_sort_bucket<2, false>(sn, s, src, m, dst, mv);
        else if (m <= 256) wave_sort_bucket<4, false>(sn, s, src, m, dst, mv);
        else wave_sort_bucket<8, false>(sn, s, src, m, dst, mv);
    } else {
        if (m <= 64) wave_sort_bucket<1, true>(sn, s, src, m, dst, mv);
        else if (m <= 128) wave_sort_bucket<2, true>(sn, s, src, m, dst, mv);
        else if (m <= 256) wave_sort_bucket<4, true>(sn, s, src, m, dst, mv);
        else wave_sort_bucket<8, true>(sn, s, src, m, dst, mv);
    }
}
// The first kernel's list: a wave per bucket of 513 .. SN_WAVE_CAP2 rows, sixteen per lane; larger ones go on the next list
__global__ void __launch_bounds__(256) ssn_local_wave2_kernel(Sn sn) {
    const uint32_t s = blockIdx.y, o = sn.node_base[s], nn = sn.node_base[s + 1] - o;
    uint32_t *w = sn.w(s);
    if (nn == 0 || w[SN_OFF_FLAGS] != 0) return;
    const uint32_t n_work = w[SN_OFF_FLAGS + 2];
    const uint32_t *bucket_start = w + SN_OFF_START;
    const ulonglong2 *tree = reinterpret_cast<const ulonglong2 *>(w + SN_OFF_TREE);
    const uint32_t lane = threadIdx.x & 63, out = sn.seg_out[s];
    for (uint32_t wi = blockIdx.x * 4 + (threadIdx.x >> 6); wi < n_work; wi += gridDim.x * 4) {
        const uint32_t bid = w[SN_OFF_MED + wi], j = bid >> 1;
        const uint32_t st = bucket_start[bid], m = bucket_start[bid + 1] - st;
        if (m > (uint32_t)SN_WAVE_CAP2) { if (lane == 0) w[SN_OFF_BIG + atomicAdd(&w[SN_OFF_FLAGS + 1], 1u)] = bid; continue; }
        uint64_t mv = 0;
        const bool one = !sn_pair_mixed(tree, j, &mv);
        if (one) wave_sort_bucket<16, false>(sn, s, sn.rows + o + st, m, out + st, mv);
        else wave_sort_bucket<16, true>(sn, s, sn.rows + o + st, m, out + st, mv);
    }
}

// What the wave kernels leave: buckets of more than SN_WAVE_CAP2 rows (an LDS network up to SN_CAP rows, a rank sort through memory
// above), and the copy of a small segment.
__global__ void __launch_bounds__(256) ssn_local_kernel(Sn sn) {
    __shared__ uint64_t km[SN_CAP], ka[SN_CAP];
    const uint32_t s = blockIdx.y, o = sn.node_base[s], nn = sn.node_base[s + 1] - o;
    if (nn == 0) return;
    uint32_t *w = sn.w(s);
    const uint32_t out = sn.seg_out[s];
    if (w[SN_OFF_FLAGS] != 0) {      // small segment: the sample kernel sorted every row into the scratch
        const uint32_t n = w[SN_OFF_FLAGS + 3];
        for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) { const ulonglong2 r = sn.rows[o + i]; sn.put(s, out + i, r.x, r.y); }
        return;
    }
    const uint32_t *bucket_start = w + SN_OFF_START;
    const ulonglong2 *tree = reinterpret_cast<const ulonglong2 *>(w + SN_OFF_TREE);
    const uint32_t n_work = w[SN_OFF_FLAGS + 1];
    for (uint32_t wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
        const uint32_t bid = w[SN_OFF_BIG + wi];
        const bool mixed = sn_pair_mixed(tree, bid >> 1);   // (both networks here move whole keys; what is left out is the store of the key words)
        const uint32_t st = bucket_start[bid], m = bucket_start[bid + 1] - st;
        const ulonglong2 *src = sn.rows + o + st;
        const uint32_t dst = out + st;
        __syncthreads();   // LDS reuse across the buckets of this workgroup
        if (m <= (uint32_t)SN_CAP) {
            uint32_t N = 2;
            while (N < m) N <<= 1;
            for (uint32_t i = threadIdx.x; i < N; i += 256) {
                if (i < m) { const ulonglong2 r = src[i]; km[i] = r.x; ka[i] = r.y; } else { km[i] = ~0ull; ka[i] = ~0ull; }
            }
            __syncthreads();
            bitonic2<256>(km, ka, N);
            for (uint32_t i = threadIdx.x; i < m; i += 256) sn.put_if(mixed, s, dst + i, km[i], ka[i]);
            continue;
        }
        // A bucket of more than SN_CAP rows (an unrepresentative sample; every bucket of a segment of millions of rows): the network runs
        // IN PLACE in the scratch, through memory, by this one workgroup -- O(m log^2 m) where the rank sort it replaces was O(m^2).  The
        // variant whose merges start with a MIRROR step compares upwards only, so the places behind m act as +inf pads without existing.
        ulonglong2 *buf = sn.rows + o + st;
        uint32_t N = 2;
        while (N < m) N <<= 1;
        auto exchange = [&](uint32_t i, uint32_t l) {             // i < l < m: the smaller key to i
            const ulonglong2 x = buf[i], y = buf[l];
            if (less2(Key2{y.x, y.y}, Key2{x.x, x.y})) { buf[i] = y; buf[l] = x; }
        };
        for (uint32_t k = 2; k <= N; k <<= 1) {
            const uint32_t hk = k >> 1;
            for (uint32_t t = threadIdx.x; t < N / 2; t += 256) {
                const uint32_t blk = t / hk, off = t - blk * hk, i = blk * k + off, l = blk * k + (k - 1u - off);
                if (l < m) exchange(i, l);
            }
            __threadfence_block();
            __syncthreads();
            for (uint32_t j = hk >> 1; j > 0; j >>= 1) {
                for (uint32_t t = threadIdx.x; t < N / 2; t += 256) {
                    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
                    if (l < m) exchange(i, l);
                }
                __threadfence_block();
                __syncthreads();
            }
        }
        for (uint32_t i = threadIdx.x; i < m; i += 256) { const ulonglong2 r = buf[i]; sn.put_if(mixed, s, dst + i, r.x, r.y); }
    }
}
}  // namespace

void ssn_local_launch(Ctx *ctx, const Sn &sn, uint32_t S) {
    hipLaunchKernelGGL(ssn_local_wave_kernel, dim3(SN_NLEAF / 4, S), dim3(256), 0, ctx->stream, sn);
    hipLaunchKernelGGL(ssn_local_wave2_kernel, dim3(8, S), dim3(256), 0, ctx->stream, sn);
    hipLaunchKernelGGL(ssn_local_kernel, dim3(8, S), dim3(256), 0, ctx->stream, sn);
}

}  // namespace ptx
