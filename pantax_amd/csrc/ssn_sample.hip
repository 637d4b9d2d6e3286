// ssn_sample.hip -- node-order row sort, stage 1: 4096 evenly spaced nodes of every segment, the rows among them sorted in LDS -> 1023 splitters at
// even ranks of the valid samples, stored as an implicit search tree in breadth-first order.  A segment of <= 4096 nodes is sorted completely right
// here (and, fused, its node statistics, column sums and c0 are formed here: the node pass returns early for it).
#include "ssn_device.hpp"

namespace ptx {

namespace {
template <bool FUSED>   // (compile time: the samplers of the two-kernel path keep the code they had)
__global__ void __launch_bounds__(256) ssn_gather_kernel(Sn sn) {
    const uint32_t s = blockIdx.y, o = sn.node_base[s], n = sn.node_base[s + 1] - o;
    uint32_t *w = sn.w(s);
    uint64_t *samp = reinterpret_cast<uint64_t *>(w + SN_OFF_SAMP);
    const bool small = n <= (uint32_t)SN_SAMPLE;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;   // grid.x covers SN_SAMPLE
    const uint64_t pos = small ? i : ((uint64_t)i * n) / SN_SAMPLE;
    uint64_t m = ~0ull, a = ~0ull;                       // not a row: sorts last
    const bool dead = !sn.mask && sn.skip_empty && sn.hp.sp_p[s] <= 0;   // a segment without LP columns has no rows: nothing sampled, nothing sorted (round 6)
    if (dead) { if (i == 0) { w[SN_OFF_FLAGS] = small ? 1u : 0u; w[SN_OFF_FLAGS + 1] = 0; w[SN_OFF_FLAGS + 2] = 0; w[SN_OFF_FLAGS + 3] = 0; } return; }
    if (pos < n) {
        const double av = sn_node_ab<FUSED>(sn, o + pos);
        const uint64_t mv = av > 0.0 ? sn_node_mask(sn, s, o + pos) : 0ull;
        if (av > 0.0 && mv != 0ull) { m = mv; a = (uint64_t)__double_as_longlong(av); }   // positive doubles order like their bit patterns
    }
    samp[i] = m; samp[SN_SAMPLE + i] = a;
    if (i == 0) { w[SN_OFF_FLAGS] = small ? 1u : 0u; w[SN_OFF_FLAGS + 1] = 0; w[SN_OFF_FLAGS + 2] = 0; w[SN_OFF_FLAGS + 3] = 0; }
}
// One 1024-thread workgroup per segment sorts its 4096 samples in LDS; the splitters are the valid samples at even ranks.
template <bool FUSED>
__global__ void __launch_bounds__(1024) ssn_sample_kernel(Sn sn) {
    __shared__ uint64_t km[SN_SAMPLE], ka[SN_SAMPLE];
    __shared__ uint32_t s_nv;
    const uint32_t s = blockIdx.x, o = sn.node_base[s], n = sn.node_base[s + 1] - o;
    uint32_t *w = sn.w(s);
    if (n == 0) { if (threadIdx.x == 0) { sn.seg_n[s] = 0; if (sn.c0) sn.c0[s] = 0.0; } return; }
    if constexpr (FUSED) {
        if (n <= (uint32_t)SN_SAMPLE && (!sn.fz.active || sn.fz.active[s])) {   // (workgroup-uniform) the histogram pass returns early for a small segment:
            NodeAcc acc;                                                        // its statistics are summed here, columns or not
            for (uint32_t i = threadIdx.x; i < n; i += 1024) acc.add(sn_node_ab<true>(sn, o + i), sn.fz.min_depth);
            sn_block_partial<16>(acc, sn.npart + (size_t)s * sn.G);
        }
    }
    if (!sn.mask && sn.skip_empty && sn.hp.sp_p[s] <= 0) {   // (see ssn_gather_kernel; the histogram pass writes the empty counts of a large segment)
        if (threadIdx.x == 0) { sn.seg_n[s] = 0; w[SN_OFF_FLAGS + 3] = 0; if (sn.c0) sn.c0[s] = 0.0; }
        return;
    }
    const uint64_t *samp = reinterpret_cast<const uint64_t *>(w + SN_OFF_SAMP);
    const bool small = n <= (uint32_t)SN_SAMPLE;
    if (threadIdx.x == 0) s_nv = 0;
    for (uint32_t i = threadIdx.x; i < (uint32_t)SN_SAMPLE; i += 1024) { km[i] = samp[i]; ka[i] = samp[SN_SAMPLE + i]; }
    __syncthreads();
    bitonic2<1024>(km, ka, SN_SAMPLE);
    uint32_t c = 0;
    for (uint32_t i = threadIdx.x; i < (uint32_t)SN_SAMPLE; i += 1024) c += ka[i] != ~0ull ? 1u : 0u;
    if (c) atomicAdd(&s_nv, c);
    __syncthreads();
    const uint32_t nv = s_nv;
    if (small) {                                         // every row of the segment, sorted: copied out by the local kernel
        for (uint32_t i = threadIdx.x; i < nv; i += 1024) sn.rows[o + i] = make_ulonglong2(km[i], ka[i]);
        if (threadIdx.x == 0) { sn.seg_n[s] = nv; w[SN_OFF_FLAGS + 3] = nv; }
        if (!sn.mask && sn.hp.ratio) {                   // masks from the haplotype words: this segment's column sums are this kernel's (the histogram pass skips it)
            __shared__ unsigned long long s_r[128];
            if (threadIdx.x < 128) s_r[threadIdx.x] = 0;
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < n; i += 1024) {
                uint64_t m = sn_node_mask(sn, s, o + i);
                const unsigned long long c = FUSED ? (m ? sn_node_cov<true>(sn, o + i) : 0u) : sn_node_cov<false>(sn, o + i), l = sn.hp.node_len[o + i];
                while (m) { const int k = __ffsll((long long)m) - 1; m &= m - 1; if (c) atomicAdd(&s_r[2 * k], c); atomicAdd(&s_r[2 * k + 1], l); }
            }
            __syncthreads();
            if (threadIdx.x < 128 && s_r[threadIdx.x]) atomicAdd(&sn.hp.ratio[2 * sn.hp.hap_off[s] + threadIdx.x], s_r[threadIdx.x]);
        }
        if (sn.c0) {                                     // the segment's nodes without a column (fixed order: deterministic)
            __shared__ double s_c[16];
            double c = 0.0;
            for (uint32_t i = threadIdx.x; i < n; i += 1024) { const double av = sn_node_ab<FUSED>(sn, o + i); if (av > 0.0 && sn_node_mask(sn, s, o + i) == 0ull) c += av; }
            c = wave_reduce(c, [](double x, double y) { return x + y; });
            if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
            __syncthreads();
            if (threadIdx.x == 0) { double t = 0.0; for (int q = 0; q < 16; ++q) t += s_c[q]; sn.c0[s] = t; }
        }
        return;
    }
    ulonglong2 *tree = reinterpret_cast<ulonglong2 *>(w + SN_OFF_TREE);
    for (uint32_t k = threadIdx.x; k < (uint32_t)SN_NLEAF; k += 1024) {
        if (k == 0) { tree[0] = make_ulonglong2(~0ull, ~0ull); continue; }
        const uint32_t j = tree_rank(k);                 // splitter j = the valid sample of rank (j + 1) nv / SN_NLEAF
        uint32_t r = (uint32_t)(((uint64_t)(j + 1) * nv) >> SN_LEVELS);
        if (r >= nv) r = nv ? nv - 1 : 0;
        tree[k] = nv ? make_ulonglong2(km[r], ka[r]) : make_ulonglong2(~0ull, ~0ull);
    }
}
}  // namespace

void ssn_sample_launch(Ctx *ctx, const Sn &sn, uint32_t S, bool fused) {
    if (fused) {
        hipLaunchKernelGGL(ssn_gather_kernel<true>, dim3(SN_SAMPLE / 256, S), dim3(256), 0, ctx->stream, sn);
        hipLaunchKernelGGL(ssn_sample_kernel<true>, dim3(S), dim3(1024), 0, ctx->stream, sn);
    } else {
        hipLaunchKernelGGL(ssn_gather_kernel<false>, dim3(SN_SAMPLE / 256, S), dim3(256), 0, ctx->stream, sn);
        hipLaunchKernelGGL(ssn_sample_kernel<false>, dim3(S), dim3(1024), 0, ctx->stream, sn);
    }
}

}  // namespace ptx
