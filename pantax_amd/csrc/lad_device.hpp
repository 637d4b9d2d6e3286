// lad_device.hpp -- device helpers that more than one stage of the strain step uses: fixed-order block reductions (node statistics, solver,
// objective), the mask . x dot products (solver, objective), splitmix64 (wide-mask hash, solver), and the chunk bound of the per-species partials.
#pragma once
#include "common.hpp"
#include "wave.hpp"

namespace ptx {

constexpr int STAT_CHUNKS = 256;  // most workgroups per species; partials are combined in fixed order (deterministic)

template <int NT>
__device__ __forceinline__ double block_sum_f64(double v, double *red) {
    v = wave_reduce(v, [](double x, double y) { return x + y; });
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += red[w];   // fixed order: deterministic
    __syncthreads();
    return t;
}
template <int NT>
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long *red) {
    v = wave_reduce(v, [](unsigned long long x, unsigned long long y) { return x + y; });
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += red[w];
    __syncthreads();
    return t;
}
template <int NT>
__device__ __forceinline__ double block_max_f64(double v, double *red) {
    v = wave_reduce(v, [](double x, double y) { return fmax(x, y); });
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) t = fmax(t, red[w]);
    __syncthreads();
    return t;
}

__device__ __forceinline__ double mdot(uint64_t m, const double *x) {   // ascending-bit order
    double s = 0.0;
    while (m) { int j = __ffsll((long long)m) - 1; s += x[j]; m &= m - 1; }
    return s;
}
template <int NW>
__device__ __forceinline__ double mdotw(const uint64_t *mw, const double *x) {   // ascending-bit order over NW mask words
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { uint64_t m = mw[w]; while (m) { int j = __ffsll((long long)m) - 1; s += x[64 * w + j]; m &= m - 1; } }
    return s;
}
// s += x[base + j] over the set bits j of m in ascending order, FOUR loads in flight (the additions keep their order: same bits as one at a time)
__device__ __forceinline__ void mdot_word4(uint64_t m, const double *x, int base, double &s) {
    while (m) {
        int j[4]; bool on[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { on[r] = m != 0ull; j[r] = on[r] ? __ffsll((long long)m) - 1 : 0; m &= m - 1; }   // (0 & anything = 0: an empty m stays empty)
        double t[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r] = x[base + j[r]];
#pragma unroll
        for (int r = 0; r < 4; ++r) if (on[r]) s += t[r];
    }
}
template <int NW>   // NW == 0: nw words, a run-time number
__device__ __forceinline__ double mdotx(const uint64_t *mw, int nw, const double *x) {
    if constexpr (NW != 0) return mdotw<NW>(mw, x);
    else {
        double s = 0.0;
        for (int w = 0; w < nw; ++w) mdot_word4(mw[w], x, 64 * w, s);
        return s;
    }
}
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace ptx
