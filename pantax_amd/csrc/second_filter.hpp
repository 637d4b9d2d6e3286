// second_filter.hpp -- a13 on the device: the second filter's decision of one species, taken by one thread of its solver workgroup between the
// two solves of lad_pair_kernel (stage_lad.hip).  Same arithmetic as the host reporting code in api_strain.cpp (IEEE f64, no contraction-sensitive forms).
#pragma once
#include "common.hpp"

namespace ptx {

__device__ __forceinline__ double d_round2(double x) { return round(x * 100.0) / 100.0; }   // f64::round: half away from zero

// second_filter_paths (profile.rs:1229-1285): which columns are pinned to zero in the second solve
struct SecondFilterArgs {
    const uint64_t *hap_off;
    const uint32_t *hap_nt;      // [H] unique-trio rows per haplotype, [S] any in the species: the first filter's copies
    const uint8_t *sp_trio;
    const int32_t *hap_bit, *sp_p;
    const uint32_t *nnz;
    const double *meanf;
    const unsigned long long *ratio;
    const double *x1;
    const int32_t *status1;
    double fc, sr;
    uint8_t *fixed2, *need2;
};
// second_filter_paths decisions of one species (profile.rs:1234-1268): which LP columns are pinned to zero in
// the second solve, and whether there is a second solve at all
__device__ __forceinline__ void second_filter_species(const SecondFilterArgs &F, uint32_t s) {
    const uint64_t h0 = F.hap_off[s], h1 = F.hap_off[s + 1];
    uint8_t need = 0;
    for (uint64_t h = h0; h < h1; ++h) F.fixed2[h] = 0;   // column k of the species lives at h0 + k
    if (F.sp_p[s] > 0 && F.status1[s] == 0 && (h1 - h0) != 1 && F.sp_trio[s]) {
        for (uint64_t h = h0; h < h1; ++h) {
            const int k = F.hap_bit[h];
            if (k < 0) continue;
            const double fm = F.meanf[h];
            bool keep = false;
            if (fm != 0.0) {                                               // :1238
                const double sol = F.x1[h0 + k];
                const double f = d_round2(fabs(sol - fm) / (sol + fm));
                if (f > F.fc) {
                    if (f <= 0.6) {
                        const double frac_r = d_round2((double)F.nnz[h] / (double)F.hap_nt[h]);
                        const float cov = (float)F.ratio[(h0 + k) * 2], len = (float)F.ratio[(h0 + k) * 2 + 1];
                        const double sc = frac_r * (double)(cov / len);
                        if (!(sc < F.sr || sol == 0.0)) keep = true;       // rescue
                    }
                } else if (sol != 0.0) keep = true;
            }
            if (!keep) { F.fixed2[h0 + k] = 1; need = 1; }
        }
    }
    F.need2[s] = need;
}

}  // namespace ptx
