// bootstrap_plan_check.cpp -- the host side of pantax_hip_strain_bootstrap at its edges: the plan of the chunks (pantax_amd/csrc/bootstrap_plan.hpp), the
// summary over replicates and the weight helper.  A program of its own: tests/test_bootstrap_plan.py compiles it with bootstrap_plan.cpp and report_plan.cpp by the host C++
// compiler under -fsanitize=address,undefined and runs it; it returns non-zero at the first check that fails.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "bootstrap_plan.hpp"
#include "bootstrap_weight.hpp"
#include "report_plan.hpp"

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "bootstrap_plan_check:%d: %s\n", __LINE__, #cond);     \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

using namespace ptx;

int main() {
    BootstrapPlan pl;
    std::string err;
    // ---- the bound of a replicate
    CHECK(bootstrap_rows_bound(0) == 0);
    CHECK(bootstrap_rows_bound(1) == 16);                    // the certain bound 16 N is the smaller one for few rows
    CHECK(bootstrap_rows_bound(5) == 80);
    CHECK(bootstrap_rows_bound(100) == 100 + 80 + 64);
    CHECK(bootstrap_rows_bound(101) == 101 + 88 + 64);       // ceil(sqrt(101)) = 11
    CHECK(bootstrap_rows_bound(1ull << 40) == (1ull << 40) + 8 * (1ull << 20) + 64);
    CHECK(bootstrap_rows_bound(~0ull) == ~0ull);             // saturates
    CHECK(bootstrap_rows_bound((1ull << 63) + 12345) > (1ull << 63));
    for (uint64_t n = 1; n < 5000; ++n) CHECK(bootstrap_rows_bound(n) >= n && bootstrap_rows_bound(n) <= 16 * n && bootstrap_rows_bound(n + 1) >= bootstrap_rows_bound(n));
    // ---- the plan: R = 1
    CHECK(bootstrap_plan(1000, 1, 1u << 20, pl, err));
    CHECK(pl.per_chunk == 1 && pl.n_chunks == 1 && pl.bound == 1000 + 8 * 32 + 64 && pl.chunk_rows == pl.bound);
    // all of them in one chunk, and never more than R
    CHECK(bootstrap_plan(1000, 34, 1u << 20, pl, err));
    CHECK(pl.per_chunk == 34 && pl.n_chunks == 1 && pl.chunk_rows == 34 * pl.bound);
    // a cap of exactly one replicate, of exactly two, and one row below one
    const uint64_t b1000 = bootstrap_rows_bound(1000);
    CHECK(bootstrap_plan(1000, 34, b1000, pl, err) && pl.per_chunk == 1 && pl.n_chunks == 34 && pl.chunk_rows == b1000);
    CHECK(bootstrap_plan(1000, 34, 2 * b1000, pl, err) && pl.per_chunk == 2 && pl.n_chunks == 17);
    CHECK(bootstrap_plan(1000, 34, 3 * b1000 - 1, pl, err) && pl.per_chunk == 2);
    CHECK(bootstrap_plan(1000, 33, 2 * b1000, pl, err) && pl.per_chunk == 2 && pl.n_chunks == 17);   // the last chunk holds one
    err.clear();
    CHECK(!bootstrap_plan(1000, 34, b1000 - 1, pl, err));
    CHECK(err.find("bootstrap_rows_max") != std::string::npos && err.find("1000 rows") != std::string::npos && pl.per_chunk == 0);
    CHECK(!bootstrap_plan(1000, 34, 0, pl, err));
    // no rows at all: nothing to size, one chunk
    CHECK(bootstrap_plan(0, 101, 0, pl, err) && pl.per_chunk == 101 && pl.n_chunks == 1 && pl.bound == 0 && pl.chunk_rows == 0);
    // no replicate count at all, and one beyond 32 bits
    CHECK(!bootstrap_plan(10, 0, 1000, pl, err));
    CHECK(!bootstrap_plan(10, 1ull << 32, 1ull << 40, pl, err));
    CHECK(bootstrap_plan(10, 0xFFFFFFFFull, 1ull << 40, pl, err) && pl.per_chunk >= 1);
    // u64 sizes: the cap is cut to 32-bit row positions, the scan's items stay below 2^32, rows beyond any cap are refused
    CHECK(bootstrap_plan(1u << 20, 1u << 20, ~0ull, pl, err));
    CHECK(pl.per_chunk >= 1 && pl.chunk_rows <= BOOT_ROWS_HARD_MAX && (uint64_t)pl.per_chunk * (1u << 20) <= BOOT_ROWS_HARD_MAX);
    CHECK((uint64_t)pl.n_chunks * pl.per_chunk >= (1u << 20) && ((uint64_t)pl.n_chunks - 1) * pl.per_chunk < (1u << 20));
    CHECK(!bootstrap_plan(1ull << 32, 2, ~0ull, pl, err));
    CHECK(!bootstrap_plan(~0ull, 2, ~0ull, pl, err));
    CHECK(!bootstrap_plan((1ull << 63) + 1, 101, ~0ull, pl, err));
    CHECK(bootstrap_plan(4000000000ull, 3, ~0ull, pl, err) && pl.per_chunk == 1 && pl.n_chunks == 3);
    // the default cap: a quarter of the free memory in rows, cut to 32-bit positions
    CHECK(bootstrap_default_cap(0) == 0);
    CHECK(bootstrap_default_cap(4 * BOOT_BYTES_PER_ROW * 1000 + 5) == 1000);
    CHECK(bootstrap_default_cap(~0ull) == BOOT_ROWS_HARD_MAX);
    // ---- the weight: replicate 0, the table's borders, the hand case of tests/test_bootstrap_ref.py
    CHECK(pantax_hip_bootstrap_weight(1, 2, 0, 3) == 1 && pantax_hip_bootstrap_weight(~0ull, ~0ull, 0, ~0ull) == 1);
    CHECK(boot_weight_of(0) == 0 && boot_weight_of(0x5E2D58D8B3BCDF19ull) == 0 && boot_weight_of(0x5E2D58D8B3BCDF1Aull) == 1);
    CHECK(boot_weight_of(0xBC5AB1B16779BE34ull) == 1 && boot_weight_of(0xBC5AB1B16779BE35ull) == 2);
    CHECK(boot_weight_of(0xFFFFFFFFFFFABE21ull) == 15 && boot_weight_of(0xFFFFFFFFFFFABE22ull) == 16 && boot_weight_of(~0ull) == 16);
    CHECK(boot_sm(562) == 0x583afb6005b2b82full && boot_species_hash(42, 562) == 0x26cb153f4791da56ull);
    const uint32_t w1[8] = {0, 1, 2, 2, 1, 1, 1, 3}, w2[8] = {2, 1, 1, 0, 0, 0, 1, 0};
    for (uint64_t v = 0; v < 8; ++v) CHECK(pantax_hip_bootstrap_weight(42, 562, 1, v) == w1[v] && pantax_hip_bootstrap_weight(42, 562, 2, v) == w2[v]);
    (void)pantax_hip_bootstrap_weight(~0ull, ~0ull, 0xFFFFFFFFu, ~0ull);   // every sum wraps: unsigned arithmetic
    {   // 10^6 draws: every cell within 4 binomial standard deviations of n p_j
        const uint64_t n = 1000000;
        uint64_t hist[17] = {0};
        for (uint32_t b = 1; b <= 1000; ++b) for (uint64_t v = 0; v < 1000; ++v) ++hist[pantax_hip_bootstrap_weight(99, 4711, b, v)];
        double p = std::exp(-1.0), rest = 1.0;
        for (int j = 0; j < 17; ++j) {
            const double pj = j < 16 ? p : (rest > 0 ? rest : 0.0);
            CHECK(std::fabs((double)hist[j] - n * pj) <= 4 * std::sqrt(n * pj * (1 - pj)) + 1e-9);
            rest -= p;
            p /= (double)(j + 1);
        }
    }
    // ---- the summary
    double out[10];
    CHECK(pantax_hip_bootstrap_summary(0, nullptr, nullptr, nullptr) == PANTAX_HIP_E_INVALID);
    CHECK(pantax_hip_bootstrap_summary(3, nullptr, nullptr, out) == PANTAX_HIP_E_INVALID);
    for (double &o : out) o = 7.0;
    CHECK(pantax_hip_bootstrap_summary(0, nullptr, nullptr, out) == 0);
    for (double o : out) CHECK(o == 0.0);
    const double one[1] = {2.5};
    CHECK(pantax_hip_bootstrap_summary(1, one, nullptr, out) == 0);
    CHECK(out[0] == 1 && out[1] == 2.5 && out[2] == 0.0 && out[3] == 2.5 && out[7] == 2.5 && out[8] == 0.0 && out[9] == 2.5);
    const double two[2] = {4.0, 1.0};
    CHECK(pantax_hip_bootstrap_summary(2, two, nullptr, out) == 0);
    CHECK(out[0] == 2 && out[1] == 2.5 && out[2] == std::sqrt(4.5) && out[3] == 1.0 && out[7] == 1.0 && out[9] == 1.0);
    std::vector<double> x(101);
    std::vector<int32_t> st(101, 0);
    for (int i = 0; i <= 100; ++i) x[i] = 100 - i;
    CHECK(pantax_hip_bootstrap_summary(101, x.data(), st.data(), out) == 0);
    CHECK(out[0] == 101 && out[1] == 50.0 && out[3] == 2.0 && out[4] == 25.0 && out[5] == 50.0 && out[6] == 75.0 && out[7] == 97.0 && out[8] == 1.0 / 101 && out[9] == 0.0);
    for (int i = 0; i <= 100; ++i) st[i] = i % 2 ? PANTAX_HIP_E_SOLVER : 0;   // every second one not solved: 100, 98, .., 0
    CHECK(pantax_hip_bootstrap_summary(101, x.data(), st.data(), out) == 0);
    CHECK(out[0] == 51 && out[1] == 50.0 && out[5] == 50.0 && out[9] == 0.0 && out[8] == 1.0 / 51);
    for (int i = 0; i <= 100; ++i) st[i] = 1;
    CHECK(pantax_hip_bootstrap_summary(101, x.data(), st.data(), out) == 0);
    for (double o : out) CHECK(o == 0.0);
    // ---- the report in the file seam's plan: a field of pantax_hip_profile_ext2, which begins with the 16-byte first version; a row of EXT2_REPORTS
    {
        static_assert(offsetof(pantax_hip_profile_ext2, v1) == 0 && sizeof(pantax_hip_profile_ext) == 16, "the first version keeps its place and size");
        static_assert(offsetof(pantax_hip_profile_ext2, strain_bootstrap_file) == 16 && offsetof(pantax_hip_profile_ext2, strain_bootstrap_replicates) == 24 &&
                      offsetof(pantax_hip_profile_ext2, strain_bootstrap_seed) == 32 && sizeof(pantax_hip_profile_ext2) == 40, "appended behind it");
        CHECK(N_EXT2_REPORTS == 1 && EXT2_REPORTS[X2REP_BOOTSTRAP].field == &pantax_hip_profile_ext2::strain_bootstrap_file && EXT2_REPORTS[X2REP_BOOTSTRAP].rows);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        pantax_hip_profile_ext2 e2{};
        e2.v1.struct_size = sizeof(e2);
        e2.strain_bootstrap_file = "boot.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(&e2.v1, 1, false, rp, err));
        CHECK(rp.ext2_want[X2REP_BOOTSTRAP] && !rp.ext2_run[X2REP_BOOTSTRAP] && rp.ext2_path[X2REP_BOOTSTRAP] == "boot.tsv" && !rp.ext_want[XREP_FIT]);
        CHECK(rp.bs_replicates == 100 && rp.bs_seed == 0);          // 0 replicates read as 100; a seed the struct holds is taken as it is
        resume_reports(rp, true, true, false);
        CHECK(rp.ext2_run[X2REP_BOOTSTRAP] && rp.any_run() && rp.rows_run());
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext2_run[X2REP_BOOTSTRAP] && !rp.any_run());
        e2.strain_bootstrap_replicates = 8; e2.strain_bootstrap_seed = 43;
        CHECK(plan_ext_reports(&e2.v1, 1, false, rp, err) && rp.bs_replicates == 8 && rp.bs_seed == 43);
        e2.strain_bootstrap_replicates = 0xFFFFFFFFull;
        CHECK(!plan_ext_reports(&e2.v1, 1, false, rp, err) && err.find("strain_bootstrap_replicates") != std::string::npos);
        e2.strain_bootstrap_replicates = 0xFFFFFFFEull;
        CHECK(plan_ext_reports(&e2.v1, 1, false, rp, err) && rp.bs_replicates == 0xFFFFFFFEu);
        CHECK(!plan_ext_reports(&e2.v1, 2, false, rp, err) && err == "profile: the bootstrap report (strain_bootstrap_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(&e2.v1, 1, true, rp, err) && err == "profile: the bootstrap report (strain_bootstrap_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e2.v1.strain_fit_file = "fit.tsv";                            // the fit report's refusal comes first
        CHECK(!plan_ext_reports(&e2.v1, 2, false, rp, err) && err.find("strain_fit_file") != std::string::npos);
        // a caller with the first version only: the report is off whatever lies behind the 16 bytes; 24 and 32 bytes hold the path but not the seed: 42
        e2.v1.struct_size = 16;
        CHECK(plan_ext_reports(&e2.v1, 1, false, rp, err) && rp.ext_want[XREP_FIT] && !rp.ext2_want[X2REP_BOOTSTRAP] && rp.ext2_path[X2REP_BOOTSTRAP].empty());
        e2.v1.struct_size = 24; e2.strain_bootstrap_replicates = 8;
        CHECK(plan_ext_reports(&e2.v1, 1, false, rp, err) && rp.ext2_want[X2REP_BOOTSTRAP] && rp.bs_replicates == 100 && rp.bs_seed == 42);
        e2.v1.struct_size = 32;
        CHECK(plan_ext_reports(&e2.v1, 1, false, rp, err) && rp.bs_replicates == 8 && rp.bs_seed == 42);
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e2.v1.struct_size = sizeof(e2); e2.strain_bootstrap_file = off;
            e2.v1.strain_fit_file = nullptr;
            CHECK(plan_ext_reports(&e2.v1, 2, true, rp, err) && !rp.ext2_want[X2REP_BOOTSTRAP]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext2_want[X2REP_BOOTSTRAP] && rp.bs_replicates == 100 && rp.bs_seed == 42);
    }
    std::printf("bootstrap_plan_check: ok\n");
    return 0;
}
