// fragments_plan_check.cpp -- the host side of the fragment support at its edges: the fragment key of a read id (pantax_hip_fragment_key) on ids done by
// hand, and the report's row in the plan of the file seam (pantax_hip_profile_ext11 behind the 200-byte tenth version).  A program of its own:
// tests/test_fragments_plan.py compiles it with fragments_plan.cpp and report_plan.cpp by the host C++ compiler under -fsanitize=address,undefined and
// runs it; it returns non-zero at the first check that fails.  Every argument is an id in hex digits ("-": the empty id): its key and tag are printed,
// one line an id, for the test to hold against the Python restatement.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "fragments_plan.hpp"
#include "report_plan.hpp"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "fragments_plan_check:%d: %s\n", __LINE__, #cond); \
            return 1;                                                               \
        }                                                                           \
    } while (0)

using namespace ptx;

namespace {

struct KeyTag { uint64_t key; uint8_t tag; int rc; };
KeyTag key_of(const std::string &id) {
    KeyTag k{77, 77, 0};
    std::vector<char> exact(id.begin(), id.end());   // no byte behind the id: the sanitizer sees a read past its end
    static const char none = 0;
    k.rc = pantax_hip_fragment_key(exact.empty() ? &none : exact.data(), exact.size(), &k.key, &k.tag);
    return k;
}
uint64_t hash_of(const std::string &s) { return fragment_id_hash(s.data(), s.size()); }
bool is(const KeyTag &k, uint64_t key, unsigned tag) { return k.rc == 0 && k.key == key && k.tag == tag; }
int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

}  // namespace

int main(int argc, char **argv) {
    // ---- the id hash: FNV-1a-64 (the published vectors) and the avalanche behind it
    const auto avalanche = [](uint64_t h) { h ^= h >> 32; h *= 0xd6e8feb86659fd93ull; h ^= h >> 32; return h; };
    CHECK(hash_of("") == avalanche(0xcbf29ce484222325ull) && hash_of("a") == avalanche(0xaf63dc4c8601ec8cull) && hash_of("foobar") == avalanche(0x85944171f73967e8ull));
    // ---- key and tag
    CHECK(is(key_of("a/1"), hash_of("a"), 1) && is(key_of("a/2"), hash_of("a"), 2));      // exactly 3 bytes: the shortest suffixed id
    CHECK(is(key_of("/1"), hash_of("/1"), 0));                                            // no stem
    CHECK(is(key_of("x/3"), hash_of("x/3"), 0) && is(key_of("x/0"), hash_of("x/0"), 0));
    CHECK(is(key_of("ab"), hash_of("ab"), 0) && is(key_of("a/"), hash_of("a/"), 0) && is(key_of("a"), hash_of("a"), 0) && is(key_of(""), hash_of(""), 0));
    CHECK(is(key_of("S0R4970856/2"), hash_of("S0R4970856"), 2) && is(key_of("a/1/1"), hash_of("a/1"), 1) && is(key_of("//2"), hash_of("/"), 2));
    CHECK(is(key_of(std::string("\0/1", 3)), hash_of(std::string("\0", 1)), 1));         // a NUL is a byte like any other
    CHECK(is(key_of("\xff\xfe/2"), hash_of("\xff\xfe"), 2));                              // bytes above 127 hash as unsigned
    {
        uint64_t key = 5;
        uint8_t tag = 5;
        CHECK(pantax_hip_fragment_key(nullptr, 3, &key, &tag) == PANTAX_HIP_E_INVALID && pantax_hip_fragment_key("a/1", 3, nullptr, &tag) == PANTAX_HIP_E_INVALID &&
              pantax_hip_fragment_key("a/1", 3, &key, nullptr) == PANTAX_HIP_E_INVALID && key == 5 && tag == 5);
    }
    CHECK(FRAG_MAX_LIST == 64 && FRG_N_CLASSES == PANTAX_HIP_FRAGMENT_CLASSES && FRG_N_HAP == 4 && FRG_COUNTED == 0 && FRG_PAIRED == 1 && FRG_CONCORDANT == 2 &&
          FRG_DISCORDANT == 3 && FRG_HALF == 4 && FRG_UNEXPLAINED == 5 && FRG_SINGLE == 6 && FRG_MULTI == 7 && FRG_ELSEWHERE == 8 && FRG_UNIQUE_BY_PAIR == 2 &&
          FRG_ASSIGNED == 3);
    CHECK(PANTAX_HIP_MATE_NONE == 0xFFFFFFFFu && PANTAX_HIP_MATE_AMBIGUOUS == 0xFFFFFFFEu);
    // ---- the report's row in the plan of the file seam: pantax_hip_profile_ext11 behind the 200-byte tenth version
    {
        static_assert(offsetof(pantax_hip_profile_ext11, v10) == 0 && sizeof(pantax_hip_profile_ext10) == 200 && sizeof(pantax_hip_profile_ext9) == 168 &&
                          sizeof(pantax_hip_profile_ext8) == 152 && sizeof(pantax_hip_profile_ext7) == 136 && sizeof(pantax_hip_profile_ext6) == 120 &&
                          sizeof(pantax_hip_profile_ext5) == 88 && sizeof(pantax_hip_profile_ext4) == 64 && sizeof(pantax_hip_profile_ext3) == 48 &&
                          sizeof(pantax_hip_profile_ext2) == 40 && sizeof(pantax_hip_profile_ext) == 16,
                      "the closed versions of the extension keep their sizes");
        static_assert(offsetof(pantax_hip_profile_ext11, strain_fragments_file) == 200 && sizeof(pantax_hip_profile_ext11) == 208, "the eleventh version");
        CHECK(N_EXT11_REPORTS == 1 && EXT11_REPORTS[X11REP_FRAGMENTS].field == &pantax_hip_profile_ext11::strain_fragments_file && EXT11_REPORTS[X11REP_FRAGMENTS].rows);
        CHECK(std::string(EXT11_REPORTS[X11REP_FRAGMENTS].name) == "strain_fragments_file" && std::string(EXT11_REPORTS[X11REP_FRAGMENTS].what) == "fragment support report");
        CHECK(N_EXT10_REPORTS == 1 && N_EXT9_REPORTS == 1 && N_EXT8_REPORTS == 1);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        std::string err;
        pantax_hip_profile_ext11 e11{};
        pantax_hip_profile_ext *e1 = &e11.v10.v9.v8.v7.v6.v5.v4.v3.v2.v1;
        e1->struct_size = sizeof(e11);
        e11.strain_fragments_file = "fr.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(e1, 1, false, rp, err));
        CHECK(rp.ext11_want[X11REP_FRAGMENTS] && !rp.ext11_run[X11REP_FRAGMENTS] && rp.ext11_path[X11REP_FRAGMENTS] == "fr.tsv" && !rp.ext10_want[X10REP_RAREFY]);
        resume_reports(rp, true, true, false);
        CHECK(rp.ext11_run[X11REP_FRAGMENTS] && rp.any_run() && rp.rows_run() && !rp.ext10_run[X10REP_RAREFY]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext11_run[X11REP_FRAGMENTS] && !rp.any_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext11_run[X11REP_FRAGMENTS]);
        resume_reports(rp, true, false, true);                         // the strain-only resume writes it
        CHECK(rp.ext11_run[X11REP_FRAGMENTS]);
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err == "profile: the fragment support report (strain_fragments_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(e1, 1, true, rp, err) &&
              err == "profile: the fragment support report (strain_fragments_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e11.v10.strain_rarefy_file = "rf.tsv";                          // the rarefaction report's refusal comes first
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err.find("strain_rarefy_file") != std::string::npos);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext10_want[X10REP_RAREFY] && rp.ext11_want[X11REP_FRAGMENTS]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes, the rarefaction report on where it is held
        for (const uint64_t size : {16ull, 40ull, 48ull, 64ull, 88ull, 120ull, 136ull, 152ull, 168ull, 176ull, 200ull}) {
            e1->struct_size = size;
            CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext11_want[X11REP_FRAGMENTS] && rp.ext11_path[X11REP_FRAGMENTS].empty());
            CHECK(rp.ext10_want[X10REP_RAREFY] == (size >= 176));
        }
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e1->struct_size = sizeof(e11); e11.strain_fragments_file = off; e11.v10.strain_rarefy_file = nullptr;
            CHECK(plan_ext_reports(e1, 2, true, rp, err) && !rp.ext11_want[X11REP_FRAGMENTS]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext11_want[X11REP_FRAGMENTS]);
    }
    // ---- the ids of the caller
    for (int a = 1; a < argc; ++a) {
        std::string id;
        if (std::strcmp(argv[a], "-") != 0) {
            const size_t n = std::strlen(argv[a]);
            CHECK(n % 2 == 0);
            for (size_t i = 0; i < n; i += 2) {
                const int hi = nibble(argv[a][i]), lo = nibble(argv[a][i + 1]);
                CHECK(hi >= 0 && lo >= 0);
                id.push_back((char)(hi * 16 + lo));
            }
        }
        const KeyTag k = key_of(id);
        CHECK(k.rc == 0);
        std::printf("key %016llx %u\n", (unsigned long long)k.key, (unsigned)k.tag);
    }
    std::printf("fragments_plan_check: ok\n");
    return 0;
}
