// ssn_node_bits_check.cpp -- options node_bits / node_bits_words of the fused node pass (ssn_node_bits, pantax_amd/csrc/ssn_plan.hpp) at their edges:
// which kernel instantiation a pair of values selects, and which pairs are refused.  A program of its own, compiled by tests/test_ssn_node_bits.py with
// the host compiler alone.
#include <cstdio>
#include "ssn_plan.hpp"

using namespace ptx;

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "ssn_node_bits_check:%d: %s\n", __LINE__, #cond); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

int main() {
    CHECK(SSN_NODE_BITS_WORDS == 1 || SSN_NODE_BITS_WORDS == 2);
    // the default, spelled three ways
    CHECK(ssn_node_bits(nullptr, 0) == SSN_NODE_BITS_WORDS);
    CHECK(ssn_node_bits("", 0) == SSN_NODE_BITS_WORDS);
    CHECK(ssn_node_bits("range", 0) == SSN_NODE_BITS_WORDS);
    // words a lane holds
    CHECK(ssn_node_bits("", 1) == 1 && ssn_node_bits("range", 1) == 1);
    CHECK(ssn_node_bits("", 2) == 2 && ssn_node_bits("range", 2) == 2);
    // gather: no stretch is loaded, whatever the (valid) word count
    CHECK(ssn_node_bits("gather", 0) == 0 && ssn_node_bits("gather", 1) == 0 && ssn_node_bits("gather", 2) == 0);
    // refused
    CHECK(ssn_node_bits("", 3) < 0 && ssn_node_bits("", -1) < 0 && ssn_node_bits("gather", 3) < 0);
    CHECK(ssn_node_bits("Range", 0) < 0 && ssn_node_bits("scatter", 0) < 0 && ssn_node_bits("range ", 0) < 0 && ssn_node_bits("split", 1) < 0);
    std::printf("ssn_node_bits_check: ok\n");
    return 0;
}
