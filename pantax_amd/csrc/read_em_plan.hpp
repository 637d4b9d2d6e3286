// read_em_plan.hpp -- the host decisions of pantax_hip_strain_read_em (stage_read_em.hip) as pure functions of plain values: how many slots the class
// table of a species gets, how a table that overflowed grows, which classes of a species the report prints.  The host helper of the contract
// (pantax_hip_read_em) is defined in read_em_plan.cpp beside them.  pantax_hip.h and standard headers only: tests/native/read_em_check.cpp compiles this
// with the host compiler alone.
#pragma once
#include <cstdint>
#include <vector>

namespace ptx {

constexpr uint64_t READ_EM_MAX_K = 64;                 // candidates of a species whose classes fit one mask word; more: the species is skipped
constexpr uint64_t READ_CLASS_SLOTS_DEFAULT = 2048;    // option read_class_slots = 0
constexpr uint32_t READ_EM_LDS_CLASSES = 2048;         // classes whose (mask, r) the estimate keeps in LDS (option read_em_lds_classes = 0)

// the smallest power of two >= n (n <= 2^63; 0 and 1 give 1)
constexpr uint64_t read_class_pow2(uint64_t n) {
    uint64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
// non-zero masks over K candidates, cut to 2^62 (K >= 62: more than any table holds)
constexpr uint64_t read_class_masks(uint64_t K) { return K == 0 ? 0 : (K >= 62 ? (1ull << 62) : (1ull << K) - 1); }
// Slots of the open-addressed class table of a species of K candidates on the first pass: the power of two >= 2 min(2^K - 1, opt), opt = the option
// read_class_slots (0: 2048; cut to 2^31).  K = 0 and K > 64 own no table.  At most half full while the species has no more than min(..) classes.
constexpr uint64_t read_class_slots(uint64_t K, uint64_t opt) {
    const uint64_t o = opt == 0 ? READ_CLASS_SLOTS_DEFAULT : (opt > (1ull << 31) ? (1ull << 31) : opt);
    const uint64_t m = read_class_masks(K);
    return (K == 0 || K > READ_EM_MAX_K) ? 0 : read_class_pow2(2 * (m < o ? m : o));
}
// The bound of the growth: a species of K candidates and `counted` counted reads has at most min(2^K - 1, counted) classes, so a table of
// read_class_slots_bound slots (twice that, rounded up) always has a free slot on every probe sequence: overflow is impossible there.
constexpr uint64_t read_class_slots_bound(uint64_t K, uint64_t counted) {
    const uint64_t m = read_class_masks(K), c = counted > (1ull << 62) ? (1ull << 62) : (counted ? counted : 1);
    return (K == 0 || K > READ_EM_MAX_K) ? 0 : read_class_pow2(2 * (m < c ? m : c));
}
// A species whose table of `slots` slots overflowed is rerun with 8 times the slots, at most the bound (and never fewer than it had: slots >= bound
// cannot overflow, the caller treats it as an internal error).  Eightfold per rerun up to the bound: the loop of reruns is bounded by log8 of the bound,
// and since the last table cannot overflow the result is never truncated.
constexpr uint64_t read_class_grow(uint64_t slots, uint64_t K, uint64_t counted) {
    const uint64_t bound = read_class_slots_bound(K, counted);
    const uint64_t next = slots > (bound >> 3) ? bound : slots * 8;
    return next > slots ? next : slots;
}

// The classes of a species the report prints: the first min(J, N) by span descending, ties by mask ascending; their indices into the species' classes
// (which are in ascending mask) in print order.
std::vector<uint64_t> read_class_rank(uint64_t J, const uint64_t *mask, const uint64_t *span, uint64_t N);

}  // namespace ptx
