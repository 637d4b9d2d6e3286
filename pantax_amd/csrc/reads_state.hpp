// reads_state.hpp -- what resident reads hold beside their columns, as one small state type whose fields change only through named transitions (one per
// event in the host code) and are read only through named queries.  Host only, no HIP: tests/native/reads_state_check.cpp drives it against a
// transcription of the seven flags it replaced.  The states, the events and who raises them: DESIGN.md, "Lifecycle of resident reads".
//
// Derived from the columns (step_off, node_id, pstart, pend, qlen, mapq, flags) are, in the order they are made:
//   the locus-grouped copy   build_step_read: the padded step stream, the slot of every read, {first step, #steps, ...} and {min id, max id} per slot
//   the binning              bin_reads_launch against ONE db: grouped reads keep {species index, node base - first id} of THAT db in their slot records,
//                            ungrouped reads (a slice that will be routed away) the species array in file order
//   the species array        grouped reads: gathered from the slot records on request (species_ensure)
//   the slot-order flags     grouped reads with drop flags: d_g_flag, filed in front of the binning kernel once per change of the flags
//   the long walks' sums     taken by the binning kernel on its way where the db has graphs (else walk_sum_kernel in coverage_prepare)
//
// THE RULE OF THE DROP FLAGS.  The drop flag of a grouped read rides in its slot record (coding: common.hpp, slot_species), which only the binning pass
// writes: a change of the flags reaches the coverage pass of grouped reads only through a binning pass, so flags_replaced voids their binning.  Ungrouped
// reads carry the flag beside the species array (route_pack reads d_flags itself): their binning stands.
#pragma once
#include <cstdint>

namespace ptx {

class ReadsState {
public:
    // ---- queries
    bool has_flags() const { return has_flags_; }                              // d_flags holds a drop flag per read
    bool grouped() const { return grouped_; }                                  // the locus-grouped copy is there, whole
    // the last binning pass finished, ran against the db `uid` (Db::uid, never 0, never reused), and nothing it wrote was replaced since
    bool binned_against(uint64_t uid) const { return uid != 0 && binned_uid_ == uid; }
    bool species_in_file_order() const { return species_file_order_; }         // d_species reflects the last binning pass
    bool slot_flags_current() const { return slot_flags_current_; }            // d_g_flag holds the flags of d_flags
    bool long_sums_from(uint64_t uid) const { return uid != 0 && long_sums_uid_ == uid; }   // d_long_sum / d_long_len0 were filled by the binning pass against `uid`

    // ---- transitions
    // pantax_hip_reads_upload, the device tokenizer, reads_from_routed: new columns are in place, everything derived from them is void
    void columns_replaced(bool has_flags) { *this = ReadsState(); has_flags_ = has_flags; }
    // build_step_read (also through reads_group): the slot arrays are being rewritten -- nothing that lives in them or was read from them is claimed ...
    void layout_begun() { grouped_ = false; void_binning(); slot_flags_current_ = false; }
    void layout_finished() { grouped_ = true; }                                // ... and "grouped" holds only from here on
    // pantax_hip_reads_set_flags, route_reads of the file seam: d_flags was replaced (or dropped).  The rule at the top
    void flags_replaced(bool has_flags) {
        has_flags_ = has_flags; slot_flags_current_ = false;
        if (grouped_) binned_uid_ = 0;
    }
    // bin_reads_launch: between the two events nothing is claimed
    void bin_begun() { void_binning(); }
    void bin_finished(uint64_t uid, bool species_in_file_order, bool long_sums_taken) {
        binned_uid_ = uid; species_file_order_ = species_in_file_order; long_sums_uid_ = long_sums_taken ? uid : 0;
    }
    void slot_flags_filed() { slot_flags_current_ = true; }                    // flags_to_slots_kernel is enqueued
    void species_gathered() { species_file_order_ = true; }                    // species_ensure

private:
    void void_binning() { binned_uid_ = 0; species_file_order_ = false; long_sums_uid_ = 0; }
    bool has_flags_ = false, grouped_ = false, species_file_order_ = false, slot_flags_current_ = false;
    uint64_t binned_uid_ = 0;      // Db::uid of the db the slot records / the species array hold indices of; 0: not binned
    uint64_t long_sums_uid_ = 0;   // Db::uid of the db whose binning pass took the walk sums; 0: nobody (walk_sum_kernel does it)
};

}  // namespace ptx
