// segments_check.cpp -- the host side of pantax_hip_strain_segments at its edges: the stitching of per-tile summaries into runs that cross tile borders and
// the output slot of every kept run (pantax_amd/csrc/segments_plan.hpp), the chain helper on cases done by hand, and the report's row in the plan of the
// file seam.  A program of its own: tests/test_segments_plan.py compiles it with segments_plan.cpp and report_plan.cpp by the host C++ compiler under
// -fsanitize=address,undefined and runs it; it returns non-zero at the first check that fails.
//
// The device's part is played by a CPU summariser of one tile (tile_sum: what segments_tile_kernel writes) and a CPU emitter of a tile's kept interior runs
// (tile_emit: what segments_emit_kernel writes); class strings are cut into tiles of 1, 2, 16 and 1 024 steps and the stitched result is compared with a
// direct run-length pass over the whole walk.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>
#include "../../include/pantax_hip.h"
#include "report_plan.hpp"
#include "segments_plan.hpp"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "segments_check:%d: %s\n", __LINE__, #cond);       \
            return 1;                                                               \
        }                                                                           \
    } while (0)

using namespace ptx;

namespace {

struct Seg {
    uint8_t cls; uint64_t step; uint32_t n_steps; uint64_t start, len, bases;
    bool operator==(const Seg &o) const { return cls == o.cls && step == o.step && n_steps == o.n_steps && start == o.start && len == o.len && bases == o.bases; }
};
struct Walk { std::vector<uint8_t> cls; std::vector<uint32_t> len; std::vector<uint64_t> bases; };
struct Totals {
    uint64_t hap_len = 0, n[2] = {0, 0}, len[2] = {0, 0}, max[2] = {0, 0};
    bool operator==(const Totals &o) const {
        return hap_len == o.hap_len && n[0] == o.n[0] && n[1] == o.n[1] && len[0] == o.len[0] && len[1] == o.len[1] && max[0] == o.max[0] && max[1] == o.max[1];
    }
};

// every run of steps [i0, i1) of one class, in order: f(class, first step, end step)
template <class F> void runs_of(const Walk &w, size_t i0, size_t i1, F f) {
    for (size_t i = i0; i < i1;) {
        size_t j = i;
        while (j < i1 && w.cls[j] == w.cls[i]) ++j;
        f(w.cls[i], i, j);
        i = j;
    }
}
SegPiece piece(const Walk &w, size_t i, size_t j) {
    SegPiece p{0, 0, (uint32_t)(j - i), w.cls[i]};
    for (size_t k = i; k < j; ++k) { p.len += w.len[k]; p.bases += w.bases[k]; }
    return p;
}
// the direct pass: every run of class 1 or 2 counts, those of at least min_len bases are segments
void direct(const Walk &w, uint64_t min_len, std::vector<Seg> &segs, Totals &t) {
    uint64_t o = 0;
    runs_of(w, 0, w.cls.size(), [&](uint8_t c, size_t i, size_t j) {
        const SegPiece p = piece(w, i, j);
        if (c == 1 || c == 2) {
            t.n[c - 1] += 1; t.len[c - 1] += p.len; t.max[c - 1] = std::max(t.max[c - 1], p.len);
            if (p.len >= min_len) segs.push_back(Seg{c, i, p.n_steps, o, p.len, p.bases});
        }
        o += p.len;
    });
    t.hap_len = o;
}
// what the wave of the tile [i0, i1) reports
SegTileSum tile_sum(const Walk &w, size_t i0, size_t i1, uint64_t min_len) {
    SegTileSum s{};
    runs_of(w, i0, i1, [&](uint8_t c, size_t i, size_t j) {
        const SegPiece p = piece(w, i, j);
        s.sum_len += p.len;
        if (i == i0) { s.lead = p; s.whole = j == i1; }
        if (j == i1) s.trail = p;
        if (i != i0 && j != i1 && (c == 1 || c == 2)) {
            s.n[c - 1] += 1; s.len[c - 1] += p.len; s.max[c - 1] = std::max(s.max[c - 1], p.len);
            s.n_keep += p.len >= min_len;
        }
    });
    return s;
}
// ... and what it writes in the second pass, from the place the plan gave it
void tile_emit(const Walk &w, size_t i0, size_t i1, uint64_t min_len, const SegTilePlace &pl, std::vector<Seg> &out, std::vector<uint8_t> &written) {
    uint64_t o = pl.base, slot = pl.out0;
    runs_of(w, i0, i1, [&](uint8_t c, size_t i, size_t j) {
        const SegPiece p = piece(w, i, j);
        if (i != i0 && j != i1 && (c == 1 || c == 2) && p.len >= min_len) {
            out.at(slot) = Seg{c, pl.step0 + (i - i0), p.n_steps, o, p.len, p.bases};
            written.at(slot) += 1;
            ++slot;
        }
        o += p.len;
    });
}
// the walks cut into tiles (walk c begins `lead[c]` steps into a tile of `tile` steps), summarised, planned, emitted: equal to the direct pass?
bool stitched_equals_direct(const std::vector<Walk> &walks, const std::vector<size_t> &lead, size_t tile, uint64_t min_len) {
    const uint64_t C = walks.size();
    std::vector<uint64_t> tile_first(C + 1, 0);
    std::vector<uint32_t> steps;
    std::vector<SegTileSum> sums;
    std::vector<std::pair<size_t, size_t>> span;
    for (uint64_t c = 0; c < C; ++c) {
        const size_t n = walks[c].cls.size();
        for (size_t i = 0; i < n;) {
            const size_t j = std::min(n, i == 0 ? tile - lead[c] % tile : i + tile);
            span.push_back({i, j}); steps.push_back((uint32_t)(j - i)); sums.push_back(tile_sum(walks[c], i, j, min_len));
            i = j;
        }
        tile_first[c + 1] = sums.size();
    }
    std::vector<uint64_t> seg_off(C + 1, 7), hap_len(C, 7), n_runs(2 * C, 7), run_len(2 * C, 7), run_max(2 * C, 7);
    SegPlan plan;
    segments_plan(C, tile_first.data(), steps.data(), sums.data(), min_len, seg_off.data(), hap_len.data(), n_runs.data(), run_len.data(), run_max.data(), plan);
    std::vector<Seg> got(seg_off[C]);
    std::vector<uint8_t> written(seg_off[C], 0);
    for (uint64_t c = 0; c < C; ++c)
        for (uint64_t t = tile_first[c]; t < tile_first[c + 1]; ++t) tile_emit(walks[c], span[t].first, span[t].second, min_len, plan.place[t], got, written);
    for (const SegBorder &b : plan.border) { got.at(b.slot) = Seg{b.cls, b.step, b.n_steps, b.start, b.len, b.bases}; written.at(b.slot) += 1; }
    for (const uint8_t n : written) if (n != 1) return false;   // one writer per slot
    if (seg_off[0] != 0) return false;
    for (uint64_t c = 0; c < C; ++c) {
        std::vector<Seg> exp;
        Totals te, tg;
        direct(walks[c], min_len, exp, te);
        tg.hap_len = hap_len[c];
        for (int k = 0; k < 2; ++k) { tg.n[k] = n_runs[2 * c + k]; tg.len[k] = run_len[2 * c + k]; tg.max[k] = run_max[2 * c + k]; }
        if (!(te == tg) || seg_off[c + 1] - seg_off[c] != exp.size()) return false;
        if (!std::equal(exp.begin(), exp.end(), got.begin() + seg_off[c])) return false;
    }
    return true;
}
Walk walk_of(const std::string &classes, std::mt19937_64 &rng) {
    Walk w;
    for (const char ch : classes) {
        w.cls.push_back((uint8_t)(ch - '0'));
        w.len.push_back(1 + (uint32_t)(rng() % 40));
        w.bases.push_back(ch == '1' ? 0 : rng() % (1ull << 40));
    }
    return w;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261020);
    const size_t TILES[4] = {1, 2, 16, 1024};
    // ---- shapes by hand, at every tile size, begun at the tile's first step and mid-tile
    {
        const std::string hand[] = {
            "1",                                       // a walk of one step
            "0", "2",
            "1111111111111111111111111111111111111",   // every tile a whole run
            "0000000000000000000000000000000000",      // ... of class 0: nothing to report
            "1122",                                    // a gap directly followed by a peak: at tile 2 a lead and a trail of different classes, a class change at the border
            "0110220011",                              // a run that ends exactly at a tile's last step (tile 2: "01|10|22|00|11")
            "1101100111011110",                        // 16 steps: one tile at 16, runs at both ends
            "11011001110111101",                       // 17: a second tile of one step
            "2222222222222222" "2222222222222222" "2222222222222222" "1",   // whole-run tiles, then a change of class at the border
            "0121012101210121012101210121012101",      // runs of one step
        };
        for (const std::string &s : hand)
            for (const size_t tile : TILES)
                for (const size_t lead : {(size_t)0, (size_t)1, tile / 2, tile - 1})
                    for (const uint64_t min_len : {1ull, 20ull, 41ull, 1000ull}) {
                        const Walk w = walk_of(s, rng);
                        CHECK(stitched_equals_direct({w}, {lead}, tile, min_len));
                    }
    }
    // ---- random class strings: short runs, long runs, several walks in one selection, an empty walk among them
    for (int round = 0; round < 400; ++round) {
        const size_t tile = TILES[round % 4];
        std::vector<Walk> walks;
        std::vector<size_t> lead;
        const int C = 1 + (int)(rng() % 3);
        for (int c = 0; c < C; ++c) {
            const size_t n = rng() % 7 == 0 ? 0 : 1 + rng() % (tile == 1024 ? 5000 : 200);
            const unsigned stay = 1 + (unsigned)(rng() % (round % 3 == 0 ? 2000 : 8));   // the mean run length
            std::string s;
            char cur = (char)('0' + rng() % 3);
            for (size_t i = 0; i < n; ++i) {
                if (rng() % stay == 0) cur = (char)('0' + rng() % 3);
                s.push_back(cur);
            }
            walks.push_back(walk_of(s, rng));
            lead.push_back(rng() % tile);
        }
        CHECK(stitched_equals_direct(walks, lead, tile, 1 + rng() % (round % 2 ? 60 : 3)));
    }
    {   // a walk of one tile; a whole run through three tiles is ONE run with the sums of all of them
        Walk w = walk_of(std::string(2600, '1'), rng);
        std::vector<Seg> exp;
        Totals t;
        direct(w, 1, exp, t);
        CHECK(exp.size() == 1 && t.n[0] == 1 && t.max[0] == t.hap_len && exp[0].n_steps == 2600 && exp[0].start == 0);
        CHECK(stitched_equals_direct({w}, {500}, 1024, 1) && stitched_equals_direct({w}, {500}, 1024, t.hap_len) && stitched_equals_direct({w}, {500}, 1024, t.hap_len + 1));
    }
    // ---- the chain helper on the cases done by hand (tests/test_segments_ref.py)
    {
        const uint8_t cls[5] = {1, 1, 2, 1, 1};
        const uint64_t start[5] = {0, 20, 25, 31, 46}, len[5] = {10, 5, 5, 4, 1}, bases[5] = {0, 0, 99, 0, 0};
        const uint32_t n_steps[5] = {1, 2, 1, 1, 1};
        uint8_t cc[5];
        uint64_t first[5], last[5], q[5 * PANTAX_HIP_SEGMENT_CHAIN_N], m = 99;
        CHECK(pantax_hip_segment_chain(5, cls, start, len, n_steps, bases, 10, 0, &m, cc, first, last, q) == 0 && m == 3);
        CHECK(cc[0] == 1 && first[0] == 0 && last[0] == 3 && q[0] == 0 && q[1] == 35 && q[2] == 35 && q[3] == 19 && q[4] == 3 && q[5] == 4 && q[6] == 0);
        CHECK(cc[1] == 2 && first[1] == 2 && last[1] == 2 && q[7] == 25 && q[8] == 30 && q[9] == 5 && q[13] == 99);
        CHECK(cc[2] == 1 && first[2] == 4 && q[14] == 46 && q[15] == 47);
        CHECK(pantax_hip_segment_chain(5, cls, start, len, n_steps, bases, 9, 0, &m, cc, first, last, q) == 0 && m == 4 && q[1] == 10 && q[7] == 20 && q[8] == 35);
        CHECK(pantax_hip_segment_chain(5, cls, start, len, n_steps, bases, 11, 0, &m, cc, first, last, q) == 0 && m == 2 && q[1] == 47 && q[4] == 4);
        CHECK(pantax_hip_segment_chain(5, cls, start, len, n_steps, bases, 0, 0, &m, cc, first, last, q) == 0 && m == 5);
        CHECK(pantax_hip_segment_chain(5, cls, start, len, n_steps, bases, 10, 6, &m, cc, first, last, q) == 0 && m == 1 && q[2] == 35);
        CHECK(pantax_hip_segment_chain(5, cls, start, len, n_steps, bases, 10, 36, &m, cc, first, last, q) == 0 && m == 0);
        CHECK(pantax_hip_segment_chain(0, nullptr, nullptr, nullptr, nullptr, nullptr, 10, 0, &m, nullptr, nullptr, nullptr, nullptr) == 0 && m == 0);
        CHECK(pantax_hip_segment_chain(5, cls, start, len, n_steps, bases, 10, 0, nullptr, cc, first, last, q) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_segment_chain(5, nullptr, start, len, n_steps, bases, 10, 0, &m, cc, first, last, q) == PANTAX_HIP_E_INVALID);
        const uint8_t bad_cls[2] = {1, 3};
        const uint64_t overlap[2] = {0, 9};
        CHECK(pantax_hip_segment_chain(2, bad_cls, start, len, n_steps, bases, 10, 0, &m, cc, first, last, q) == PANTAX_HIP_E_INVALID);
        CHECK(pantax_hip_segment_chain(2, cls, overlap, len, n_steps, bases, 10, 0, &m, cc, first, last, q) == PANTAX_HIP_E_INVALID);
    }
    // ---- the report in the file seam's plan: four fields of pantax_hip_profile_ext6, which begins with the 88-byte fifth version; the one row of EXT6_REPORTS
    {
        static_assert(offsetof(pantax_hip_profile_ext6, v5) == 0 && sizeof(pantax_hip_profile_ext5) == 88 && sizeof(pantax_hip_profile_ext4) == 64 &&
                          sizeof(pantax_hip_profile_ext3) == 48 && sizeof(pantax_hip_profile_ext2) == 40 && sizeof(pantax_hip_profile_ext) == 16,
                      "the earlier versions keep their place and size");
        static_assert(offsetof(pantax_hip_profile_ext6, strain_segments_file) == 88 && offsetof(pantax_hip_profile_ext6, strain_segments_min) == 96 &&
                          offsetof(pantax_hip_profile_ext6, strain_segments_bridge) == 104 && offsetof(pantax_hip_profile_ext6, strain_segments_peak) == 112 &&
                          sizeof(pantax_hip_profile_ext6) == 120,
                      "appended behind them");
        CHECK(N_EXT6_REPORTS == 1 && EXT6_REPORTS[X6REP_SEGMENTS].field == &pantax_hip_profile_ext6::strain_segments_file && EXT6_REPORTS[X6REP_SEGMENTS].rows);
        CHECK(std::string(EXT6_REPORTS[X6REP_SEGMENTS].name) == "strain_segments_file" && std::string(EXT6_REPORTS[X6REP_SEGMENTS].what) == "segment report");
        CHECK(N_EXT5_REPORTS == 1 && N_EXT4_REPORTS == 1 && N_EXT3_REPORTS == 1 && N_EXT2_REPORTS == 1 && N_EXT_REPORTS == 1);
        const pantax_hip_profiling_config cfg{};
        ReportPlan rp;
        std::string err;
        pantax_hip_profile_ext6 e6{};
        pantax_hip_profile_ext *e1 = &e6.v5.v4.v3.v2.v1;
        e1->struct_size = sizeof(e6);
        e6.strain_segments_file = "seg.tsv";
        CHECK(plan_reports(&cfg, 1, false, rp, err) && plan_ext_reports(e1, 1, false, rp, err));
        CHECK(rp.ext6_want[X6REP_SEGMENTS] && !rp.ext6_run[X6REP_SEGMENTS] && rp.ext6_path[X6REP_SEGMENTS] == "seg.tsv" && !rp.ext5_want[X5REP_EM]);
        CHECK(rp.sg_min == 1000 && rp.sg_bridge == 100 && rp.sg_peak == 10);
        resume_reports(rp, true, true, false);
        CHECK(rp.ext6_run[X6REP_SEGMENTS] && rp.any_run() && rp.rows_run() && !rp.ext5_run[X5REP_EM]);
        resume_reports(rp, true, true, true);
        CHECK(!rp.ext6_run[X6REP_SEGMENTS] && !rp.any_run());
        resume_reports(rp, false, true, false);
        CHECK(!rp.ext6_run[X6REP_SEGMENTS]);
        e6.strain_segments_min = 1; e6.strain_segments_bridge = 1; e6.strain_segments_peak = 3;          // the bridge field holds bridge + 1: an explicit 0
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.sg_min == 1 && rp.sg_bridge == 0 && rp.sg_peak == 3);
        e6.strain_segments_min = ~0ull; e6.strain_segments_bridge = ~0ull; e6.strain_segments_peak = PANTAX_HIP_SEGMENTS_PEAK_OFF;   // peaks off
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.sg_min == ~0ull && rp.sg_bridge == ~0ull - 1 && rp.sg_peak == 0);
        e6.strain_segments_min = 7; e6.strain_segments_bridge = 8; e6.strain_segments_peak = 9;
        e1->struct_size = 96;                                          // a struct that holds the file alone: the defaults
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext6_want[X6REP_SEGMENTS] && rp.sg_min == 1000 && rp.sg_bridge == 100 && rp.sg_peak == 10);
        e1->struct_size = 104;                                         // ... the file and the minimum
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.sg_min == 7 && rp.sg_bridge == 100 && rp.sg_peak == 10);
        e1->struct_size = 112;                                         // ... and the bridge
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.sg_min == 7 && rp.sg_bridge == 7 && rp.sg_peak == 10);
        e1->struct_size = sizeof(e6);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.sg_min == 7 && rp.sg_bridge == 7 && rp.sg_peak == 9);
        e6.strain_segments_min = e6.strain_segments_bridge = e6.strain_segments_peak = 0;
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err == "profile: the segment report (strain_segments_file) needs one rank and an unsharded ingest (world_size 2)");
        CHECK(!plan_ext_reports(e1, 1, true, rp, err) && err == "profile: the segment report (strain_segments_file) needs one rank and an unsharded ingest (world_size 1, sharded)");
        e6.v5.strain_em_file = "em.tsv";                               // the read class report's refusal comes first
        CHECK(!plan_ext_reports(e1, 2, false, rp, err) && err.find("strain_em_file") != std::string::npos);
        CHECK(plan_ext_reports(e1, 1, false, rp, err) && rp.ext5_want[X5REP_EM] && rp.ext6_want[X6REP_SEGMENTS]);
        // a caller with an earlier version: the report is off whatever lies behind its bytes, the read class report on where it is held
        for (const uint64_t size : {16ull, 40ull, 48ull, 64ull, 72ull, 88ull}) {
            e1->struct_size = size;
            CHECK(plan_ext_reports(e1, 1, false, rp, err) && !rp.ext6_want[X6REP_SEGMENTS] && rp.ext6_path[X6REP_SEGMENTS].empty() && rp.sg_min == 1000 && rp.sg_bridge == 100);
            CHECK(rp.ext5_want[X5REP_EM] == (size >= 72));
        }
        for (const char *off : {(const char *)nullptr, "", "None"}) {
            e1->struct_size = sizeof(e6); e6.strain_segments_file = off; e6.v5.strain_em_file = nullptr;
            CHECK(plan_ext_reports(e1, 2, true, rp, err) && !rp.ext6_want[X6REP_SEGMENTS]);
        }
        CHECK(plan_ext_reports(nullptr, 1, false, rp, err) && !rp.ext6_want[X6REP_SEGMENTS]);
    }
    std::printf("segments_check: ok\n");
    return 0;
}
