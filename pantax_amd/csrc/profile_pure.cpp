// profile_pure.cpp -- the decisions of the file seam that need no ctx, no HIP call and no file: plain values in, plain values out (profile_run.hpp)
#include <algorithm>
#include <cmath>
#include "profile_pure.hpp"

namespace ptx {
bool species_wanted(int mode, const std::set<std::string> &designated, const RangeRow &row) {
    if ((mode == 0 && row.is_pan != 0) || (mode == 1 && row.is_pan != 1)) return false;
    return designated.empty() || designated.count(row.species) != 0;
}
// every rank computes the same table from the same inputs
std::vector<int> lpt_owner(const std::vector<double> &weight, int W) {
    std::vector<int> owner(weight.size(), 0);
    if (W <= 1) return owner;
    std::vector<uint32_t> by_weight(weight.size());
    std::vector<double> load(W, 0.0);
    for (uint32_t i = 0; i < by_weight.size(); ++i) by_weight[i] = i;
    std::stable_sort(by_weight.begin(), by_weight.end(), [&](uint32_t a, uint32_t b) { return weight[a] > weight[b]; });
    for (uint32_t i : by_weight) {
        int r = 0;
        for (int q = 1; q < W; ++q) if (load[q] < load[r]) r = q;
        owner[i] = r; load[r] += weight[i];
    }
    return owner;
}
// A resident db addresses its path steps with 32 bits: a selection beyond steps_max (3e9, not 2^32: the visit table's 32-bit slots hold pads too, a fifth more at
// fifty strains per species) is cut into contiguous groups of species that go through the device one after the other (species are independent from a4 on,
// profile.rs:3297-3319).  The groups also let group g + 1 travel on the loader thread beside the work on group g: 2e8 path steps and more are cut into four
// groups even when one db could hold them (db_groups: 1 = one db, n = that many, 0 = by size).  Balanced: ceil(total / limit) groups, each filled to total / groups.
std::vector<std::pair<uint32_t, uint32_t>> cut_groups(const std::vector<uint64_t> &steps_of, const std::vector<uint64_t> &nodes_of, uint64_t steps_max, int db_groups) {
    const uint32_t Su = (uint32_t)steps_of.size();
    uint64_t steps_total = 0;
    for (uint64_t ps : steps_of) steps_total += ps;
    uint64_t n_groups = std::max<uint64_t>(1, (steps_total + steps_max - 1) / steps_max);
    if (db_groups > 0) n_groups = std::max<uint64_t>(n_groups, (uint64_t)db_groups);
    else if (steps_total >= 200000000ull && Su >= 8) n_groups = std::max<uint64_t>(n_groups, 4);
    n_groups = std::min<uint64_t>(n_groups, Su);
    std::vector<std::pair<uint32_t, uint32_t>> groups;
    uint64_t cum = 0;                                  // path steps of the groups cut so far
    for (uint32_t k0 = 0; k0 < Su;) {
        uint32_t k1 = k0;
        uint64_t steps = 0, nodes = 0;
        // the group ends where the running total comes closest to its share of the whole ((g + 1) / n of the steps): even groups, and the last of the n
        // takes whatever is left -- no small one behind it (the hard limits still cut: 32-bit path steps and node indices of one db)
        const uint64_t boundary = groups.size() + 1 >= n_groups ? ~0ull : (uint64_t)((double)steps_total * (double)(groups.size() + 1) / (double)n_groups);
        while (k1 < Su) {
            const uint64_t ps = steps_of[k1];
            if (k1 > k0 && (steps + ps > steps_max || nodes + nodes_of[k1] > 0xF0000000ull || (boundary != ~0ull && cum + steps + ps / 2 > boundary))) break;
            steps += ps; nodes += nodes_of[k1]; ++k1;
        }
        cum += steps;
        groups.emplace_back(k0, k1);
        k0 = k1;
    }
    return groups;
}
bool mixed_ids(const std::vector<uint64_t> &kh, const std::vector<uint64_t> &kv, std::vector<uint64_t> &mixed) {
    const uint64_t n = kh.size();
    bool dup_any = false;
    for (uint64_t i = 0; i < n;) {
        uint64_t j = i;
        int64_t sp0 = -1;
        bool mix = false;
        for (; j < n && kh[j] == kh[i]; ++j) {
            if (!(kv[j] >> 32)) continue;                       // incomplete rows take no part in the species set
            const int64_t spj = (int64_t)(uint32_t)kv[j];
            if (sp0 < 0) sp0 = spj; else if (spj != sp0) mix = true;
        }
        if (j - i > 1) dup_any = true;
        if (mix) mixed.push_back(kh[i]);
        i = j;
    }
    return dup_any;
}
static std::string cell(bool has, double v, bool rnd) { return has ? fmt_f64(rnd ? std::round(v * 100.0) / 100.0 : v) : std::string(); }
std::string strain_row_text(const std::string &species, const GenomeRow *gr, const pantax_hip_hap_metrics &m, double abund, bool has_abund, bool rnd) {
    std::string s = species;
    s += '\t'; if (gr) s += gr->strain_taxid;
    s += '\t'; if (gr) s += gr->genome_id;
    s += '\t' + cell(m.has & PANTAX_HIP_HAS_SECOND, m.second_sol, rnd);
    s += '\t' + (has_abund ? fmt_f64(abund) : std::string());
    s += '\t' + cell(m.has & PANTAX_HIP_HAS_RATIO, m.path_cov_ratio, rnd);
    s += '\t' + cell(m.has & PANTAX_HIP_HAS_FRACTION, m.unique_trio_nodes_fraction, rnd);
    s += '\t' + cell(m.has & PANTAX_HIP_HAS_FREQ_MEAN, m.frequencies_mean, rnd);
    s += '\t' + cell(m.has & PANTAX_HIP_HAS_FIRST, m.first_sol, rnd);
    s += '\t' + cell(m.has & PANTAX_HIP_HAS_DIVERGENCE, m.divergence, rnd);
    s += '\t' + cell(m.has & PANTAX_HIP_HAS_TOTAL_DIFF, m.total_cov_diff, rnd);
    return s;
}
const char *near_miss_stage(const pantax_hip_hap_metrics &m) {
    if (!(m.has & PANTAX_HIP_HAS_FIRST)) return "first_filter";
    return (m.has & PANTAX_HIP_HAS_SECOND) ? "table_filter" : "second_filter";   // (a survivor the highs semantics leave without a second_sol counts with the second filter)
}
std::string near_miss_row_text(const std::string &species, const GenomeRow *gr, const pantax_hip_hap_metrics *m, uint32_t rank, const char *cls, const uint64_t *q,
                               bool with_share, uint64_t orphan_bases) {
    const auto metric = [m](uint32_t bit, double v) { return m && (m->has & bit) ? fmt_f64(v) : std::string("-"); };
    std::string s = species;
    if (m) {
        s += '\t'; if (gr) s += gr->strain_taxid;
        s += '\t'; if (gr) s += gr->genome_id;
        s += '\t' + std::to_string(rank);
    } else s += "\t-\t-\t-";
    s += '\t'; s += cls;
    for (int i = 0; i < 4; ++i) s += '\t' + std::to_string(q[i]);
    if (q[1]) s += '\t' + fmt_f64((double)q[3] / (double)q[1]) + '\t' + fmt_f64((double)q[2] / (double)q[1]);
    else s += "\t-\t-";
    s += '\t' + (with_share && orphan_bases ? fmt_f64((double)q[3] / (double)orphan_bases) : std::string("-"));
    s += '\t'; s += m ? near_miss_stage(*m) : "-";
    s += '\t' + metric(PANTAX_HIP_HAS_FRACTION, m ? m->unique_trio_nodes_fraction : 0.0);
    s += '\t' + metric(PANTAX_HIP_HAS_FREQ_MEAN, m ? m->frequencies_mean : 0.0);
    s += '\t' + metric(PANTAX_HIP_HAS_FIRST, m ? m->first_sol : 0.0);
    s += '\t' + metric(PANTAX_HIP_HAS_SECOND, m ? m->second_sol : 0.0);
    return s;
}
const char *hap_pair_class(uint64_t only_a_len, uint64_t only_b_len) {
    return only_a_len == 0 && only_b_len == 0 ? "identical" : (only_a_len == 0 || only_b_len == 0) ? "nested" : "distinct";
}

}  // namespace ptx
