// profile_reports.cpp -- the per-strain reports of the file seam (profile_reports.hpp): per group of species, behind its strain step, the group's rows of
// strain_abundance.txt are selected once (GroupSel) and every running report takes from the device what it needs; behind the tables every running report
// writes its file.  begin, collect_group and write at the end are the three places that name the reports.  The pair evidence report
// (PAIR_REPORTS of report_plan.hpp) is about pairs of rows and is collected and written the same way; so are the model fit report, the bootstrap report, the leave-one-out
// report, the add-one report, the read class report, the segment report, the mosaic read report, the read rescue report, the link support report, the rarefaction report, the fragment support report and the replication index report, whose files are named in the seam's sized extension (EXT_REPORTS .. EXT12_REPORTS).
#include <algorithm>
#include <cmath>
#include <fstream>
#include <thread>
#include <unordered_map>
#include "fragments_plan.hpp"
#include "hap_pairs_plan.hpp"
#include "links_plan.hpp"
#include "mosaic_plan.hpp"
#include "profile_run.hpp"
#include "read_em_plan.hpp"
#include "rescue_plan.hpp"

namespace ptx {
namespace {
constexpr size_t EVIDENCE_N = 4, DEPTH_N = 2 * PANTAX_HIP_DEPTH_BINS;   // u64 per class: {n_nodes, len, covered, bases}; a histogram of [96]{n_nodes, len}
constexpr size_t FIT_N = 8;   // {n_nodes, len, bases, expected, excess, deficit, blind_nodes, blind_expected}
// The group's rows of strain_abundance.txt, decided in the group's own turn (the a15 filter is row-local) and read by every report: `pass` as bits over
// the shard's haplotypes; per species of the group [off[k - k0], off[k - k0 + 1]) the species-local haplotypes `hap` in ascending order with their
// second_sol weights `w`; the i-th of them is entry entry0 + i of ReportData
struct GroupSel { std::vector<uint8_t> pass; std::vector<uint64_t> off; std::vector<uint32_t> hap; std::vector<double> w; size_t entry0 = 0; };
int group_select(Run &run, uint32_t k0, uint32_t k1, ShardResult &sh, GroupSel &g) {
    const uint32_t Sg = k1 - k0;
    std::vector<uint8_t> rep_g(Sg);
    for (uint32_t k = k0; k < k1; ++k) rep_g[k - k0] = (sh.info[k].status1 == 0 && sh.info[k].status2 == 0) ? 1 : 0;
    g.pass.assign(sh.hap_names.size() ? sh.hap_names.size() : 1, 0);
    PTX_TRY(pantax_hip_abundance_filter(Sg, sh.hap_off.data() + k0, sh.met.data(), rep_g.data(), run.cfg->single_cov_diff, run.cfg->min_cov, g.pass.data(), nullptr, nullptr, nullptr, nullptr));
    g.off.assign(Sg + 1, 0);
    g.entry0 = sh.rep.n_entries;
    for (uint32_t k = k0; k < k1; ++k) {
        for (uint64_t h = sh.hap_off[k]; h < sh.hap_off[k + 1]; ++h)
            if (g.pass[h]) { sh.rep.entry[h] = (int64_t)(g.entry0 + g.hap.size()); g.hap.push_back((uint32_t)(h - sh.hap_off[k])); g.w.push_back(sh.met[h].second_sol); }
        g.off[k - k0 + 1] = g.hap.size();
    }
    sh.rep.n_entries += g.hap.size();
    return 0;
}
// --read-strains: the candidates of every read are the rows of its species
int group_read_strains(Run &run, const Ingest &in, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    const uint64_t R = in.R;
    const pantax_hip_read_strain_set cs{k1 - k0, g.off.data(), g.hap.data(), g.w.data()};
    constexpr int32_t UNTOUCHED = -3;   // entries of reads outside this group's species keep it
    std::vector<uint32_t> t_hap(R, 0u);
    std::vector<int32_t> t_n(R, UNTOUCHED), g_sp(R, -1);
    std::vector<double> t_post(R, 0.0);
    PTX_TRY(pantax_hip_read_strains(run.ctx, db, in.reads.rd, &cs, t_hap.data(), t_n.data(), t_post.data()));
    if (R) {   // the group-local species of every read (the slot records of this group's binning pass)
        PTX_TRY(species_ensure(run.ctx, in.reads.rd));
        PTX_TRY(download(run.ctx, g_sp.data(), in.reads.rd->d_species.p, R));
        PTX_HIP(run.ctx, hipStreamSynchronize(run.ctx->stream));
    }
    auto &rs = sh.rep.rs;
    for (uint64_t r = 0; r < R; ++r) {
        if (t_n[r] == UNTOUCHED) continue;
        rs.n[r] = t_n[r]; rs.post[r] = t_post[r];
        rs.hap[r] = t_n[r] > 0 && g_sp[r] >= 0 ? sh.hap_off[k0 + (uint32_t)g_sp[r]] + t_hap[r] : ~0ull;
    }
    run.lap("  read strains");
    return 0;
}
// --strain-coverage, while the coverage result of the group is still on the device: the windows of the group's rows
int group_cov_track(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &ct = sh.rep.ct;
    const pantax_hip_cov_track_set set{k1 - k0, g.off.data(), g.hap.data(), run.p.rep.ct_window};
    std::vector<uint64_t> w_off(g.hap.size() + 1, 0);
    const int rc_size = pantax_hip_strain_cov_track(run.ctx, db, &set, w_off.data(), 0, nullptr, nullptr, nullptr, nullptr);   // sizes: E_LIMIT unless there is no window
    if (rc_size != 0 && rc_size != PANTAX_HIP_E_LIMIT) return rc_size;
    const uint64_t n = w_off[g.hap.size()], at = ct.len.size();
    ct.n_nodes.resize(at + n); ct.len.resize(at + n); ct.covered.resize(at + n); ct.bases.resize(at + n);
    if (n) PTX_TRY(pantax_hip_strain_cov_track(run.ctx, db, &set, w_off.data(), n, ct.n_nodes.data() + at, ct.len.data() + at, ct.covered.data() + at, ct.bases.data() + at));
    for (size_t e = 0; e < g.hap.size(); ++e) ct.win_off.push_back(at + w_off[e + 1]);
    run.lap("  strain coverage track");
    return 0;
}
// --strain-growth, beside the coverage track and on the same rows: the own-node windows of the group's rows (the fit is the writer's)
int group_growth(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &gr = sh.rep.gr;
    const pantax_hip_cov_track_set set{k1 - k0, g.off.data(), g.hap.data(), run.p.rep.gr_window};
    std::vector<uint64_t> w_off(g.hap.size() + 1, 0);
    const int rc_size = pantax_hip_strain_growth(run.ctx, db, &set, w_off.data(), 0, nullptr, nullptr, nullptr, nullptr);   // sizes: E_LIMIT unless there is no window
    if (rc_size != 0 && rc_size != PANTAX_HIP_E_LIMIT) return rc_size;
    const uint64_t n = w_off[g.hap.size()], at = gr.len.size();
    std::vector<uint32_t> n_own(n);   // (the report prints no step counts)
    gr.len.resize(at + n); gr.len_own.resize(at + n); gr.bases_own.resize(at + n);
    if (n) PTX_TRY(pantax_hip_strain_growth(run.ctx, db, &set, w_off.data(), n, n_own.data(), gr.len.data() + at, gr.len_own.data() + at, gr.bases_own.data() + at));
    for (size_t e = 0; e < g.hap.size(); ++e) gr.win_off.push_back(at + w_off[e + 1]);
    run.lap("  strain growth");
    return 0;
}
// --strain-segments, beside the coverage track and on the same rows: peak_depth = max(2, ceil(F x second_sol)) clamped at 2^31 (0 with peaks off); the device
// is asked for the seeds of min(min_span, bridge + 1) bases, which the writer chains
int group_segments(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &sg = sh.rep.sg;
    const ReportPlan &plan = run.p.rep;
    const size_t C = g.hap.size(), e0 = g.entry0;
    sg.peak.resize(e0 + C); sg.hap_len.resize(e0 + C); sg.n_runs.resize(2 * (e0 + C)); sg.run_len.resize(2 * (e0 + C)); sg.run_max.resize(2 * (e0 + C));
    for (size_t c = 0; c < C; ++c) {
        const double v = std::ceil((double)plan.sg_peak * g.w[c]);
        sg.peak[e0 + c] = plan.sg_peak == 0 ? 0 : !(v >= 2.0) ? 2 : v >= 2147483648.0 ? 1ull << 31 : (uint64_t)v;
    }
    const uint64_t seed = plan.sg_bridge == ~0ull ? plan.sg_min : std::min(plan.sg_min, plan.sg_bridge + 1);
    const pantax_hip_segment_set set{k1 - k0, g.off.data(), g.hap.data(), sg.peak.data() + e0, seed};
    std::vector<uint64_t> s_off(C + 1, 0);
    const int rc_size = pantax_hip_strain_segments(run.ctx, db, &set, s_off.data(), 0, sg.hap_len.data() + e0, sg.n_runs.data() + 2 * e0, sg.run_len.data() + 2 * e0,
                                                   sg.run_max.data() + 2 * e0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);   // sizes: E_LIMIT unless there is no segment
    if (rc_size != 0 && rc_size != PANTAX_HIP_E_LIMIT) return rc_size;
    const uint64_t n = s_off[C], at = sg.len.size();
    sg.cls.resize(at + n); sg.step.resize(at + n); sg.n_steps.resize(at + n); sg.start.resize(at + n); sg.len.resize(at + n); sg.bases.resize(at + n);
    if (n) PTX_TRY(pantax_hip_strain_segments(run.ctx, db, &set, s_off.data(), n, sg.hap_len.data() + e0, sg.n_runs.data() + 2 * e0, sg.run_len.data() + 2 * e0,
                                              sg.run_max.data() + 2 * e0, sg.cls.data() + at, sg.step.data() + at, sg.n_steps.data() + at, sg.start.data() + at,
                                              sg.len.data() + at, sg.bases.data() + at));
    for (size_t e = 0; e < C; ++e) sg.seg_off.push_back(at + s_off[e + 1]);
    run.lap("  strain segments");
    return 0;
}
// --strain-evidence and --strain-depth, on the same coverage result: Sel_s = the group's rows; `call` writes n_hap u64 per entry and n_species per species
int group_node_sums(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, decltype(&pantax_hip_strain_evidence) call, size_t n_hap, size_t n_species, ReportData::NodeSums &out, const char *lap) {
    const pantax_hip_evidence_set set{k1 - k0, g.off.data(), g.hap.data()};
    out.hap.resize(n_hap * (g.entry0 + g.hap.size()));
    PTX_TRY(call(run.ctx, db, &set, out.hap.data() + n_hap * g.entry0, out.species.data() + n_species * (size_t)k0));
    run.lap(lap);
    return 0;
}
// --strain-fit, on the same coverage result: Sel_s = the group's rows, their weights the unrounded second_sol
int group_fit(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &ft = sh.rep.ft;
    const pantax_hip_fit_set set{k1 - k0, g.off.data(), g.hap.data(), g.w.data()};
    ft.hap.resize(2 * FIT_N * (g.entry0 + g.hap.size()));
    PTX_TRY(pantax_hip_strain_fit(run.ctx, db, &set, ft.hap.data() + 2 * FIT_N * g.entry0, ft.species.data() + 3 * FIT_N * (size_t)k0));
    run.lap("  strain fit");
    return 0;
}
// --strain-bootstrap, on the same coverage result: Sel_s = the group's rows (column = position: ascending haplotype), sp_key = the species taxid
uint64_t taxid_key(const std::string &taxid) {
    uint64_t v = 0;
    bool number = !taxid.empty() && taxid.size() <= 19;
    for (const char c : taxid) { if (c < '0' || c > '9') { number = false; break; } v = v * 10 + (uint64_t)(c - '0'); }
    if (number) return v;
    uint64_t h = 0xCBF29CE484222325ull;   // a taxid that is no number: FNV-1a of its text
    for (const char c : taxid) { h ^= (unsigned char)c; h *= 0x100000001B3ull; }
    return h;
}
int group_bootstrap(Run &run, const Ingest &in, const Selection &sn, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &bs = sh.rep.bs;
    const uint32_t Sg = k1 - k0;
    const uint64_t R = bs.R, Cg = g.hap.size();
    std::vector<uint64_t> key(Sg);
    for (uint32_t k = k0; k < k1; ++k) key[k - k0] = taxid_key(in.ranges[sn.sel[sh.use[k]]].species);
    const pantax_hip_bootstrap_set set{Sg, g.off.data(), g.hap.data(), key.data(), run.p.rep.bs_seed, run.p.rep.bs_replicates};
    std::vector<double> x(R * Cg), obj(R * Sg);
    std::vector<uint64_t> rows(R * Sg);
    std::vector<int32_t> status(R * Sg);
    PTX_TRY(pantax_hip_strain_bootstrap(run.ctx, db, &set, x.data(), obj.data(), rows.data(), status.data()));
    bs.x.resize(R * (g.entry0 + Cg));
    for (uint64_t b = 0; b < R; ++b) {   // replicate-major -> the R values of an entry, of a species side by side
        for (uint64_t c = 0; c < Cg; ++c) bs.x[R * (g.entry0 + c) + b] = x[b * Cg + c];
        for (uint32_t k = 0; k < Sg; ++k) {
            bs.obj[R * (k0 + k) + b] = obj[b * Sg + k]; bs.rows[R * (k0 + k) + b] = rows[b * Sg + k]; bs.status[R * (k0 + k) + b] = status[b * Sg + k];
        }
    }
    run.lap("  strain bootstrap");
    return 0;
}
// --strain-rarefy, on the same coverage result and the resident reads: Sel_s = the group's rows (column = position: ascending haplotype)
int group_rarefy(Run &run, const Ingest &in, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &rf = sh.rep.rf;
    const uint32_t Sg = k1 - k0;
    const uint64_t E = rf.E, Cg = g.hap.size();
    const pantax_hip_rarefy_set set{Sg, g.off.data(), g.hap.data(), run.p.rep.rf_seed, run.p.rep.rf_levels, run.p.rep.rf_replicates};
    std::vector<double> x(E * Cg), obj(E * Sg);
    std::vector<uint64_t> rows(E * Sg), reads(2 * E * Sg), member(2 * E * Cg);
    std::vector<int32_t> status(E * Sg);
    PTX_TRY(pantax_hip_strain_rarefy(run.ctx, db, in.reads.rd, &set, x.data(), obj.data(), rows.data(), status.data(), reads.data(), member.data()));
    rf.x.resize(E * (g.entry0 + Cg)); rf.member.resize(2 * E * (g.entry0 + Cg));
    for (uint64_t e = 0; e < E; ++e) {   // entry-major -> the E values of a selection entry, of a species side by side
        for (uint64_t c = 0; c < Cg; ++c) {
            rf.x[E * (g.entry0 + c) + e] = x[e * Cg + c];
            for (int j = 0; j < 2; ++j) rf.member[2 * (E * (g.entry0 + c) + e) + j] = member[2 * (e * Cg + c) + j];
        }
        for (uint32_t k = 0; k < Sg; ++k) {
            const uint64_t at = E * (k0 + k) + e;
            rf.obj[at] = obj[e * Sg + k]; rf.rows[at] = rows[e * Sg + k]; rf.status[at] = status[e * Sg + k];
            for (int j = 0; j < 2; ++j) rf.reads[2 * at + j] = reads[2 * (e * Sg + k) + j];
        }
    }
    run.lap("  strain rarefaction");
    return 0;
}
// --strain-dropout, on the same coverage result: Sel_s = the group's rows (column = position: ascending haplotype)
int group_dropout(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &dr = sh.rep.dr;
    const uint32_t Sg = k1 - k0;
    const uint64_t Cg = g.hap.size(), Q = Cg + Sg;
    uint64_t X = 0;
    for (uint32_t k = 0; k < Sg; ++k) { const uint64_t K = g.off[k + 1] - g.off[k]; X += (K + 1) * K; }
    const pantax_hip_evidence_set set{Sg, g.off.data(), g.hap.data()};
    std::vector<double> x(X ? X : 1), obj(Q);
    std::vector<int32_t> status(Q);
    std::vector<uint64_t> rows(Sg), cnt(4 * Q);
    PTX_TRY(pantax_hip_strain_dropout(run.ctx, db, &set, x.data(), obj.data(), status.data(), rows.data(), cnt.data()));
    const size_t n = g.entry0 + Cg;
    dr.refit.resize(n); dr.obj_without.resize(n); dr.gain.resize(n); dr.shift.resize(n); dr.cnt.resize(4 * n); dr.st.resize(n); dr.sub.resize(n);
    uint64_t x0 = 0;
    for (uint32_t k = 0; k < Sg; ++k) {
        const uint64_t c0 = g.off[k], K = g.off[k + 1] - c0, q0 = c0 + k;
        dr.rows[k0 + k] = rows[k]; dr.obj[k0 + k] = obj[q0]; dr.status[k0 + k] = status[q0]; dr.K[k0 + k] = (uint32_t)K;
        for (uint64_t j = 0; j < K; ++j) {
            const size_t e = g.entry0 + c0 + j;
            const double *xf = x.data() + x0, *xd = xf + (j + 1) * K;
            double o[3] = {-1.0, 0.0, 0.0};
            if (K <= 64) PTX_TRY(pantax_hip_dropout_substitute((uint32_t)K, (uint32_t)j, xf, xd, o));
            dr.refit[e] = xf[j]; dr.obj_without[e] = obj[q0 + 1 + j]; dr.st[e] = status[q0 + 1 + j];
            std::copy(cnt.begin() + 4 * (q0 + 1 + j), cnt.begin() + 4 * (q0 + 1 + j) + 4, dr.cnt.begin() + 4 * e);
            dr.sub[e] = o[0] < 0 ? -1 : (int64_t)(g.entry0 + c0 + (uint64_t)o[0]); dr.gain[e] = o[1]; dr.shift[e] = o[2];
        }
        x0 += (K + 1) * K;
    }
    run.lap("  strain dropout");
    return 0;
}
// --strain-pair-evidence, on the same coverage result: Sel_s = the group's rows, but for a species of more rows than the call serves, which gets no block
int group_pair_evidence(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &pe = sh.rep.pe;
    const uint32_t Sg = k1 - k0;
    std::vector<uint64_t> s_off(Sg + 1, 0), p_off(Sg + 1, 0);
    std::vector<uint32_t> s_hap;
    for (uint32_t k = 0; k < Sg; ++k) {
        const uint64_t K = g.off[k + 1] - g.off[k];
        pe.K[k0 + k] = (uint32_t)K;
        if (K >= 2 && K <= HAP_PAIRS_MAX_K) s_hap.insert(s_hap.end(), g.hap.begin() + (ptrdiff_t)g.off[k], g.hap.begin() + (ptrdiff_t)g.off[k + 1]);
        s_off[k + 1] = s_hap.size();
    }
    const pantax_hip_evidence_set set{Sg, s_off.data(), s_hap.data()};
    const int rc_size = pantax_hip_strain_pair_evidence(run.ctx, db, &set, p_off.data(), 0, nullptr, nullptr);   // sizes: E_LIMIT unless there is no entry
    if (rc_size != 0 && rc_size != PANTAX_HIP_E_LIMIT) return rc_size;
    const size_t pair0 = pe.pair.size() / 4;
    pe.pair.resize(4 * (pair0 + p_off[Sg]));
    if (p_off[Sg]) PTX_TRY(pantax_hip_strain_pair_evidence(run.ctx, db, &set, p_off.data(), p_off[Sg], pe.pair.data() + 4 * pair0, nullptr));
    for (uint32_t k = 0; k < Sg; ++k) pe.pair_off[k0 + k] = pair0 + p_off[k];
    run.lap("  strain pair evidence");
    return 0;
}
// --strain-read-support: the candidates and weights of group_read_strains, summed on the device (nothing per read comes back)
int group_read_support(Run &run, const Ingest &in, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &sup = sh.rep.sup;
    const uint32_t Sg = k1 - k0;
    std::vector<uint64_t> p_off(Sg + 1, 0);
    const pantax_hip_read_strain_set cs{Sg, g.off.data(), g.hap.data(), g.w.data()};
    sup.hap.resize(9 * (g.entry0 + g.hap.size()));
    uint64_t n_pair = 0;
    for (uint32_t k = 0; k < Sg; ++k) { const uint64_t K = g.off[k + 1] - g.off[k]; sup.K[k0 + k] = (uint32_t)K; n_pair += K <= 64 ? K * K : 0; }
    const size_t pair0 = sup.pair.size();
    sup.pair.resize(pair0 + n_pair);
    PTX_TRY(pantax_hip_strain_read_support(run.ctx, db, in.reads.rd, &cs, sup.hap.data() + 9 * g.entry0, sup.species.data() + 12 * (size_t)k0, p_off.data(), n_pair,
                                           sup.pair.data() + pair0));
    for (uint32_t k = 0; k < Sg; ++k) sup.pair_off[k0 + k] = pair0 + p_off[k];
    run.lap("  strain read support");
    return 0;
}
// --strain-mosaic, beside the read support call and with its candidates and weights: the cut reads summed on the device.  Junctions (unless the plan's top
// is off) with a first guess of their number; a second call only when the group has more breaks than that: n_breaks then says how many
int group_mosaic(Run &run, const Ingest &in, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &mo = sh.rep.mo;
    const uint32_t Sg = k1 - k0;
    std::vector<uint64_t> p_off(Sg + 1, 0);
    const pantax_hip_read_strain_set cs{Sg, g.off.data(), g.hap.data(), g.w.data()};
    mo.hap.resize(2 * (g.entry0 + g.hap.size()));
    uint64_t n_pair = 0;
    for (uint32_t k = 0; k < Sg; ++k) { const uint64_t K = g.off[k + 1] - g.off[k]; mo.K[k0 + k] = (uint32_t)K; n_pair += K <= 64 ? K * K : 0; }
    const size_t pair0 = mo.pair.size();
    mo.pair.resize(pair0 + n_pair);
    uint64_t cap = run.p.rep.mo_top ? 4096 : 0, n_junctions = 0, n_breaks = 0;
    std::vector<uint32_t> jn;
    std::vector<uint64_t> jc;
    for (;;) {
        jn.assign(3 * cap, 0); jc.assign(cap, 0);
        const int rc = pantax_hip_strain_mosaic(run.ctx, db, in.reads.rd, &cs, mo.species.data() + 3 * MOS_N_CLASSES * (size_t)k0, mo.extra.data() + 3 * (size_t)k0,
                                                mo.hap.data() + 2 * g.entry0, p_off.data(), n_pair, mo.pair.data() + pair0, cap, cap ? jn.data() : nullptr,
                                                cap ? jc.data() : nullptr, &n_junctions, &n_breaks);
        if (rc == PANTAX_HIP_E_LIMIT && cap && n_breaks > cap) { cap = n_breaks; continue; }
        if (rc != 0) return rc;
        break;
    }
    uint64_t j = 0;
    for (uint32_t k = 0; k < Sg; ++k) {
        mo.pair_off[k0 + k] = pair0 + p_off[k];
        for (; j < n_junctions && jn[3 * j] == k; ++j) { mo.jn_a.push_back(jn[3 * j + 1]); mo.jn_b.push_back(jn[3 * j + 2]); mo.jn_count.push_back(jc[j]); }
        mo.jn_off[k0 + k + 1] = mo.jn_count.size();
    }
    run.lap("  strain mosaic reads");
    return 0;
}
// --strain-em, right behind the read support call: the candidates of group_read_strains with G = the len of the strain's `all` class of the node evidence
// (the evidence report's when it runs, else a call of its own) in place of the weights; max_iter from the plan, tol 1e-6
int group_read_em(Run &run, const Ingest &in, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &em = sh.rep.em;
    const uint32_t Sg = k1 - k0;
    const size_t C = g.hap.size();
    std::vector<uint64_t> own_hap, own_species;
    const uint64_t *ev = nullptr;                                          // [C][2][4] of this group's entries
    if (run.p.rep.run[REP_EVIDENCE]) ev = sh.rep.ev.hap.data() + 2 * EVIDENCE_N * g.entry0;
    else {
        const pantax_hip_evidence_set set{Sg, g.off.data(), g.hap.data()};
        own_hap.assign(2 * EVIDENCE_N * (C ? C : 1), 0); own_species.assign(3 * EVIDENCE_N * (size_t)Sg, 0);
        PTX_TRY(pantax_hip_strain_evidence(run.ctx, db, &set, own_hap.data(), own_species.data()));
        ev = own_hap.data();
    }
    em.len.resize(g.entry0 + C); em.x.resize(g.entry0 + C, 0.0);
    for (size_t c = 0; c < C; ++c) em.len[g.entry0 + c] = ev[2 * EVIDENCE_N * c + 1];
    const pantax_hip_read_em_set cs{Sg, g.off.data(), g.hap.data(), em.len.data() + g.entry0, run.p.rep.em_iterations, 1e-6};
    std::vector<uint64_t> c_off(Sg + 1, 0), c_mask, c_q;
    uint64_t cap = 4096;
    for (;;) {   // a second call only when the group has more classes than the first guess holds: c_off then says how many
        c_mask.assign(cap, 0); c_q.assign(3 * cap, 0);
        const int rc = pantax_hip_strain_read_em(run.ctx, db, in.reads.rd, &cs, em.species.data() + 6 * (size_t)k0, c_off.data(), cap, c_mask.data(), c_q.data(),
                                                 em.x.data() + g.entry0, em.iter.data() + k0, em.conv.data() + k0, em.delta.data() + k0);
        if (rc == PANTAX_HIP_E_LIMIT && c_off[Sg] > cap) { cap = c_off[Sg]; continue; }
        if (rc != 0) return rc;
        break;
    }
    for (uint32_t k = 0; k < Sg; ++k) {
        em.K[k0 + k] = (uint32_t)(g.off[k + 1] - g.off[k]);
        for (uint64_t j = c_off[k]; j < c_off[k + 1]; ++j) em.cls.push_back(ReportData::EmClass{c_mask[j], {c_q[3 * j], c_q[3 * j + 1], c_q[3 * j + 2]}});
        em.cls_off[k0 + k + 1] = em.cls.size();
    }
    run.lap("  strain read classes");
    return 0;
}
// The candidates of a group and their near-miss sums, for the near-miss report and the add-one report: Sel_s = the group's rows; Cand_s = every other
// haplotype of a species of <= 64 haplotypes, of a wider one the unreported haplotypes that have a unique_trio_nodes_fraction, the 256 largest (ties: lower
// index first) -- the cap bounds the node-mask arena of the walk route at four words a node.  One stage call a group, by whichever report asks first
struct GroupCand { bool done = false; std::vector<uint64_t> off; std::vector<uint32_t> hap; std::vector<uint64_t> out /*[J][2][4]*/, species /*[Sg][3][4]*/; };
int group_candidates(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, const ShardResult &sh, GroupCand &gc) {
    constexpr uint64_t WIDE_CAP = 256;
    if (gc.done) return 0;
    const uint32_t Sg = k1 - k0;
    gc.off.assign(Sg + 1, 0);
    gc.hap.clear();
    for (uint32_t k = k0; k < k1; ++k) {
        const uint64_t h0 = sh.hap_off[k], nh = sh.hap_off[k + 1] - h0;
        const size_t at = gc.hap.size();
        for (uint64_t h = h0; h < h0 + nh; ++h)
            if (!g.pass[h] && (nh <= 64 || (sh.met[h].has & PANTAX_HIP_HAS_FRACTION))) gc.hap.push_back((uint32_t)(h - h0));
        if (nh > 64) {
            std::stable_sort(gc.hap.begin() + at, gc.hap.end(), [&](uint32_t a, uint32_t b) { return sh.met[h0 + a].unique_trio_nodes_fraction > sh.met[h0 + b].unique_trio_nodes_fraction; });
            if (gc.hap.size() - at > WIDE_CAP) gc.hap.resize(at + WIDE_CAP);
        }
        gc.off[k - k0 + 1] = gc.hap.size();
    }
    const pantax_hip_near_miss_set set{Sg, g.off.data(), g.hap.data(), gc.off.data(), gc.hap.data()};
    gc.out.assign(8 * gc.hap.size(), 0);
    gc.species.assign(12 * (size_t)Sg, 0);
    PTX_TRY(pantax_hip_strain_near_miss(run.ctx, db, &set, gc.out.data(), gc.species.data()));
    gc.done = true;
    return 0;
}
// --strain-addin, on the same coverage result, behind the leave-one-out test: Sel_s = the group's rows (column = position: ascending haplotype); Cand_s = the
// group's candidates in the rank order of pantax_hip_near_miss_rank, top = strain_addin_top, cut to 64 - K_s (a candidate without novel bases has no rank
// and is not tested; a species of more than 64 rows gets no candidate and comes back beyond the limit)
int group_addin(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh, GroupCand &gc) {
    auto &ai = sh.rep.ai;
    const uint32_t Sg = k1 - k0;
    PTX_TRY(group_candidates(run, db, k0, k1, g, sh, gc));
    std::vector<uint64_t> a_off(Sg + 1, 0);
    std::vector<uint32_t> a_hap, rank;
    for (uint32_t k = 0; k < Sg; ++k) {
        const uint64_t c0 = gc.off[k], n = gc.off[k + 1] - c0, K = g.off[k + 1] - g.off[k];
        uint32_t kept = 0;
        rank.assign(n ? n : 1, 0);
        if (n && K < 64) PTX_TRY(pantax_hip_near_miss_rank((uint32_t)n, gc.hap.data() + c0, gc.out.data() + 8 * c0, run.p.rep.ai_top, rank.data(), &kept));
        kept = (uint32_t)std::min<uint64_t>(kept, K < 64 ? 64 - K : 0);
        for (uint32_t i = 0; i < kept; ++i) a_hap.push_back(gc.hap[c0 + rank[i]]);
        a_off[k + 1] = a_hap.size();
    }
    const uint64_t Q = a_hap.size() + Sg;
    uint64_t X = 0;
    for (uint32_t k = 0; k < Sg; ++k) { const uint64_t K = g.off[k + 1] - g.off[k], J = a_off[k + 1] - a_off[k]; X += (J + 1) * (K + J); }
    const pantax_hip_near_miss_set set{Sg, g.off.data(), g.hap.data(), a_off.data(), a_hap.data()};
    std::vector<double> x(X ? X : 1), obj(Q);
    std::vector<int32_t> status(Q);
    std::vector<uint64_t> rows(Sg), cnt(4 * Q);
    PTX_TRY(pantax_hip_strain_addin(run.ctx, db, &set, x.data(), obj.data(), status.data(), rows.data(), cnt.data()));
    uint64_t x0 = 0;
    for (uint32_t k = 0; k < Sg; ++k) {
        const uint64_t s0 = g.off[k], K = g.off[k + 1] - s0, J = a_off[k + 1] - a_off[k], W = K + J, q0 = a_off[k] + k;
        ai.rows[k0 + k] = rows[k]; ai.obj[k0 + k] = obj[q0]; ai.status[k0 + k] = status[q0]; ai.novel[k0 + k] = cnt[4 * q0 + 1]; ai.K[k0 + k] = (uint32_t)K;
        for (uint64_t c = 0; c < J; ++c) {
            ReportData::AddinRow r{};
            const double *xb = x.data() + x0, *xa = xb + (c + 1) * W;
            double o[3] = {-1.0, 0.0, 0.0};
            PTX_TRY(pantax_hip_addin_donor((uint32_t)W, (uint32_t)K, xb, xa, o));
            r.hap = sh.hap_off[k0 + k] + a_hap[a_off[k] + c];
            r.obj_with = obj[q0 + 1 + c]; r.st = status[q0 + 1 + c]; r.coverage = xa[K + c];
            std::copy(cnt.begin() + 4 * (q0 + 1 + c), cnt.begin() + 4 * (q0 + 1 + c) + 4, r.cnt);
            r.donor = o[0] < 0 ? -1 : (int64_t)(sh.hap_off[k0 + k] + g.hap[s0 + (uint64_t)o[0]]); r.loss = o[1]; r.shift = o[2];
            ai.cand.push_back(r);
        }
        ai.row_off[k0 + k + 1] = ai.cand.size();
        x0 += (J + 1) * W;
    }
    run.lap("  strain add-one");
    return 0;
}
// --strain-near-miss, on the same coverage result: the candidates pantax_hip_near_miss_rank keeps are the ones printed; their `all` comes from one evidence
// call of the group over them alone
int group_near_miss(Run &run, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh, GroupCand &gc) {
    auto &nm = sh.rep.nm;
    const uint32_t Sg = k1 - k0;
    PTX_TRY(group_candidates(run, db, k0, k1, g, sh, gc));
    const std::vector<uint64_t> &c_off = gc.off, &c_out = gc.out;
    const std::vector<uint32_t> &c_hap = gc.hap;
    std::copy(gc.species.begin(), gc.species.end(), nm.species.begin() + 12 * (size_t)k0);
    // the printed candidates of every species, in rank order
    std::vector<uint64_t> p_off(Sg + 1, 0);
    std::vector<uint32_t> p_hap, rank;
    const size_t row0 = nm.rows.size();
    for (uint32_t k = k0; k < k1; ++k) {
        const uint64_t c0 = c_off[k - k0], n = c_off[k - k0 + 1] - c0;
        uint32_t kept = 0;
        rank.assign(n ? n : 1, 0);
        if (n) PTX_TRY(pantax_hip_near_miss_rank((uint32_t)n, c_hap.data() + c0, c_out.data() + 8 * c0, run.p.rep.nm_top, rank.data(), &kept));
        for (uint32_t i = 0; i < kept; ++i) {
            ReportData::NearMissRow r{};
            r.hap = sh.hap_off[k] + c_hap[c0 + rank[i]];
            std::copy(c_out.begin() + 8 * (c0 + rank[i]), c_out.begin() + 8 * (c0 + rank[i]) + 8, r.q);
            nm.rows.push_back(r);
            p_hap.push_back(c_hap[c0 + rank[i]]);
        }
        p_off[k - k0 + 1] = p_hap.size();
        nm.row_off[k + 1] = nm.rows.size();
    }
    const pantax_hip_evidence_set printed{Sg, p_off.data(), p_hap.data()};
    std::vector<uint64_t> e_hap(8 * p_hap.size()), e_species(12 * (size_t)Sg);
    PTX_TRY(pantax_hip_strain_evidence(run.ctx, db, &printed, e_hap.data(), e_species.data()));
    for (size_t i = 0; i < p_hap.size(); ++i) std::copy(e_hap.begin() + 8 * i, e_hap.begin() + 8 * i + 4, nm.rows[row0 + i].q + 8);   // all
    run.lap("  strain near misses");
    return 0;
}
// --strain-rescue, beside the mosaic call: Sel_s = the group's rows; Cand_s = the group's candidates (rescue_candidates: the rank order of
// pantax_hip_near_miss_rank with top = 0, then the rest in ascending haplotype index, cut to 64 - K_s; a species of more than 64 rows goes in with its rows
// alone and comes back skipped).  The candidates pantax_hip_rescue_rank keeps are the ones printed
int group_rescue(Run &run, const Ingest &in, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh, GroupCand &gc) {
    auto &rc = sh.rep.rc;
    const uint32_t Sg = k1 - k0;
    PTX_TRY(group_candidates(run, db, k0, k1, g, sh, gc));
    std::vector<uint64_t> c_off(Sg + 1, 0);
    std::vector<uint32_t> c_hap, rank;
    for (uint32_t k = 0; k < Sg; ++k) {
        const uint64_t c0 = gc.off[k], n = gc.off[k + 1] - c0, K = g.off[k + 1] - g.off[k];
        uint32_t kept = 0;
        rank.assign(n ? n : 1, 0);
        if (n && K < RESCUE_MAX_LIST) PTX_TRY(pantax_hip_near_miss_rank((uint32_t)n, gc.hap.data() + c0, gc.out.data() + 8 * c0, 0, rank.data(), &kept));
        for (const uint32_t c : rescue_candidates(K, (uint32_t)n, gc.hap.data() + c0, rank.data(), kept)) c_hap.push_back(gc.hap[c0 + c]);
        c_off[k + 1] = c_hap.size();
        rc.open[k0 + k] = K + (c_off[k + 1] - c_off[k]) <= RESCUE_MAX_LIST ? 1 : 0;
    }
    const pantax_hip_near_miss_set set{Sg, g.off.data(), g.hap.data(), c_off.data(), c_hap.data()};
    std::vector<uint64_t> out(9 * c_hap.size()), steps(c_hap.size());
    PTX_TRY(pantax_hip_strain_read_rescue(run.ctx, db, in.reads.rd, &set, rc.species.data() + 3 * RES_N_CLASSES * (size_t)k0, rc.step.data() + 3 * (size_t)k0,
                                          out.data(), steps.data()));
    for (uint32_t k = 0; k < Sg; ++k) {
        const uint64_t c0 = c_off[k], n = c_off[k + 1] - c0;
        uint32_t kept = 0;
        rank.assign(n ? n : 1, 0);
        if (n) PTX_TRY(pantax_hip_rescue_rank((uint32_t)n, c_hap.data() + c0, out.data() + 9 * c0, run.p.rep.rs_top, rank.data(), &kept));
        for (uint32_t i = 0; i < kept; ++i) {
            ReportData::RescueRow r{};
            r.hap = sh.hap_off[k0 + k] + c_hap[c0 + rank[i]];
            std::copy(out.begin() + 9 * (c0 + rank[i]), out.begin() + 9 * (c0 + rank[i]) + 9, r.q);
            r.steps = steps[c0 + rank[i]];
            rc.rows.push_back(r);
        }
        rc.row_off[k0 + k + 1] = rc.rows.size();
    }
    run.lap("  strain read rescue");
    return 0;
}
// --strain-links, beside the read rescue call: Sel_s = the group's rows; the two calls of the cap protocol.  A species of more than 64 rows comes back skipped
int group_links(Run &run, const Ingest &in, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &lk = sh.rep.lk;
    const size_t C = g.hap.size(), e0 = g.entry0;
    const pantax_hip_read_strain_set set{k1 - k0, g.off.data(), g.hap.data(), nullptr};
    lk.hap.resize(LNK_N_HAP * (e0 + C));
    for (uint32_t k = k0; k < k1; ++k) lk.open[k] = g.off[k - k0 + 1] - g.off[k - k0] <= LINKS_MAX_LIST ? 1 : 0;
    uint64_t *const sp = lk.species.data() + LNK_N_SPECIES * (size_t)k0, *const lt = lk.link.data() + LNK_N_TABLE * (size_t)k0, *const hp = lk.hap.data() + LNK_N_HAP * e0;
    std::vector<uint64_t> b_off(C + 1, 0);
    const int rc_size = pantax_hip_strain_links(run.ctx, db, in.reads.rd, &set, sp, lt, hp, b_off.data(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);   // sizes: E_LIMIT unless there is no break
    if (rc_size != 0 && rc_size != PANTAX_HIP_E_LIMIT) return rc_size;
    const uint64_t n = b_off[C], at = lk.start.size();
    std::vector<uint64_t> step(n);
    lk.start.resize(at + n); lk.flank.resize(at + n); lk.mask.resize(at + n); lk.node_a.resize(at + n); lk.node_b.resize(at + n);
    if (n) PTX_TRY(pantax_hip_strain_links(run.ctx, db, in.reads.rd, &set, sp, lt, hp, b_off.data(), n, step.data(), lk.start.data() + at, lk.node_a.data() + at,
                                           lk.node_b.data() + at, lk.flank.data() + at, lk.mask.data() + at));
    for (size_t e = 0; e < C; ++e) lk.brk_off.push_back(at + b_off[e + 1]);
    run.lap("  strain link support");
    return 0;
}
// --strain-fragments, beside the rarefaction call and with the candidates and weights of group_read_strains.  Before the first group: key and tag of every
// record from the mapped text and the id spans, on the host crew, and the mates of the whole file in one call
int group_fragments(Run &run, const Ingest &in, pantax_hip_db *db, uint32_t k0, uint32_t k1, const GroupSel &g, ShardResult &sh) {
    auto &fr = sh.rep.fr;
    const uint32_t Sg = k1 - k0;
    const uint64_t R = in.R;
    if (!fr.have_mate) {
        if (in.hr.id_span.size() != R) return fail(run.ctx, PANTAX_HIP_E_STATE, "profile: the fragment support report needs the id spans of the GAF");
        std::vector<uint64_t> key(R);
        std::vector<uint8_t> tag(R);
        const int n_thr = (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
        parallel_for(R, n_thr, [&](uint64_t i0, uint64_t i1) {
            for (uint64_t r = i0; r < i1; ++r) fragment_key(in.mf.data + in.text_begin + in.hr.id_span[r].first, in.hr.id_span[r].second, key[r], tag[r]);
        });
        uint64_t counts[4];
        fr.mate.assign(R, PANTAX_HIP_MATE_NONE);
        PTX_TRY(pantax_hip_fragment_mates(run.ctx, R, key.data(), tag.data(), fr.mate.data(), counts));
        fr.have_mate = true;
        run.lap("  fragment mates");
    }
    std::vector<uint64_t> p_off(Sg + 1, 0);
    const pantax_hip_read_strain_set cs{Sg, g.off.data(), g.hap.data(), g.w.data()};
    fr.hap.resize(3 * FRG_N_HAP * (g.entry0 + g.hap.size()));
    uint64_t n_pair = 0;
    for (uint32_t k = 0; k < Sg; ++k) { const uint64_t K = g.off[k + 1] - g.off[k]; fr.K[k0 + k] = (uint32_t)K; n_pair += K <= FRAG_MAX_LIST ? K * K : 0; }
    const size_t pair0 = fr.pair.size();
    fr.pair.resize(pair0 + n_pair);
    PTX_TRY(pantax_hip_strain_fragments(run.ctx, db, in.reads.rd, &cs, fr.mate.data(), fr.hap.data() + 3 * FRG_N_HAP * g.entry0,
                                        fr.species.data() + 3 * FRG_N_CLASSES * (size_t)k0, fr.status.data() + k0, p_off.data(), n_pair, fr.pair.data() + pair0, nullptr));
    for (uint32_t k = 0; k < Sg; ++k) fr.pair_off[k0 + k] = pair0 + p_off[k];
    run.lap("  strain fragment support");
    return 0;
}

// ---- the files: what every writer is handed, what the writers share, the writers
struct Writer {
    Run &run; const Ingest &in; const Selection &sn; const ShardResult &sh; const std::vector<GenomeRow> &genomes;
    const std::vector<TrackRow> &rows;                      // the rows of strain_abundance.txt, in its order
    std::unordered_map<std::string, size_t> first_genome;   // the first genomes_info.txt row of every haplotype (the strain table's left join)
    const ReportData &rep = sh.rep;
    const uint32_t Su = (uint32_t)sh.use.size();
    const std::string &species(uint32_t k) const { return in.ranges[sn.sel[sh.use[k]]].species; }
    std::string species_head(uint32_t k) const { return species(k) + "\t-\t-"; }
    std::string strain_head(const TrackRow &r) const { return species(r.k) + '\t' + (r.gr ? r.gr->strain_taxid : "") + '\t' + (r.gr ? r.gr->genome_id : ""); }
    const GenomeRow *genome_of(uint64_t hap) const {
        const auto it = first_genome.find(sh.hap_names[hap]);
        return it != first_genome.end() ? &genomes[it->second] : nullptr;
    }
    // the row's entry; a row of the table that no group selected has no `what`
    int entry_of(const TrackRow &r, const char *what, int64_t *e) const {
        *e = rep.entry[r.hap];
        return *e < 0 ? fail(run.ctx, PANTAX_HIP_E_STATE, "profile: strain %s is a row of the strain table but has no %s", sh.hap_names[r.hap].c_str(), what) : 0;
    }
    // open, header, body(f), close and check, lap
    template <class Body> int file(ReportId id, const char *header, const char *lap, Body body) const { return file(run.p.rep.path[id], header, lap, body); }
    template <class Body> int file(const std::string &path, const char *header, const char *lap, Body body) const {
        std::ofstream f(path);
        if (!f) return fail(run.ctx, PANTAX_HIP_E_IO, "cannot write %s", path.c_str());
        f << header;
        PTX_TRY(body(f));
        f.close();
        if (!f) return fail(run.ctx, PANTAX_HIP_E_IO, "cannot write %s", path.c_str());
        run.lap(lap);
        return 0;
    }
    // the body evidence and depth share: {all, private} of every row of strain_abundance.txt, in its order, then {total, orphan} and, of three classes,
    // core of every species of the shard in the order it went through the device (the selection's: the species table's).  n u64 a class; put(head, class, q, pc)
    template <class Put> int node_sums(const char *what, const ReportData::NodeSums &d, size_t n, size_t n_classes, Put put) const {
        for (const TrackRow &r : rows) {
            int64_t e; PTX_TRY(entry_of(r, what, &e));
            const std::string head = strain_head(r), pc = fmt_f64(sh.met[r.hap].second_sol);
            put(head, "all", d.hap.data() + 2 * n * e, pc);
            put(head, "private", d.hap.data() + 2 * n * e + n, pc);
        }
        for (uint32_t k = 0; k < Su; ++k) {
            const std::string head = species_head(k);
            const uint64_t *q = d.species.data() + n_classes * n * k;
            put(head, "total", q, "-");
            put(head, "orphan", q + n, "-");
            if (n_classes < 3) continue;
            double pc = 0.0;
            bool any = false;
            for (uint64_t h = sh.hap_off[k]; h < sh.hap_off[k + 1]; ++h)
                if (rep.entry[h] >= 0) { pc += sh.met[h].second_sol; any = true; }
            if (any) put(head, "core", q + 2 * n, fmt_f64(pc));
        }
        return 0;
    }
    // --read-strains: one row per GAF record, in the -R report's order (read_id and species_taxid are its columns 1 and 3)
    int read_strains() const {
        return file(REP_READ_STRAINS, "", "read strains report", [&](std::ofstream &rf) {
            for (uint64_t r = 0; r < in.R; ++r) {
                rf.write(in.mf.data + in.text_begin + in.hr.id_span[r].first, in.hr.id_span[r].second);
                rf << '\t' << (in.sp_idx[r] >= 0 ? in.ranges[in.sp_idx[r]].species : std::string("U")) << '\t';
                if (rep.rs.n[r] < 0) rf << "U\tU\t-\t0\n";
                else if (rep.rs.n[r] == 0 || rep.rs.hap[r] == ~0ull) rf << "U\tU\t0\t0\n";
                else {
                    if (const GenomeRow *gr = genome_of(rep.rs.hap[r])) rf << gr->genome_id << '\t' << gr->strain_taxid;
                    else rf << '\t';
                    rf << '\t' << rep.rs.n[r] << '\t' << fmt_f64(rep.rs.post[r]) << '\n';
                }
            }
            return 0;
        });
    }
    // --strain-coverage: the windows of every row of strain_abundance.txt, in its order
    int cov_track() const {
        const auto &ct = rep.ct;
        const uint64_t W = run.p.rep.ct_window;
        return file(REP_COVERAGE, "species_taxid\tstrain_taxid\tgenome_ID\tstart\tend\tn_nodes\tlen\tcovered\tbases\tdepth\tbreadth\n", "strain coverage report", [&](std::ofstream &f) {
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "coverage track", &e));
                const std::string head = strain_head(r);
                const uint64_t w0 = ct.win_off[e], w1 = ct.win_off[e + 1];
                uint64_t G = 0;
                for (uint64_t i = w0; i < w1; ++i) G += ct.len[i];
                for (uint64_t i = w0; i < w1; ++i) {
                    if (ct.len[i] == 0) continue;   // no node starts here: a longer node runs through
                    const uint64_t start = (i - w0) * W, end = i + 1 == w1 ? G : start + W;   // (only the last window can be cut short: start + W <= G before it)
                    f << head << '\t' << start << '\t' << end << '\t' << ct.n_nodes[i] << '\t' << ct.len[i] << '\t' << ct.covered[i] << '\t' << ct.bases[i] << '\t'
                      << fmt_f64((double)ct.bases[i] / (double)ct.len[i]) << '\t' << fmt_f64((double)ct.covered[i] / (double)ct.len[i]) << '\n';
                }
            }
            return 0;
        });
    }
    // --strain-growth: one row per row of strain_abundance.txt, in its order: pantax_hip_growth_fit over the row's own-node windows
    int growth() const {
        const auto &gr = rep.gr;
        const ReportPlan &plan = run.p.rep;
        const uint64_t W = plan.gr_window;
        const uint64_t min_own = std::max<uint64_t>(1, (uint64_t)((unsigned __int128)W * plan.gr_min_own / 1000));
        return file(plan.ext12_path[X12REP_GROWTH],
                    "species_taxid\tstrain_taxid\tgenome_ID\twindow\tn_windows\tn_kept\tn_zero\tn_fit\town_len\town_fraction\tmedian_depth\tslope\tintercept\tr2\tindex\tstatus\tpredicted_coverage\n",
                    "strain growth report", [&](std::ofstream &f) {
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "growth", &e));
                const uint64_t w0 = gr.win_off[e], n = gr.win_off[e + 1] - w0;
                uint64_t G = 0;
                for (uint64_t i = w0; i < w0 + n; ++i) G += gr.len[i];
                pantax_hip_growth_fit_result q;
                if (pantax_hip_growth_fit(n, gr.len_own.data() + w0, gr.bases_own.data() + w0, min_own, plan.gr_trim, PANTAX_HIP_GROWTH_MIN_WINDOWS, PANTAX_HIP_GROWTH_MIN_DEPTH, &q) != 0)
                    return fail(run.ctx, PANTAX_HIP_E_STATE, "profile: the growth fit refused its parameters");
                f << strain_head(r) << '\t' << W << '\t' << n << '\t' << q.n_kept << '\t' << q.n_zero << '\t' << q.n_fit << '\t' << q.own_len << '\t'
                  << (G ? fmt_f64((double)q.own_len / (double)G) : std::string("-")) << '\t' << fmt_f64(q.median_depth) << '\t' << fmt_f64(q.slope) << '\t' << fmt_f64(q.intercept) << '\t'
                  << fmt_f64(q.r2) << '\t' << fmt_f64(q.index) << '\t' << pantax_hip_growth_status_name(q.status) << '\t' << fmt_f64(sh.met[r.hap].second_sol) << '\n';
            }
            return 0;
        });
    }
    // --strain-segments: per row of strain_abundance.txt, in its order, the strain, the totals of either class over all runs, and the chains of its kept
    // segments (pantax_hip_segment_chain with the plan's bridge and min_span) in ascending start, ranked per class
    int segments() const {
        const auto &sg = rep.sg;
        const ReportPlan &plan = run.p.rep;
        return file(plan.ext6_path[X6REP_SEGMENTS],
                    "species_taxid\tstrain_taxid\tgenome_ID\tclass\trank\tstart\tend\tspan\tin_class\tn_segments\tn_nodes\tbases\tdepth\tfraction\tthreshold\tpredicted_coverage\n",
                    "strain segment report", [&](std::ofstream &f) {
            std::vector<uint8_t> c_cls;
            std::vector<uint64_t> c_first, c_last, c_q;
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "segments", &e));
                const std::string head = strain_head(r), pc = fmt_f64(sh.met[r.hap].second_sol);
                const uint64_t G = sg.hap_len[e], pd = sg.peak[e];
                const std::string thr = pd ? std::to_string((unsigned long long)pd) : std::string("-");
                f << head << "\tstrain\t-\t0\t" << G << '\t' << G << "\t-\t-\t-\t-\t-\t-\t" << thr << '\t' << pc << '\n';
                for (int k = 0; k < 2; ++k)
                    f << head << '\t' << (k ? "peak_total" : "gap_total") << "\t-\t-\t-\t" << sg.run_max[2 * e + k] << '\t' << sg.run_len[2 * e + k] << '\t' << sg.n_runs[2 * e + k]
                      << "\t-\t-\t-\t" << (G ? fmt_f64((double)sg.run_len[2 * e + k] / (double)G) : std::string("-")) << '\t' << (k ? thr : std::string("-")) << '\t' << pc << '\n';
                const uint64_t s0 = sg.seg_off[e], n = sg.seg_off[e + 1] - s0;
                uint64_t m = 0;
                c_cls.resize(n); c_first.resize(n); c_last.resize(n); c_q.resize(PANTAX_HIP_SEGMENT_CHAIN_N * n);
                if (pantax_hip_segment_chain(n, sg.cls.data() + s0, sg.start.data() + s0, sg.len.data() + s0, sg.n_steps.data() + s0, sg.bases.data() + s0, plan.sg_bridge,
                                             plan.sg_min, &m, c_cls.data(), c_first.data(), c_last.data(), c_q.data()) != 0)
                    return fail(run.ctx, PANTAX_HIP_E_STATE, "profile: the segments of a strain are not ascending and disjoint");
                uint64_t rank[2] = {0, 0};
                for (uint64_t i = 0; i < m; ++i) {
                    const uint64_t *q = c_q.data() + PANTAX_HIP_SEGMENT_CHAIN_N * i;
                    const bool peak = c_cls[i] == PANTAX_HIP_SEGMENT_PEAK;
                    f << head << '\t' << (peak ? "peak" : "gap") << '\t' << ++rank[peak ? 1 : 0] << '\t' << q[0] << '\t' << q[1] << '\t' << q[2] << '\t' << q[3] << '\t' << q[4] << '\t'
                      << q[5] << '\t' << q[6] << '\t' << fmt_f64((double)q[6] / (double)q[3]) << '\t' << fmt_f64((double)q[3] / (double)q[2]) << '\t' << (peak ? thr : std::string("-"))
                      << '\t' << pc << '\n';
                }
            }
            return 0;
        });
    }
    // --strain-evidence: the sums {n_nodes, len, covered, bases} of every class, with depth and breadth
    int evidence() const {
        return file(REP_EVIDENCE, "species_taxid\tstrain_taxid\tgenome_ID\tclass\tn_nodes\tlen\tcovered\tbases\tdepth\tbreadth\tpredicted_coverage\n", "strain evidence report", [&](std::ofstream &f) {
            return node_sums("node evidence", rep.ev, EVIDENCE_N, 3, [&f](const std::string &head, const char *cls, const uint64_t *q, const std::string &pc) {
                f << head << '\t' << cls << '\t' << q[0] << '\t' << q[1] << '\t' << q[2] << '\t' << q[3] << '\t';
                if (q[1]) f << fmt_f64((double)q[3] / (double)q[1]) << '\t' << fmt_f64((double)q[2] / (double)q[1]);
                else f << "-\t-";
                f << '\t' << pc << '\n';
            });
        });
    }
    // --strain-fit: the sums {n_nodes, len, bases, expected, excess, deficit, blind_nodes, blind_expected} of every class, with fit = 1 - (excess + deficit) /
    // (bases + expected): {all, private} of every row of strain_abundance.txt, in its order, then {total, explained, orphan} of every species of the shard in the
    // order it went through the device; explained only where the species has rows, with the f64 sum of their weights in ascending haplotype index
    int fit() const {
        return file(run.p.rep.ext_path[XREP_FIT], "species_taxid\tstrain_taxid\tgenome_ID\tclass\tn_nodes\tlen\tbases\texpected\texcess\tdeficit\tblind_nodes\tblind_expected\tfit\tpredicted_coverage\n",
                    "strain fit report", [&](std::ofstream &f) {
            const auto put = [&f](const std::string &head, const char *cls, const uint64_t *q, const std::string &pc) {
                f << head << '\t' << cls;
                for (size_t i = 0; i < FIT_N; ++i) f << '\t' << q[i];
                const uint64_t off = q[4] + q[5], of = q[2] + q[3];
                f << '\t' << (of ? fmt_f64(1.0 - (double)off / (double)of) : std::string("-")) << '\t' << pc << '\n';
            };
            const auto &d = rep.ft;
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "model fit", &e));
                const std::string head = strain_head(r), pc = fmt_f64(sh.met[r.hap].second_sol);
                put(head, "all", d.hap.data() + 2 * FIT_N * e, pc);
                put(head, "private", d.hap.data() + 2 * FIT_N * e + FIT_N, pc);
            }
            for (uint32_t k = 0; k < Su; ++k) {
                const std::string head = species_head(k);
                const uint64_t *q = d.species.data() + 3 * FIT_N * k;
                double pc = 0.0;
                bool any = false;
                for (uint64_t h = sh.hap_off[k]; h < sh.hap_off[k + 1]; ++h)
                    if (rep.entry[h] >= 0) { pc += sh.met[h].second_sol; any = true; }
                put(head, "total", q, "-");
                if (any) put(head, "explained", q + FIT_N, fmt_f64(pc));
                put(head, "orphan", q + 2 * FIT_N, "-");
            }
            return 0;
        });
    }
    // --strain-bootstrap: per row of strain_abundance.txt, in its order, the refit and the summary of its x over the replicates, its share of the species'
    // refit and the 2.5 % / 97.5 % quantiles of its share per replicate; then per species of the shard in the order it went through the device the rows and
    // the objective of the refit and the summary of the replicates' objectives ("skipped": more rows than the call serves)
    int bootstrap() const {
        return file(run.p.rep.ext2_path[X2REP_BOOTSTRAP],
                    "species_taxid\tstrain_taxid\tgenome_ID\tclass\tpredicted_coverage\trefit\tn_solved\tmean\tsd\tq025\tq25\tq50\tq75\tq975\tmin\tzero_fraction\tshare\tshare_q025\tshare_q975\tn_rows\tobjective\n",
                    "strain bootstrap report", [&](std::ofstream &f) {
            const auto &d = rep.bs;
            const uint64_t R = d.R, n = R - 1;
            // {n_solved, mean, sd, q025 .. q975, min, zero_fraction} of one summary in the file's order; "-" but for n_solved where nothing was solved
            const auto stats = [&f](const double *o, bool zero_fraction) {
                f << '\t' << (uint64_t)o[0];
                static const int order[9] = {1, 2, 3, 4, 5, 6, 7, 9, 8};
                for (const int i : order) f << '\t' << (o[0] > 0 && (i != 8 || zero_fraction) ? fmt_f64(o[i]) : std::string("-"));
            };
            std::vector<double> share(n);
            double o[10], os[10];
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "bootstrap", &e));
                const int32_t *st = d.status.data() + R * r.k;
                f << strain_head(r) << "\tstrain\t" << fmt_f64(sh.met[r.hap].second_sol);
                if (st[0] != 0 && st[0] != 1) {   // the species was not served
                    f << "\t-\t0";
                    for (int i = 0; i < 14; ++i) f << "\t-";
                    f << '\n';
                    continue;
                }
                const double *x = d.x.data() + R * e;
                // the species' entries, in column order
                double refit_sum = 0.0;
                std::fill(share.begin(), share.end(), 0.0);
                for (uint64_t h = sh.hap_off[r.k]; h < sh.hap_off[r.k + 1]; ++h)
                    if (rep.entry[h] >= 0) {
                        const double *xe = d.x.data() + R * (uint64_t)rep.entry[h];
                        refit_sum += xe[0];
                        for (uint64_t b = 0; b < n; ++b) share[b] += xe[1 + b];
                    }
                for (uint64_t b = 0; b < n; ++b) share[b] = share[b] == 0.0 ? 0.0 : x[1 + b] / share[b];
                PTX_TRY(pantax_hip_bootstrap_summary(n, x + 1, st + 1, o));
                PTX_TRY(pantax_hip_bootstrap_summary(n, share.data(), st + 1, os));
                f << '\t' << fmt_f64(x[0]);
                stats(o, true);
                f << '\t' << fmt_f64(refit_sum == 0.0 ? 0.0 : x[0] / refit_sum) << '\t' << (os[0] > 0 ? fmt_f64(os[3]) : std::string("-")) << '\t'
                  << (os[0] > 0 ? fmt_f64(os[7]) : std::string("-")) << "\t-\t-\n";
            }
            for (uint32_t k = 0; k < Su; ++k) {
                const int32_t *st = d.status.data() + R * k;
                const bool skipped = st[0] != 0 && st[0] != 1;
                PTX_TRY(pantax_hip_bootstrap_summary(n, d.obj.data() + R * k + 1, st + 1, o));
                f << species_head(k) << '\t' << (skipped ? "skipped" : "species") << "\t-\t-";
                stats(o, false);
                f << "\t-\t-\t-\t" << d.rows[R * k] << '\t' << (skipped ? std::string("-") : fmt_f64(d.obj[R * k])) << '\n';
            }
            return 0;
        });
    }
    // --strain-dropout: per row of strain_abundance.txt, in its order, the refit and what the fit loses without the strain; then per species of the shard
    // with rows in the table, in the order it went through the device, the rows and the objective of the refit ("skipped": more rows than the call serves)
    int dropout() const {
        return file(run.p.rep.ext3_path[X3REP_DROPOUT],
                    "species_taxid\tstrain_taxid\tgenome_ID\tclass\tpredicted_coverage\trefit\tn_rows\tobjective\tobjective_without\tdelta\tdelta_fraction\tn_member\tn_only\tn_worse\tn_better\tsubstitute_strain_taxid\tsubstitute_genome_ID\tsubstitute_gain\tshift\n",
                    "strain dropout report", [&](std::ofstream &f) {
            const auto &d = rep.dr;
            std::vector<const TrackRow *> row_of(d.refit.size(), nullptr);   // entry -> its first row of the table
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "leave-one-out test", &e));
                if (!row_of[e]) row_of[e] = &r;
            }
            for (const TrackRow &r : rows) {
                const int64_t e = rep.entry[r.hap];
                f << strain_head(r) << "\tstrain\t" << fmt_f64(sh.met[r.hap].second_sol);
                if (d.status[r.k] != 0 || d.st[e] != 0) {   // the species was not served, has no row, or one of the two LPs failed
                    for (int i = 0; i < 14; ++i) f << "\t-";
                    f << '\n';
                    continue;
                }
                const double delta = d.obj_without[e] - d.obj[r.k];
                f << '\t' << fmt_f64(d.refit[e]) << '\t' << d.rows[r.k] << '\t' << fmt_f64(d.obj[r.k]) << '\t' << fmt_f64(d.obj_without[e]) << '\t' << fmt_f64(delta) << '\t'
                  << (d.obj_without[e] != 0.0 ? fmt_f64(delta / d.obj_without[e]) : std::string("-"));
                for (int c = 0; c < 4; ++c) f << '\t' << d.cnt[4 * e + c];
                const TrackRow *sub = d.sub[e] >= 0 ? row_of[d.sub[e]] : nullptr;
                if (sub) f << '\t' << (sub->gr ? sub->gr->strain_taxid : "") << '\t' << (sub->gr ? sub->gr->genome_id : "") << '\t' << fmt_f64(d.gain[e]);
                else f << "\t-\t-\t-";
                f << '\t' << fmt_f64(d.shift[e]) << '\n';
            }
            for (uint32_t k = 0; k < Su; ++k) {
                if (d.K[k] == 0) continue;
                const bool skipped = d.status[k] != 0 && d.status[k] != 1;
                f << species_head(k) << '\t' << (skipped ? "skipped" : "species") << "\t-\t-\t" << d.rows[k] << '\t' << (skipped ? std::string("-") : fmt_f64(d.obj[k]));
                for (int i = 0; i < 11; ++i) f << "\t-";
                f << '\n';
            }
            return 0;
        });
    }
    // --strain-addin (strain_taxid / genome_ID: the first genomes_info.txt row of the haplotype, of candidates and donors alike): per species of the shard, in
    // the order it went through the device, its tested candidates in rank order: what the fit gains with the
    // candidate, the coverage it gets and the reported strain it takes it from; then per species with rows in the table or a tested candidate the rows,
    // the objective of the reported strains alone and the rows none of them walks ("skipped": more rows in the table than the call serves)
    int addin() const {
        return file(run.p.rep.ext4_path[X4REP_ADDIN],
                    "species_taxid\tstrain_taxid\tgenome_ID\trank\tclass\tn_rows\tobjective\tobjective_with\tgain\tgain_fraction\tcoverage\tn_member\tn_novel\tn_better\tn_worse\tdonor_strain_taxid\tdonor_genome_ID\tdonor_loss\tshift\tstage\tunique_trio_nodes_fraction\n",
                    "strain add-one report", [&](std::ofstream &f) {
            const auto &d = rep.ai;
            for (uint32_t k = 0; k < Su; ++k)
                for (uint64_t i = d.row_off[k]; i < d.row_off[k + 1]; ++i) {
                    const ReportData::AddinRow &r = d.cand[i];
                    const GenomeRow *gr = genome_of(r.hap);
                    const pantax_hip_hap_metrics &m = sh.met[r.hap];
                    f << species(k) << '\t' << (gr ? gr->strain_taxid : "") << '\t' << (gr ? gr->genome_id : "") << '\t' << (i - d.row_off[k]) + 1 << "\tcandidate";
                    if (d.status[k] != 0 || r.st != 0) {   // one of the two LPs did not solve
                        for (int c = 0; c < 14; ++c) f << "\t-";
                    } else {
                        const double gain = d.obj[k] - r.obj_with;
                        f << '\t' << d.rows[k] << '\t' << fmt_f64(d.obj[k]) << '\t' << fmt_f64(r.obj_with) << '\t' << fmt_f64(gain) << '\t'
                          << (d.obj[k] != 0.0 ? fmt_f64(gain / d.obj[k]) : std::string("-")) << '\t' << fmt_f64(r.coverage);
                        for (int c = 0; c < 4; ++c) f << '\t' << r.cnt[c];
                        if (r.donor >= 0) {   // (named as the candidates are: the report does not follow the rows of the table)
                            const GenomeRow *don = genome_of((uint64_t)r.donor);
                            f << '\t' << (don ? don->strain_taxid : "") << '\t' << (don ? don->genome_id : "") << '\t' << fmt_f64(r.loss);
                        } else f << "\t-\t-\t-";
                        f << '\t' << fmt_f64(r.shift);
                    }
                    f << '\t' << near_miss_stage(m) << '\t' << ((m.has & PANTAX_HIP_HAS_FRACTION) ? fmt_f64(m.unique_trio_nodes_fraction) : std::string("-")) << '\n';
                }
            for (uint32_t k = 0; k < Su; ++k) {
                if (d.K[k] == 0 && d.row_off[k + 1] == d.row_off[k]) continue;
                const bool skipped = d.status[k] != 0 && d.status[k] != 1;
                f << species_head(k) << "\t-\t" << (skipped ? "skipped" : "species") << '\t' << d.rows[k] << '\t' << (skipped ? std::string("-") : fmt_f64(d.obj[k])) << "\t-\t-\t-\t-\t-\t"
                  << (skipped ? std::string("-") : std::to_string(d.novel[k])) << "\t-\t-\t-\t-\t-\t-\t-\t-\n";
            }
            return 0;
        });
    }
    // --strain-read-support: {compatible, unique, assigned} of every row of strain_abundance.txt, in its order; {counted, unexplained, ambiguous, uninformative}
    // of every species of the shard in the order it went through the device (a species without rows: counted only); the shared reads of every pair of rows
    int read_support() const {
        const auto &sup = rep.sup;
        return file(REP_READ_SUPPORT, "species_taxid\tstrain_taxid\tgenome_ID\tclass\tn_reads\tn_steps\tspan\tfraction\tother_strain_taxid\n", "strain read support report", [&](std::ofstream &f) {
            const auto frac = [](uint64_t n, uint64_t of) { return of ? fmt_f64((double)n / (double)of) : std::string("-"); };
            const auto put = [&](const std::string &head, const char *cls, const uint64_t *q, uint64_t of) {   // q = {n_reads, n_steps, span}
                f << head << '\t' << cls << '\t' << q[0] << '\t' << q[1] << '\t' << q[2] << '\t' << frac(q[0], of) << "\t-\n";
            };
            const char *const of_row[3] = {"compatible", "unique", "assigned"}, *const of_species[4] = {"counted", "unexplained", "ambiguous", "uninformative"};
            std::vector<const TrackRow *> row_of(sup.hap.size() / 9, nullptr);   // entry -> its first row of the table
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "read support", &e));
                if (!row_of[e]) row_of[e] = &r;
                const std::string head = strain_head(r);
                for (int c = 0; c < 3; ++c) put(head, of_row[c], sup.hap.data() + 9 * e + 3 * c, sup.species[12 * (size_t)r.k]);
            }
            for (uint32_t k = 0; k < Su; ++k) {
                const std::string head = species_head(k);
                const uint64_t *q = sup.species.data() + 12 * (size_t)k;
                for (int c = 0; c < (sup.K[k] ? 4 : 1); ++c) put(head, of_species[c], q + 3 * c, q[0]);   // a species without rows: counted only
            }
            for (uint32_t k = 0; k < Su; ++k) {
                const uint64_t K = sup.K[k];
                if (K < 2 || K > 64) continue;
                int64_t e0 = -1;                                                        // the species' entries are consecutive, in ascending haplotype index
                for (uint64_t h = sh.hap_off[k]; h < sh.hap_off[k + 1] && e0 < 0; ++h) e0 = rep.entry[h];
                const uint64_t *pm = sup.pair.data() + sup.pair_off[k];
                for (uint64_t a = 0; a < K; ++a)
                    for (uint64_t b = a + 1; b < K; ++b) {
                        const uint64_t n = pm[a * K + b];
                        if (!n || e0 < 0 || !row_of[e0 + a] || !row_of[e0 + b]) continue;
                        const TrackRow &ra = *row_of[e0 + a], &rb = *row_of[e0 + b];
                        f << strain_head(ra) << "\tshared\t" << n << "\t-\t-\t" << frac(n, std::min(pm[a * K + a], pm[b * K + b])) << '\t'
                          << (rb.gr ? rb.gr->strain_taxid : std::string()) << '\n';
                    }
            }
            return 0;
        });
    }
    // --strain-mosaic: the donor row of every row of strain_abundance.txt, in its order; the classes of every species of the shard in the order it went
    // through the device; the switches between every two rows of a species; the plan's top junctions of every species
    int mosaic() const {
        const auto &mo = rep.mo;
        return file(run.p.rep.ext7_path[X7REP_MOSAIC],
                    "species_taxid\tstrain_taxid\tgenome_ID\tclass\tn_reads\tn_steps\tspan\tn_segments\tfraction\tother_strain_taxid\tother_genome_ID\tnode_a\tnode_b\n",
                    "strain mosaic read report", [&](std::ofstream &f) {
            const auto frac = [](uint64_t n, uint64_t of) { return of ? fmt_f64((double)n / (double)of) : std::string("-"); };
            const auto served = [&](uint32_t k) { return mo.K[k] >= 1 && mo.K[k] <= MOSAIC_MAX_K; };
            const auto sp = [&](uint32_t k, int cls) { return mo.species.data() + 3 * MOS_N_CLASSES * (size_t)k + 3 * cls; };
            std::vector<const TrackRow *> row_of(mo.hap.size() / 2, nullptr);   // entry -> its first row of the table
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "mosaic reads", &e));
                if (!row_of[e]) row_of[e] = &r;
                f << strain_head(r) << "\tdonor\t-\t";
                if (served(r.k)) {
                    const uint64_t steps = sp(r.k, MOS_MOSAIC1)[1] + sp(r.k, MOS_MOSAIC2)[1] + sp(r.k, MOS_MOSAIC3PLUS)[1];
                    f << mo.hap[2 * e + 1] << "\t-\t" << mo.hap[2 * e] << '\t' << frac(mo.hap[2 * e + 1], steps);
                } else f << "-\t-\t-\t-";
                f << "\t-\t-\t-\t-\n";
            }
            const char *const of_species[MOS_N_CLASSES] = {"counted", "compatible", "mosaic1", "mosaic2", "mosaic3plus", "foreign"};
            for (uint32_t k = 0; k < Su; ++k) {
                const std::string head = species_head(k);
                const uint64_t *ex = mo.extra.data() + 3 * (size_t)k;
                for (int c = 0; c < (served(k) ? (int)MOS_N_CLASSES : 1); ++c) {   // a species without rows, or of more than 64: counted only
                    const uint64_t *q = sp(k, c);
                    f << head << '\t' << of_species[c] << '\t' << q[0] << '\t' << q[1] << '\t' << q[2] << '\t';
                    if (c == MOS_FOREIGN) f << ex[2]; else f << '-';
                    f << '\t' << frac(q[0], sp(k, MOS_COUNTED)[0]) << "\t-\t-\t-\t-\n";
                }
                if (served(k)) {
                    uint64_t q[3];
                    for (int i = 0; i < 3; ++i) q[i] = sp(k, MOS_MOSAIC1)[i] + sp(k, MOS_MOSAIC2)[i] + sp(k, MOS_MOSAIC3PLUS)[i];
                    f << head << "\tmosaic_total\t" << q[0] << '\t' << q[1] << '\t' << q[2] << '\t' << ex[0] << '\t' << frac(q[0], sp(k, MOS_COUNTED)[0]) << "\t-\t-\t-\t-\n";
                } else if (mo.K[k] > MOSAIC_MAX_K) f << head << "\tskipped\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
            }
            for (uint32_t k = 0; k < Su; ++k) {
                const uint64_t K = mo.K[k];
                if (K < 2 || K > MOSAIC_MAX_K) continue;
                int64_t e0 = -1;                                                        // the species' entries are consecutive, in ascending haplotype index
                for (uint64_t h = sh.hap_off[k]; h < sh.hap_off[k + 1] && e0 < 0; ++h) e0 = rep.entry[h];
                const uint64_t *pm = mo.pair.data() + mo.pair_off[k];
                for (uint64_t a = 0; a < K; ++a)
                    for (uint64_t b = a + 1; b < K; ++b) {
                        const uint64_t n = pm[a * K + b] + pm[b * K + a];
                        if (!n || e0 < 0 || !row_of[e0 + a] || !row_of[e0 + b]) continue;
                        const TrackRow &ra = *row_of[e0 + a], &rb = *row_of[e0 + b];
                        f << strain_head(ra) << "\tswitch\t-\t-\t-\t" << n << '\t' << frac(n, mo.extra[3 * (size_t)k + 1]) << '\t' << (rb.gr ? rb.gr->strain_taxid : std::string()) << '\t'
                          << (rb.gr ? rb.gr->genome_id : std::string()) << "\t-\t-\n";
                    }
            }
            std::vector<uint64_t> top;
            for (uint32_t k = 0; k < Su && run.p.rep.mo_top; ++k) {
                const uint64_t j0 = mo.jn_off[k], n = mo.jn_off[k + 1] - j0;
                uint64_t m = 0;
                top.resize(n);
                if (pantax_hip_mosaic_top(n, mo.jn_a.data() + j0, mo.jn_b.data() + j0, mo.jn_count.data() + j0, run.p.rep.mo_top, top.data(), &m) != 0) continue;   // (n = 0)
                const int64_t first = in.ranges[sn.sel[sh.use[k]]].start;              // the node ids of the GAF: the species' first node id + the local index
                for (uint64_t i = 0; i < m; ++i) {
                    const uint64_t j = j0 + top[i];
                    f << species_head(k) << "\tjunction\t-\t-\t-\t" << mo.jn_count[j] << '\t' << frac(mo.jn_count[j], mo.extra[3 * (size_t)k + 1]) << "\t-\t-\t" << first + (int64_t)mo.jn_a[j]
                      << '\t' << first + (int64_t)mo.jn_b[j] << '\n';
                }
            }
            return 0;
        });
    }
    // --strain-em: the estimate beside predicted_coverage for every row of strain_abundance.txt, in its order; then per species of the shard in the order it
    // went through the device its largest classes, the rest of them in one row, the unexplained reads and the species row
    int read_em() const {
        const auto &em = rep.em;
        return file(run.p.rep.ext5_path[X5REP_EM],
                    "species_taxid\tstrain_taxid\tgenome_ID\tclass\trank\tn_members\tmembers\tn_reads\tn_steps\tspan\tshare\tlen\tem_coverage\tem_bases\tem_share\tpredicted_coverage\tn_classes\tn_iter\tconverged\tdelta\n",
                    "strain read class report", [&](std::ofstream &f) {
            std::vector<const TrackRow *> row_of(em.x.size(), nullptr);   // entry -> its first row of the table
            std::vector<int64_t> e0(Su, -1);                              // the species' entries are consecutive, in ascending haplotype index: bit i = entry e0 + i
            std::vector<double> total(Su, 0.0);                           // the sum of em_bases over the species' strains, in that order
            for (uint32_t k = 0; k < Su; ++k) {
                for (uint64_t h = sh.hap_off[k]; h < sh.hap_off[k + 1] && e0[k] < 0; ++h) e0[k] = rep.entry[h];
                for (uint32_t i = 0; e0[k] >= 0 && i < em.K[k]; ++i) total[k] += em.x[e0[k] + i] * (double)em.len[e0[k] + i];
            }
            const auto served = [&](uint32_t k) { return em.K[k] >= 1 && em.K[k] <= READ_EM_MAX_K; };
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "read classes", &e));
                if (!row_of[e]) row_of[e] = &r;
                f << strain_head(r) << "\tstrain\t-\t-\t-";
                if (served(r.k)) {
                    uint64_t q[3] = {0, 0, 0};
                    const uint64_t bit = (uint64_t)(e - e0[r.k]);
                    for (uint64_t j = em.cls_off[r.k]; j < em.cls_off[r.k + 1]; ++j)
                        if ((em.cls[j].mask >> bit) & 1ull) for (int c = 0; c < 3; ++c) q[c] += em.cls[j].q[c];
                    const double bases = em.x[e] * (double)em.len[e];
                    f << '\t' << q[0] << '\t' << q[1] << '\t' << q[2] << "\t-\t" << em.len[e] << '\t' << fmt_f64(em.x[e]) << '\t' << fmt_f64(bases) << '\t'
                      << (total[r.k] != 0.0 ? fmt_f64(bases / total[r.k]) : std::string("-"));
                } else f << "\t-\t-\t-\t-\t" << em.len[e] << "\t-\t-\t-";
                f << '\t' << fmt_f64(sh.met[r.hap].second_sol) << "\t-\t-\t-\t-\n";
            }
            const auto frac = [](uint64_t n, uint64_t of) { return of ? fmt_f64((double)n / (double)of) : std::string("-"); };
            for (uint32_t k = 0; k < Su; ++k) {
                const std::string head = species_head(k);
                const uint64_t *sp = em.species.data() + 6 * (size_t)k;
                const uint64_t J = em.cls_off[k + 1] - em.cls_off[k];
                const ReportData::EmClass *cls = em.cls.data() + em.cls_off[k];
                std::vector<uint64_t> mask(J), span(J);
                for (uint64_t j = 0; j < J; ++j) { mask[j] = cls[j].mask; span[j] = cls[j].q[2]; }
                const std::vector<uint64_t> top = read_class_rank(J, mask.data(), span.data(), run.p.rep.em_classes);
                std::vector<uint8_t> printed(J, 0);
                for (size_t i = 0; i < top.size(); ++i) {
                    const ReportData::EmClass &c = cls[top[i]];
                    printed[top[i]] = 1;
                    f << head << "\tread_class\t" << i + 1 << '\t' << __builtin_popcountll(c.mask) << '\t';
                    bool first = true;
                    for (uint64_t m = c.mask; m; m &= m - 1ull) {
                        const int64_t e = e0[k] + __builtin_ctzll(m);
                        if (!first) f << ',';
                        first = false;
                        if (e0[k] >= 0 && (size_t)e < row_of.size() && row_of[e] && row_of[e]->gr) f << row_of[e]->gr->genome_id;
                    }
                    f << '\t' << c.q[0] << '\t' << c.q[1] << '\t' << c.q[2] << '\t' << frac(c.q[2], sp[2]) << "\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
                }
                if (J > top.size()) {
                    uint64_t q[3] = {0, 0, 0};
                    for (uint64_t j = 0; j < J; ++j)
                        if (!printed[j]) for (int c = 0; c < 3; ++c) q[c] += cls[j].q[c];
                    f << head << "\tother\t-\t" << J - top.size() << "\t-\t" << q[0] << '\t' << q[1] << '\t' << q[2] << '\t' << frac(q[2], sp[2]) << "\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
                }
                f << head << "\tunexplained\t-\t-\t-\t" << sp[3] << '\t' << sp[4] << '\t' << sp[5] << '\t' << frac(sp[5], sp[2]) << "\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
                f << head << '\t' << (em.K[k] > READ_EM_MAX_K ? "skipped" : "species") << "\t-\t-\t-\t" << sp[0] << '\t' << sp[1] << '\t' << sp[2] << "\t-\t-\t-\t-\t-\t-";
                if (em.K[k] > READ_EM_MAX_K) f << "\t-\t-\t-\t-\n";
                else f << '\t' << J << '\t' << em.iter[k] << '\t' << em.conv[k] << '\t' << fmt_f64(em.delta[k]) << '\n';
            }
            return 0;
        });
    }
    // --strain-depth: per histogram of every class its node count, its length, the length at depth 0 and the length-weighted quantiles
    int depth() const {
        return file(REP_DEPTH, "species_taxid\tstrain_taxid\tgenome_ID\tclass\tn_nodes\tlen\tlen_zero\tq05\tq25\tq50\tq75\tq95\tq50_hi\tpredicted_coverage\n", "strain depth report", [&](std::ofstream &f) {
            return node_sums("depth histogram", rep.dp, DEPTH_N, 2, [&f](const std::string &head, const char *cls, const uint64_t *hist, const std::string &pc) {
                uint64_t n = 0, len = 0;
                for (uint32_t b = 0; b < PANTAX_HIP_DEPTH_BINS; ++b) { n += hist[2 * b]; len += hist[2 * b + 1]; }
                f << head << '\t' << cls << '\t' << n << '\t' << len << '\t' << hist[1];
                uint64_t hi50 = 0;
                for (const uint32_t pm : {50u, 250u, 500u, 750u, 950u}) {
                    uint32_t bin = 0;
                    uint64_t lo = 0, hi = 0;
                    if (pantax_hip_depth_quantile(hist, pm, &bin) != 0) { f << "\t-"; continue; }   // len = 0
                    pantax_hip_depth_bin_range(bin, &lo, &hi);
                    if (pm == 500u) hi50 = hi;
                    f << '\t' << lo;
                }
                if (len) f << '\t' << hi50; else f << "\t-";
                f << '\t' << pc << '\n';
            });
        });
    }
    // --strain-near-miss: per species of the shard, in the order it went through the device, the candidates group_near_miss kept, in rank order, classes novel,
    // exclusive, all each; then {orphan, claimed, contested} of every species.  strain_taxid / genome_ID: the first genomes_info.txt row of the haplotype
    int near_miss() const {
        const auto &nm = rep.nm;
        return file(REP_NEAR_MISS, "species_taxid\tstrain_taxid\tgenome_ID\trank\tclass\tn_nodes\tlen\tcovered\tbases\tdepth\tbreadth\tshare\tstage\tunique_trio_nodes_fraction\tfrequencies_mean\tfirst_sol\tsecond_sol\n",
                    "strain near-miss report", [&](std::ofstream &f) {
            const char *const cand[3] = {"novel", "exclusive", "all"}, *const spec[3] = {"orphan", "claimed", "contested"};
            for (uint32_t k = 0; k < Su; ++k)
                for (uint64_t i = nm.row_off[k]; i < nm.row_off[k + 1]; ++i) {
                    const ReportData::NearMissRow &r = nm.rows[i];
                    for (int c = 0; c < 3; ++c)   // the share of the orphan bases: not of `all`
                        f << near_miss_row_text(species(k), genome_of(r.hap), &sh.met[r.hap], (uint32_t)(i - nm.row_off[k]) + 1, cand[c], r.q + 4 * c, c < 2, nm.species[12 * (size_t)k + 3]) << '\n';
                }
            for (uint32_t k = 0; k < Su; ++k) {
                const uint64_t *q = nm.species.data() + 12 * (size_t)k;
                for (int c = 0; c < 3; ++c) f << near_miss_row_text(species(k), nullptr, nullptr, 0, spec[c], q + 4 * c, true, q[3]) << '\n';
            }
            return 0;
        });
    }
    // --strain-rescue: per species of the shard, in the order it went through the device, the candidates group_rescue kept, in rank order; then the nine
    // classes of every species.  strain_taxid / genome_ID / stage / unique_trio_nodes_fraction as the near-miss report prints them
    int rescue() const {
        const auto &rc = rep.rc;
        return file(run.p.rep.ext8_path[X8REP_RESCUE],
                    "species_taxid\tstrain_taxid\tgenome_ID\trank\tclass\tn_reads\tn_steps\tspan\tfraction\talone_reads\tforeign_reads\tforeign_steps\tclaimed_steps\tstage\tunique_trio_nodes_fraction\n",
                    "strain read rescue report", [&](std::ofstream &f) {
            const auto frac = [](uint64_t n, uint64_t of) { return of ? fmt_f64((double)n / (double)of) : std::string("-"); };
            const auto sp = [&](uint32_t k, int cls) { return rc.species.data() + 3 * RES_N_CLASSES * (size_t)k + 3 * cls; };
            for (uint32_t k = 0; k < Su; ++k)
                for (uint64_t i = rc.row_off[k]; i < rc.row_off[k + 1]; ++i) {
                    const ReportData::RescueRow &r = rc.rows[i];
                    const GenomeRow *gr = genome_of(r.hap);
                    const pantax_hip_hap_metrics &m = sh.met[r.hap];
                    f << species(k) << '\t' << (gr ? gr->strain_taxid : std::string()) << '\t' << (gr ? gr->genome_id : std::string()) << '\t' << (i - rc.row_off[k]) + 1 << "\tcandidate\t"
                      << r.q[0] << '\t' << r.q[1] << '\t' << r.q[2] << '\t' << frac(r.q[0], sp(k, RES_FOREIGN)[0] + sp(k, RES_MOSAIC)[0]) << '\t' << r.q[3] << '\t' << r.q[6] << "\t-\t"
                      << r.steps << '\t' << near_miss_stage(m) << '\t' << ((m.has & PANTAX_HIP_HAS_FRACTION) ? fmt_f64(m.unique_trio_nodes_fraction) : std::string("-")) << '\n';
                }
            const char *const of_species[RES_N_CLASSES] = {"counted", "compatible", "foreign", "foreign_rescued", "foreign_patchwork", "foreign_novel", "mosaic", "mosaic_rescued", "contested"};
            for (uint32_t k = 0; k < Su; ++k) {
                const std::string head = species_head(k) + "\t-\t";
                const uint64_t *st = rc.step.data() + 3 * (size_t)k;
                for (int c = 0; c < (rc.open[k] ? (int)RES_N_CLASSES : 1); ++c) {   // a skipped species: counted only
                    const uint64_t *q = sp(k, c);
                    f << head << of_species[c] << '\t' << q[0] << '\t' << q[1] << '\t' << q[2] << '\t' << frac(q[0], sp(k, RES_COUNTED)[0]) << "\t-\t-\t";
                    if (c == RES_FOREIGN) f << st[0] << '\t' << st[1];
                    else if (c == RES_FOREIGN_NOVEL) f << st[2] << "\t-";
                    else f << "-\t-";
                    f << "\t-\t-\n";
                }
                if (!rc.open[k]) f << head << "skipped\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
            }
            return 0;
        });
    }
    // --strain-links: per row of strain_abundance.txt, in its order, the strain's eight counters and its first lk_top breaks in the order of
    // pantax_hip_link_top; then per species of the shard, in the order it went through the device, its link table and its crossings by class
    int links() const {
        const auto &lk = rep.lk;
        return file(run.p.rep.ext9_path[X9REP_LINKS],
                    "species_taxid\tstrain_taxid\tgenome_ID\tclass\trank\tn_links\tcrossed\topen\tbroken\tprivate\tprivate_crossed\tprivate_broken\tsupport\tcrossed_fraction\tstart\tnode_a\tnode_b\tflank_depth\tshared_with\tpredicted_coverage\n",
                    "link support report", [&](std::ofstream &f) {
            const auto frac = [](uint64_t n, uint64_t of) { return of ? fmt_f64((double)n / (double)of) : std::string("-"); };
            std::vector<uint64_t> top;
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "link support", &e));
                const std::string head = strain_head(r), pc = fmt_f64(sh.met[r.hap].second_sol);
                const uint64_t *q = lk.hap.data() + LNK_N_HAP * (size_t)e;
                f << head << "\tstrain\t-";
                if (lk.open[r.k]) {
                    for (int i = 0; i < (int)LNK_N_HAP; ++i) f << '\t' << q[i];
                    f << '\t' << frac(q[LNK_CROSSED], q[LNK_LINKS]);
                } else f << "\t-\t-\t-\t-\t-\t-\t-\t-\t-";
                f << "\t-\t-\t-\t-\t-\t" << pc << '\n';
                const uint64_t b0 = lk.brk_off[e], n = lk.brk_off[e + 1] - b0;
                uint64_t m = 0;
                top.resize(n ? n : 1);
                if (pantax_hip_link_top(n, lk.flank.data() + b0, lk.start.data() + b0, run.p.rep.lk_top, top.data(), &m) != 0) continue;
                const int64_t first = in.ranges[sn.sel[sh.use[r.k]]].start;              // the node ids of the GAF: the species' first node id + the local index
                for (uint64_t i = 0; i < m; ++i) {
                    const uint64_t j = b0 + top[i];
                    f << head << "\tbreak\t" << i + 1 << "\t-\t-\t-\t-\t-\t-\t-\t-\t-\t" << lk.start[j] << '\t' << first + (int64_t)lk.node_a[j] << '\t' << first + (int64_t)lk.node_b[j]
                      << '\t' << lk.flank[j] << '\t' << __builtin_popcountll(lk.mask[j]) << '\t' << pc << '\n';
                }
            }
            const char *const of_species[LNK_N_SPECIES] = {"", "crossings", "known", "skip", "switch", "foreign"};
            for (uint32_t k = 0; k < Su; ++k) {
                const std::string head = species_head(k);
                const uint64_t *sp = lk.species.data() + LNK_N_SPECIES * (size_t)k, *lt = lk.link.data() + LNK_N_TABLE * (size_t)k;
                if (lk.open[k])
                    for (int c = 0; c < 2; ++c)
                        f << head << '\t' << (c ? "core" : "links") << "\t-\t" << lt[2 * c] << '\t' << lt[2 * c + 1] << "\t-\t-\t-\t-\t-\t-\t" << frac(lt[2 * c + 1], lt[2 * c])
                          << "\t-\t-\t-\t-\t-\t-\n";
                for (int c = LNK_CROSSINGS; c < (lk.open[k] ? (int)LNK_N_SPECIES : (int)LNK_CROSSINGS + 1); ++c)   // a skipped species: crossings only
                    f << head << '\t' << of_species[c] << "\t-\t-\t-\t-\t-\t-\t-\t-\t" << sp[c] << '\t' << frac(sp[c], sp[LNK_CROSSINGS]) << "\t-\t-\t-\t-\t-\t-\n";
                if (!lk.open[k]) f << head << "\tskipped\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
            }
            return 0;
        });
    }
    // --strain-rarefy: per row of strain_abundance.txt, in its order, a row per level 0 .. L: the summary of its x over the level's replicates
    // (pantax_hip_bootstrap_summary; level 0 = entry 0 alone), the mean scaled back by 2^level, the means of n_member and n_only; then per species of the
    // shard, in the order it went through the device, per level the means of its counted reads, added bases and rows and the mean objective of the solved LPs
    int rarefy() const {
        return file(run.p.rep.ext10_path[X10REP_RAREFY],
                    "species_taxid\tstrain_taxid\tgenome_ID\tclass\tlevel\tfraction\tn_solved\tpredicted_coverage\trefit\tmean\tsd\tmin\tmax\tscaled_mean\tzero_fraction\tn_member\tn_only\tn_reads\tbases\tn_rows\tobjective\n",
                    "rarefaction report", [&](std::ofstream &f) {
            const auto &d = rep.rf;
            const uint64_t E = d.E, L = run.p.rep.rf_levels, B = run.p.rep.rf_replicates;
            // the entries of a level: entry 0 alone, or one per replicate
            const auto n_of = [&](uint64_t l) { return l == 0 ? (uint64_t)1 : B; };
            const auto entry = [&](uint64_t l, uint64_t i) { return l == 0 ? (uint64_t)0 : 1 + i * L + (l - 1); };
            const auto mean_u64 = [&](const uint64_t *v, size_t stride, uint64_t l) {   // the f64 sum in ascending replicate, divided by their number
                double s = 0.0;
                for (uint64_t i = 0; i < n_of(l); ++i) s += (double)v[stride * entry(l, i)];
                return s / (double)n_of(l);
            };
            std::vector<double> val(B ? B : 1);
            std::vector<int32_t> st(B ? B : 1);
            double o[10];
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "rarefaction", &e));
                const int32_t *sk = d.status.data() + E * r.k;
                const std::string head = strain_head(r), pc = fmt_f64(sh.met[r.hap].second_sol);
                if (sk[0] != 0 && sk[0] != 1) continue;   // the species was not served: its "skipped" row says so
                const double *x = d.x.data() + E * (uint64_t)e;
                const uint64_t *m = d.member.data() + 2 * E * (uint64_t)e;
                for (uint64_t l = 0; l <= L; ++l) {
                    const uint64_t n = n_of(l);
                    double mx = 0.0;
                    bool any = false;
                    for (uint64_t i = 0; i < n; ++i) {
                        val[i] = x[entry(l, i)]; st[i] = sk[entry(l, i)];
                        if (st[i] == 0 && (!any || val[i] > mx)) { mx = val[i]; any = true; }
                    }
                    PTX_TRY(pantax_hip_bootstrap_summary(n, val.data(), st.data(), o));
                    const double scale = std::ldexp(1.0, (int)l);
                    f << head << "\tstrain\t" << l << '\t' << fmt_f64(1.0 / scale) << '\t' << (uint64_t)o[0] << '\t' << pc << '\t' << fmt_f64(x[0]);
                    if (o[0] > 0) f << '\t' << fmt_f64(o[1]) << '\t' << fmt_f64(o[2]) << '\t' << fmt_f64(o[9]) << '\t' << fmt_f64(mx) << '\t' << fmt_f64(o[1] * scale) << '\t' << fmt_f64(o[8]);
                    else f << "\t-\t-\t-\t-\t-\t-";
                    f << '\t' << fmt_f64(mean_u64(m, 2, l)) << '\t' << fmt_f64(mean_u64(m + 1, 2, l)) << "\t-\t-\t-\t-\n";
                }
            }
            for (uint32_t k = 0; k < Su; ++k) {
                const int32_t *sk = d.status.data() + E * k;
                const std::string head = species_head(k);
                if (sk[0] != 0 && sk[0] != 1) { f << head << "\tskipped\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n"; continue; }
                for (uint64_t l = 0; l <= L; ++l) {
                    const uint64_t n = n_of(l);
                    for (uint64_t i = 0; i < n; ++i) { val[i] = d.obj[E * k + entry(l, i)]; st[i] = sk[entry(l, i)]; }
                    PTX_TRY(pantax_hip_bootstrap_summary(n, val.data(), st.data(), o));
                    f << head << "\tspecies\t" << l << '\t' << fmt_f64(1.0 / std::ldexp(1.0, (int)l)) << '\t' << (uint64_t)o[0] << "\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t"
                      << fmt_f64(mean_u64(d.reads.data() + 2 * E * k, 2, l)) << '\t' << fmt_f64(mean_u64(d.reads.data() + 2 * E * k + 1, 2, l)) << '\t'
                      << fmt_f64(mean_u64(d.rows.data() + E * k, 1, l)) << '\t' << (o[0] > 0 ? fmt_f64(o[1]) : std::string("-")) << '\n';
                }
            }
            return 0;
        });
    }
    // --strain-fragments: {compatible, unique, unique_by_pair, assigned} of every row of strain_abundance.txt, in its order; the nine classes of every species
    // of the shard in the order it went through the device (a species without rows or of more than 64: the five that need no candidate set); the discordant
    // fragments between every two rows of a species
    int fragments() const {
        const auto &fr = rep.fr;
        return file(run.p.rep.ext11_path[X11REP_FRAGMENTS],
                    "species_taxid\tstrain_taxid\tgenome_ID\tclass\tn_fragments\tn_reads\tn_steps\tspan\tfraction\tother_strain_taxid\tother_genome_ID\n",
                    "strain fragment support report", [&](std::ofstream &f) {
            const auto frac = [](uint64_t n, uint64_t of) { return of ? fmt_f64((double)n / (double)of) : std::string("-"); };
            const auto served = [&](uint32_t k) { return fr.K[k] >= 1 && fr.K[k] <= FRAG_MAX_LIST; };
            const auto sp = [&](uint32_t k, int cls) { return fr.species.data() + 3 * FRG_N_CLASSES * (size_t)k + 3 * cls; };
            const char *const of_row[FRG_N_HAP] = {"compatible", "unique", "unique_by_pair", "assigned"};
            const char *const of_species[FRG_N_CLASSES] = {"counted", "paired", "concordant", "discordant", "half", "unexplained", "single", "multi", "mate_elsewhere"};
            std::vector<const TrackRow *> row_of(fr.hap.size() / (3 * FRG_N_HAP), nullptr);   // entry -> its first row of the table
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "fragment support", &e));
                if (!row_of[e]) row_of[e] = &r;
                const std::string head = strain_head(r);
                for (int c = 0; c < (int)FRG_N_HAP; ++c) {
                    const uint64_t *q = fr.hap.data() + 3 * FRG_N_HAP * (size_t)e + 3 * c;
                    f << head << '\t' << of_row[c];
                    if (served(r.k)) f << '\t' << q[0] << '\t' << 2 * q[0] << '\t' << q[1] << '\t' << q[2] << '\t' << frac(q[0], sp(r.k, FRG_PAIRED)[0]);
                    else f << "\t-\t-\t-\t-\t-";
                    f << "\t-\t-\n";
                }
            }
            for (uint32_t k = 0; k < Su; ++k) {
                const std::string head = species_head(k);
                const uint64_t counted = sp(k, FRG_COUNTED)[0];
                for (int c = 0; c < (int)FRG_N_CLASSES; ++c) {
                    const bool of_reads = c == FRG_COUNTED || c >= FRG_SINGLE, needs_set = c >= FRG_CONCORDANT && c <= FRG_UNEXPLAINED;
                    if (needs_set && !served(k)) continue;
                    const uint64_t *q = sp(k, c), n_reads = of_reads ? q[0] : 2 * q[0];
                    f << head << '\t' << of_species[c] << '\t';
                    if (of_reads) f << '-'; else f << q[0];
                    f << '\t' << n_reads << '\t' << q[1] << '\t' << q[2] << '\t' << frac(n_reads, counted) << "\t-\t-\n";
                }
                if (fr.K[k] > FRAG_MAX_LIST) f << head << "\tskipped\t-\t-\t-\t-\t-\t-\t-\n";
            }
            for (uint32_t k = 0; k < Su; ++k) {
                const uint64_t K = fr.K[k];
                if (K < 2 || K > FRAG_MAX_LIST) continue;
                int64_t e0 = -1;                                                        // the species' entries are consecutive, in ascending haplotype index
                for (uint64_t h = sh.hap_off[k]; h < sh.hap_off[k + 1] && e0 < 0; ++h) e0 = rep.entry[h];
                const uint64_t *pm = fr.pair.data() + fr.pair_off[k];
                for (uint64_t a = 0; a < K; ++a)
                    for (uint64_t b = a + 1; b < K; ++b) {
                        const uint64_t n = pm[a * K + b];
                        if (!n || e0 < 0 || !row_of[e0 + a] || !row_of[e0 + b]) continue;
                        const TrackRow &ra = *row_of[e0 + a], &rb = *row_of[e0 + b];
                        f << strain_head(ra) << "\tdiscordant_pair\t" << n << '\t' << 2 * n << "\t-\t-\t" << frac(n, sp(k, FRG_DISCORDANT)[0]) << '\t'
                          << (rb.gr ? rb.gr->strain_taxid : std::string()) << '\t' << (rb.gr ? rb.gr->genome_id : std::string()) << '\n';
                    }
            }
            return 0;
        });
    }
    // --strain-pair-evidence: per species of the shard, in the order it went through the device, for every two of its rows a < b (ascending haplotype index)
    // what both walk (shared) and what only a, only b walks, as {n_nodes, len, covered, bases} with depth and breadth
    int pair_evidence() const {
        const auto &pe = rep.pe;
        return file(run.p.rep.pair_path[PREP_EVIDENCE],
                    "species_taxid\tstrain_taxid\tgenome_ID\tother_strain_taxid\tother_genome_ID\tclass\tn_nodes\tlen\tcovered\tbases\tdepth\tbreadth\tpredicted_coverage\tpair_class\n",
                    "strain pair evidence report", [&](std::ofstream &f) {
            std::vector<const TrackRow *> row_of(rep.n_entries, nullptr);   // entry -> its first row of the table
            for (const TrackRow &r : rows) {
                int64_t e; PTX_TRY(entry_of(r, "pair evidence", &e));
                if (!row_of[e]) row_of[e] = &r;
            }
            const auto put = [&](const TrackRow &head, const TrackRow &other, const char *cls, const uint64_t *q, double pc, const char *pair_cls) {
                f << strain_head(head) << '\t' << (other.gr ? other.gr->strain_taxid : std::string()) << '\t' << (other.gr ? other.gr->genome_id : std::string()) << '\t' << cls << '\t'
                  << q[0] << '\t' << q[1] << '\t' << q[2] << '\t' << q[3] << '\t';
                if (q[1]) f << fmt_f64((double)q[3] / (double)q[1]) << '\t' << fmt_f64((double)q[2] / (double)q[1]);
                else f << "-\t-";
                f << '\t' << fmt_f64(pc) << '\t' << pair_cls << '\n';
            };
            for (uint32_t k = 0; k < Su; ++k) {
                const uint64_t K = pe.K[k];
                if (K < 2) continue;
                if (K > HAP_PAIRS_MAX_K) { f << species(k) << "\t-\t-\t-\t-\tskipped\t-\t-\t-\t-\t-\t-\t-\t-\n"; continue; }
                int64_t e0 = -1;                                                        // the species' entries are consecutive, in ascending haplotype index
                for (uint64_t h = sh.hap_off[k]; h < sh.hap_off[k + 1] && e0 < 0; ++h) e0 = rep.entry[h];
                const uint64_t *pm = pe.pair.data() + 4 * pe.pair_off[k];
                for (uint64_t a = 0; a < K; ++a)
                    for (uint64_t b = a + 1; b < K; ++b) {
                        if (e0 < 0 || !row_of[e0 + a] || !row_of[e0 + b]) continue;
                        const TrackRow &ra = *row_of[e0 + a], &rb = *row_of[e0 + b];
                        const uint64_t *aa = pm + 4 * (a * K + a), *bb = pm + 4 * (b * K + b), *ab = pm + 4 * (a * K + b);
                        uint64_t only_a[4], only_b[4];
                        for (int q = 0; q < 4; ++q) { only_a[q] = aa[q] - ab[q]; only_b[q] = bb[q] - ab[q]; }
                        const char *const pc = hap_pair_class(only_a[1], only_b[1]);
                        const double sa = sh.met[ra.hap].second_sol, sb = sh.met[rb.hap].second_sol;
                        put(ra, rb, "shared", ab, sa + sb, pc);
                        put(ra, rb, "only", only_a, sa, pc);
                        put(rb, ra, "only", only_b, sb, pc);
                    }
            }
            return 0;
        });
    }
};
}  // namespace

namespace reports {
void begin(const ReportPlan &plan, uint32_t Su, uint64_t H, uint64_t R, ReportData &rep) {
    if (plan.any_run()) rep.entry.assign(H, -1);
    if (plan.run[REP_READ_STRAINS]) { rep.rs.hap.assign(R, ~0ull); rep.rs.n.assign(R, -1); rep.rs.post.assign(R, 0.0); }
    if (plan.run[REP_EVIDENCE]) rep.ev.species.assign(3 * EVIDENCE_N * (size_t)Su, 0);
    if (plan.run[REP_READ_SUPPORT]) { rep.sup.species.assign(12 * (size_t)Su, 0); rep.sup.pair_off.assign(Su, 0); rep.sup.K.assign(Su, 0); }
    if (plan.run[REP_DEPTH]) rep.dp.species.assign(2 * DEPTH_N * (size_t)Su, 0);
    if (plan.run[REP_NEAR_MISS]) { rep.nm.species.assign(12 * (size_t)Su, 0); rep.nm.row_off.assign(Su + 1, 0); }
    if (plan.pair_run[PREP_EVIDENCE]) { rep.pe.pair_off.assign(Su, 0); rep.pe.K.assign(Su, 0); }
    if (plan.ext_run[XREP_FIT]) rep.ft.species.assign(3 * FIT_N * (size_t)Su, 0);
    if (plan.ext2_run[X2REP_BOOTSTRAP]) {
        rep.bs.R = (uint64_t)plan.bs_replicates + 1;
        rep.bs.obj.assign(rep.bs.R * Su, 0.0); rep.bs.rows.assign(rep.bs.R * Su, 0); rep.bs.status.assign(rep.bs.R * Su, 1);
    }
    if (plan.ext3_run[X3REP_DROPOUT]) { rep.dr.rows.assign(Su, 0); rep.dr.obj.assign(Su, 0.0); rep.dr.status.assign(Su, 1); rep.dr.K.assign(Su, 0); }
    if (plan.ext4_run[X4REP_ADDIN]) {
        rep.ai.rows.assign(Su, 0); rep.ai.novel.assign(Su, 0); rep.ai.obj.assign(Su, 0.0); rep.ai.status.assign(Su, 1); rep.ai.K.assign(Su, 0); rep.ai.row_off.assign(Su + 1, 0);
    }
    if (plan.ext5_run[X5REP_EM]) {
        rep.em.species.assign(6 * (size_t)Su, 0); rep.em.cls_off.assign(Su + 1, 0); rep.em.K.assign(Su, 0); rep.em.iter.assign(Su, 0); rep.em.conv.assign(Su, 0); rep.em.delta.assign(Su, 0.0);
    }
    if (plan.ext8_run[X8REP_RESCUE]) {
        rep.rc.species.assign(3 * RES_N_CLASSES * (size_t)Su, 0); rep.rc.step.assign(3 * (size_t)Su, 0); rep.rc.row_off.assign(Su + 1, 0); rep.rc.open.assign(Su, 0);
    }
    if (plan.ext10_run[X10REP_RAREFY]) {
        rep.rf.E = 1 + (uint64_t)plan.rf_replicates * plan.rf_levels;
        rep.rf.obj.assign(rep.rf.E * Su, 0.0); rep.rf.rows.assign(rep.rf.E * Su, 0); rep.rf.status.assign(rep.rf.E * Su, 1); rep.rf.reads.assign(2 * rep.rf.E * Su, 0);
    }
    if (plan.ext9_run[X9REP_LINKS]) {
        rep.lk.species.assign(LNK_N_SPECIES * (size_t)Su, 0); rep.lk.link.assign(LNK_N_TABLE * (size_t)Su, 0); rep.lk.open.assign(Su, 0);
    }
    if (plan.ext11_run[X11REP_FRAGMENTS]) {
        rep.fr.species.assign(3 * FRG_N_CLASSES * (size_t)Su, 0); rep.fr.pair_off.assign(Su, 0); rep.fr.K.assign(Su, 0); rep.fr.status.assign(Su, 1);
    }
    if (plan.ext7_run[X7REP_MOSAIC]) {
        rep.mo.species.assign(3 * MOS_N_CLASSES * (size_t)Su, 0); rep.mo.extra.assign(3 * (size_t)Su, 0); rep.mo.pair_off.assign(Su, 0); rep.mo.K.assign(Su, 0); rep.mo.jn_off.assign(Su + 1, 0);
    }
}
int collect_group(Run &run, const Ingest &in, const Selection &sn, pantax_hip_db *db, uint32_t k0, uint32_t k1, ShardResult &sh) {
    const ReportPlan &plan = run.p.rep;
    if (!plan.any_run()) return 0;
    GroupSel g;
    GroupCand gc;
    PTX_TRY(group_select(run, k0, k1, sh, g));
    if (plan.run[REP_READ_STRAINS]) PTX_TRY(group_read_strains(run, in, db, k0, k1, g, sh));
    if (plan.run[REP_COVERAGE]) PTX_TRY(group_cov_track(run, db, k0, k1, g, sh));
    if (plan.ext6_run[X6REP_SEGMENTS]) PTX_TRY(group_segments(run, db, k0, k1, g, sh));
    if (plan.ext12_run[X12REP_GROWTH]) PTX_TRY(group_growth(run, db, k0, k1, g, sh));
    if (plan.run[REP_EVIDENCE]) PTX_TRY(group_node_sums(run, db, k0, k1, g, pantax_hip_strain_evidence, 2 * EVIDENCE_N, 3 * EVIDENCE_N, sh.rep.ev, "  strain evidence"));
    if (plan.ext_run[XREP_FIT]) PTX_TRY(group_fit(run, db, k0, k1, g, sh));
    if (plan.ext2_run[X2REP_BOOTSTRAP]) PTX_TRY(group_bootstrap(run, in, sn, db, k0, k1, g, sh));
    if (plan.ext3_run[X3REP_DROPOUT]) PTX_TRY(group_dropout(run, db, k0, k1, g, sh));
    if (plan.ext4_run[X4REP_ADDIN]) PTX_TRY(group_addin(run, db, k0, k1, g, sh, gc));
    if (plan.pair_run[PREP_EVIDENCE]) PTX_TRY(group_pair_evidence(run, db, k0, k1, g, sh));
    if (plan.run[REP_READ_SUPPORT]) PTX_TRY(group_read_support(run, in, db, k0, k1, g, sh));
    if (plan.ext5_run[X5REP_EM]) PTX_TRY(group_read_em(run, in, db, k0, k1, g, sh));
    if (plan.ext7_run[X7REP_MOSAIC]) PTX_TRY(group_mosaic(run, in, db, k0, k1, g, sh));
    if (plan.ext8_run[X8REP_RESCUE]) PTX_TRY(group_rescue(run, in, db, k0, k1, g, sh, gc));
    if (plan.ext9_run[X9REP_LINKS]) PTX_TRY(group_links(run, in, db, k0, k1, g, sh));
    if (plan.ext10_run[X10REP_RAREFY]) PTX_TRY(group_rarefy(run, in, db, k0, k1, g, sh));
    if (plan.ext11_run[X11REP_FRAGMENTS]) PTX_TRY(group_fragments(run, in, db, k0, k1, g, sh));
    if (plan.run[REP_DEPTH]) PTX_TRY(group_node_sums(run, db, k0, k1, g, pantax_hip_strain_depth, 2 * DEPTH_N, 2 * DEPTH_N, sh.rep.dp, "  strain depth"));
    if (plan.run[REP_NEAR_MISS]) PTX_TRY(group_near_miss(run, db, k0, k1, g, sh, gc));
    return 0;
}
int write(Run &run, const Ingest &in, const Selection &sn, const ShardResult &sh, const std::vector<GenomeRow> &genomes, std::vector<TrackRow> &rows) {
    const ReportPlan &plan = run.p.rep;
    if (!plan.any_run()) return 0;
    std::stable_sort(rows.begin(), rows.end(), [](const TrackRow &a, const TrackRow &b) { return a.key > b.key; });   // the table's own sort on the same keys
    Writer w{run, in, sn, sh, genomes, rows, {}};
    for (size_t i = genomes.size(); i-- > 0;) w.first_genome[genomes[i].hap_id] = i;
    if (plan.run[REP_READ_STRAINS]) PTX_TRY(w.read_strains());
    if (plan.run[REP_COVERAGE]) PTX_TRY(w.cov_track());
    if (plan.run[REP_EVIDENCE]) PTX_TRY(w.evidence());
    if (plan.run[REP_READ_SUPPORT]) PTX_TRY(w.read_support());
    if (plan.run[REP_DEPTH]) PTX_TRY(w.depth());
    if (plan.run[REP_NEAR_MISS]) PTX_TRY(w.near_miss());
    if (plan.pair_run[PREP_EVIDENCE]) PTX_TRY(w.pair_evidence());
    if (plan.ext_run[XREP_FIT]) PTX_TRY(w.fit());
    if (plan.ext2_run[X2REP_BOOTSTRAP]) PTX_TRY(w.bootstrap());
    if (plan.ext3_run[X3REP_DROPOUT]) PTX_TRY(w.dropout());
    if (plan.ext4_run[X4REP_ADDIN]) PTX_TRY(w.addin());
    if (plan.ext5_run[X5REP_EM]) PTX_TRY(w.read_em());
    if (plan.ext6_run[X6REP_SEGMENTS]) PTX_TRY(w.segments());
    if (plan.ext7_run[X7REP_MOSAIC]) PTX_TRY(w.mosaic());
    if (plan.ext8_run[X8REP_RESCUE]) PTX_TRY(w.rescue());
    if (plan.ext9_run[X9REP_LINKS]) PTX_TRY(w.links());
    if (plan.ext10_run[X10REP_RAREFY]) PTX_TRY(w.rarefy());
    if (plan.ext11_run[X11REP_FRAGMENTS]) PTX_TRY(w.fragments());
    if (plan.ext12_run[X12REP_GROWTH]) PTX_TRY(w.growth());
    return 0;
}
}  // namespace reports
}  // namespace ptx
