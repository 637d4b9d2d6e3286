// api_profile.cpp -- the pipeline seam: pantax_hip_profile(cfg) == profile::profile(ProfilingConfig)
// (profile.rs:3325-3436): files in (GAF + DB files), files out (species_abundance.txt,
// strain_abundance.txt, ori_strain_abundance.txt, optional reads_classification.tsv).
// Host orchestration only; every per-read / per-node computation goes through the device stages.
// profile_impl (at the end) is the sequence of the phases, functions of the structs of profile_run.hpp; the shard phase is profile_shard.cpp, the ranks
// meet in RankComm (profile_comm.hpp), the I/O-free decisions are in profile_pure.cpp, the per-strain reports in report_plan.cpp / profile_reports.cpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <unordered_map>
#include <unordered_set>
#include "primitives.hpp"
#include "profile_run.hpp"

using namespace ptx;

namespace {

bool is_dir(const std::string &p) { struct stat st; return !p.empty() && stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }
std::string opt(const char *s) { return s ? std::string(s) : std::string(); }
// choose_existing_file_from_two_files (profile.rs:107-134): explicit path wins, else the DB default
std::string choose(const std::string &a, const std::string &b) { return is_file(a) ? a : (is_file(b) ? b : std::string()); }
// first line start at or after byte `c` of the mapped text (a line starts at 0 or right after a '\n')
uint64_t line_start_at_or_after(const MappedFile &mf, uint64_t c) {
    if (c == 0) return 0;
    if (c >= mf.size) return mf.size;
    const void *nl = std::memchr(mf.data + (c - 1), '\n', mf.size - (c - 1));
    return nl ? (uint64_t)(static_cast<const char *>(nl) - mf.data) + 1 : mf.size;
}
// ---- check_args_valid (profile.rs:71-199): everything here fails alike on every rank, before the first collective
int check_args(Run &run) {
    pantax_hip_ctx *ctx = run.ctx; const pantax_hip_profiling_config *cfg = run.cfg; RunPlan &p = run.p; RankComm &c = run.comm;
    if (!cfg->species && !cfg->strain) return fail(ctx, PANTAX_HIP_E_INVALID, "Please choose profiling level with --species or/and --strain.");
    // one process per GPU: the selected species are packed onto the ranks by weight; the two global sums of the strain table
    // (profile.rs:3198, :3243) and the hand-over of the rows go through the caller's all-reduce (RCCL / MPI / ...).  With an
    // alltoallv callback the input is sharded as well: every rank tokenises and bins its byte range of the GAF.
    const int W = c.W = cfg->world_size > 1 ? cfg->world_size : 1;
    c.rk = W > 1 ? cfg->rank : 0;
    if (W > 1 && (!cfg->allreduce_sum || c.rk < 0 || c.rk >= W)) return fail(ctx, PANTAX_HIP_E_INVALID, "profile: world_size %d needs 0 <= rank < world_size and an allreduce_sum callback", W);
    // a one-rank world that is given the callbacks still goes through them (like an MPI program started on one rank): the
    // whole multi-rank protocol, sharded ingest included, can be exercised on a single GPU
    c.use_comm = W > 1 || (cfg->world_size == 1 && cfg->allreduce_sum != nullptr);
    p.sharded = c.use_comm && cfg->alltoallv != nullptr;
    if (p.sharded && W > 64) return fail(ctx, PANTAX_HIP_E_LIMIT, "profile: the sharded ingest routes reads to at most 64 ranks (world_size %d)", W);
    std::string rep_err;   // the per-strain reports: wanted? one rank and an unsharded ingest; their two parameters (report_plan.cpp)
    if (!plan_reports(cfg, W, p.sharded, p.rep, rep_err) || !plan_ext_reports(run.ext, W, p.sharded, p.rep, rep_err)) return fail(ctx, PANTAX_HIP_E_INVALID, "%s", rep_err.c_str());
    p.db_dir = opt(cfg->db); p.wd = opt(cfg->wd); p.out_dir = opt(cfg->output_dir);
    if (p.out_dir.empty()) p.out_dir = p.wd;
    if (!is_dir(p.db_dir)) return fail(ctx, PANTAX_HIP_E_IO, "Specified PanTax database directory '%s' is not a valid directory path", p.db_dir.c_str());
    if (!is_dir(p.wd)) return fail(ctx, PANTAX_HIP_E_IO, "Specified PanTax work directory '%s' is not a valid directory path", p.wd.c_str());
    if (cfg->sample_nodes < 0) return fail(ctx, PANTAX_HIP_E_INVALID, "profile: --sample %d", cfg->sample_nodes);
    if (cfg->solver_semantics != PANTAX_HIP_SEMANTICS_GUROBI && cfg->solver_semantics != PANTAX_HIP_SEMANTICS_HIGHS) return fail(ctx, PANTAX_HIP_E_INVALID, "profile: solver_semantics %d", cfg->solver_semantics);
    if (!(cfg->minimization_min_cov >= 0.0) || !std::isfinite(cfg->minimization_min_cov)) return fail(ctx, PANTAX_HIP_E_INVALID, "profile: minimization_min_cov %g", cfg->minimization_min_cov);
    p.zip = opt(cfg->zip);
    if (p.zip == "h5")
        return fail(ctx, PANTAX_HIP_E_LIMIT, "profile: graph container '%s' is not available in this build (the reference gates it behind a cargo feature); use serialize / lz / zstd or GFA", p.zip.c_str());
    p.species_file = path_join(p.wd, "species_abundance.txt"); p.strain_file = path_join(p.wd, "strain_abundance.txt");
    p.report = opt(cfg->out_binning_file); p.gaf_path = opt(cfg->input_aln_file);
    return 0;
}
// which levels this call runs, from the outputs already in the work directory (profile.rs:3419-3427)
int decide_resume(Run &run) {
    const bool species_exists = !run.cfg->force && is_file(run.p.species_file);
    const bool strain_exists = !run.cfg->force && is_file(run.p.strain_file);
    run.p.full_path = run.cfg->species && !species_exists;
    run.p.strain_only = !run.p.full_path && run.cfg->strain && !strain_exists;
    run.p.strain_done = strain_exists;
    if (run.comm.use_comm) {   // rank 0 looked at the work directory before anybody wrote to it: every rank follows its decision
        double d[3] = {run.comm.rk == 0 && run.p.full_path ? 1.0 : 0.0, run.comm.rk == 0 && run.p.strain_only ? 1.0 : 0.0, run.comm.rk == 0 && run.p.strain_done ? 1.0 : 0.0};
        PTX_TRY(run.comm.allreduce(d, 3));
        run.p.full_path = d[0] != 0.0; run.p.strain_only = d[1] != 0.0; run.p.strain_done = d[2] != 0.0;
    }
    resume_reports(run.p.rep, run.cfg->strain, run.p.full_path, run.p.strain_done);
    run.p.want_report = run.p.full_path && !run.p.report.empty() && run.p.report != "None";
    return 0;
}
void rs_skipped(const RunPlan &p) {
    for (int i = 0; i < N_REPORTS; ++i)
        if (p.rep.want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.path[i].c_str());
    for (int i = 0; i < N_PAIR_REPORTS; ++i)
        if (p.rep.pair_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.pair_path[i].c_str());
    for (int i = 0; i < N_EXT_REPORTS; ++i)
        if (p.rep.ext_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext_path[i].c_str());
    for (int i = 0; i < N_EXT2_REPORTS; ++i)
        if (p.rep.ext2_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext2_path[i].c_str());
    for (int i = 0; i < N_EXT3_REPORTS; ++i)
        if (p.rep.ext3_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext3_path[i].c_str());
    for (int i = 0; i < N_EXT4_REPORTS; ++i)
        if (p.rep.ext4_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext4_path[i].c_str());
    for (int i = 0; i < N_EXT5_REPORTS; ++i)
        if (p.rep.ext5_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext5_path[i].c_str());
    for (int i = 0; i < N_EXT6_REPORTS; ++i)
        if (p.rep.ext6_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext6_path[i].c_str());
    for (int i = 0; i < N_EXT7_REPORTS; ++i)
        if (p.rep.ext7_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext7_path[i].c_str());
    for (int i = 0; i < N_EXT8_REPORTS; ++i)
        if (p.rep.ext8_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext8_path[i].c_str());
    for (int i = 0; i < N_EXT9_REPORTS; ++i)
        if (p.rep.ext9_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext9_path[i].c_str());
    for (int i = 0; i < N_EXT10_REPORTS; ++i)
        if (p.rep.ext10_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext10_path[i].c_str());
    for (int i = 0; i < N_EXT11_REPORTS; ++i)
        if (p.rep.ext11_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext11_path[i].c_str());
    for (int i = 0; i < N_EXT12_REPORTS; ++i)
        if (p.rep.ext12_want[i]) std::fprintf(stderr, "[pantax_hip_profile] note: no strain step ran in this call; %s was not written\n", p.rep.ext12_path[i].c_str());
}
// ---- a1 + a2/a3, rank-local: ranges, GAF (this rank's byte range when sharded) -> packed reads in HBM, binned against
// ALL species ranges (ranges-only db), counters on the device
int ingest_local(Run &run, Ingest &in) {
    if (!is_file(run.p.gaf_path)) return fail(run.ctx, PANTAX_HIP_E_IO, "Specified GAF mapping file '%s' is not a valid file path", run.p.gaf_path.c_str());
    const std::string range_path = choose(opt(run.cfg->range_file), path_join(run.p.db_dir, "species_range.txt"));
    if (range_path.empty()) return fail(run.ctx, PANTAX_HIP_E_IO, "Neither species range file '%s' nor '%s' is a valid file path", opt(run.cfg->range_file).c_str(), path_join(run.p.db_dir, "species_range.txt").c_str());
    std::string err = read_species_range(range_path, in.ranges);
    if (!err.empty()) return fail(run.ctx, PANTAX_HIP_E_IO, "%s", err.c_str());
    const uint32_t S = in.S = (uint32_t)in.ranges.size();
    if (S == 0) return fail(run.ctx, PANTAX_HIP_E_IO, "species range file %s is empty", range_path.c_str());
    err = in.mf.open(run.p.gaf_path);
    if (!err.empty()) return fail(run.ctx, PANTAX_HIP_E_IO, "%s", err.c_str());
    // tokenised on the device (stage_gaf.hip; host_io.cpp:parse_gaf is its checker): the packed reads stay in HBM,
    // only read_len / mapq / flags / id hashes come back for the report and the duplicate-id rule
    uint64_t text_end = in.mf.size;
    if (run.p.sharded) {
        in.text_begin = line_start_at_or_after(in.mf, in.mf.size / (uint64_t)run.comm.W * (uint64_t)run.comm.rk);
        text_end = run.comm.rk + 1 == run.comm.W ? in.mf.size : line_start_at_or_after(in.mf, in.mf.size / (uint64_t)run.comm.W * (uint64_t)(run.comm.rk + 1));
    }
    in.reads.rd = new pantax_hip_reads();
    // The per-read host columns (read_len, mapq, flags, id hash: 14 bytes per read) and the species of every read come back over PCIe only
    // for a caller that uses them: the binning report, the strain-only resume, the sharded ingest -- or, later, the duplicate-id rule when
    // two reads do share an id (host_cols below).  A plain run on distinct ids needs the species COUNTERS and the first rows only.
    // (no locus-grouped copy yet: the species decision needs the counters only -- the plain columns are binned in file order --, and the copy is
    // built while the first graphs travel, on an otherwise idle device; round 5 built it here, 27 ms behind the last byte of the GAF at 1e8 reads)
    PTX_TRY(gaf_tokenize_device(run.ctx, in.mf.data + in.text_begin, text_end - in.text_begin, in.hr, in.reads.rd, in.mf.fd, in.text_begin, /*group=*/false,
                                /*want_id_spans=*/run.p.want_report || run.p.rep.run[REP_READ_STRAINS] || run.p.rep.ext11_run[X11REP_FRAGMENTS],
                                /*want_host_columns=*/false));
    in.R = in.R_all = in.reads.rd->R;
    run.lap("ranges + GAF tokenise");
    in.rs.resize(S); in.re.resize(S);
    for (uint32_t s = 0; s < S; ++s) { in.rs[s] = in.ranges[s].start; in.re[s] = in.ranges[s].end; }
    pantax_hip_graphs g{};
    g.n_species = S; g.range_start = in.rs.data(); g.range_end = in.re.data();
    PTX_TRY(pantax_hip_db_upload(run.ctx, &g, &in.bin_db.db));
    in.rc.resize(S); in.bs.resize(S); in.lm.resize(S); in.uq.resize(S);
    PTX_TRY(pantax_hip_bin_reads(run.ctx, in.bin_db.db, in.reads.rd, nullptr, in.rc.data(), in.bs.data(), in.lm.data(), in.uq.data()));
    run.lap("bin all species");
    return 0;
}
// the host columns + the species of every read (file order), once
int host_cols(Run &run, Ingest &in) {
    if (in.have_cols) return 0;
    PTX_TRY(reads_host_columns(run.ctx, in.reads.rd, in.hr));
    in.sp_idx.resize(in.R);
    if (in.R) {
        PTX_TRY(species_ensure(run.ctx, in.reads.rd));
        PTX_TRY(download(run.ctx, in.sp_idx.data(), in.reads.rd->d_species.p, in.R));
        PTX_HIP(run.ctx, hipStreamSynchronize(run.ctx->stream));
    }
    in.have_cols = true;
    run.lap("host columns + species of every read");
    return 0;
}
// ingest: tokenise, bin all species, head rows; ends in the collective that carries its status
int ingest(Run &run, Ingest &in) {
    int local_rc = ingest_local(run, in);
    if (local_rc == 0 && (run.p.want_report || run.p.sharded || run.p.strain_only || run.p.rep.run[REP_READ_STRAINS])) local_rc = host_cols(run, in);
    // the read lengths of the first (up to 1000) binned rows of the FILE decide the equal-length branch (profile.rs:312-319): they are among the
    // first rows the binning pass hands back with its counters, unless those hold fewer than 1000 binned rows of a longer file
    if (local_rc == 0 && !in.have_cols) {
        const std::vector<int32_t> &ps = in.reads.rd->h_pre_species;
        for (size_t r = 0; r < ps.size() && in.head.size() < 1000; ++r) if (ps[r] >= 0) in.head.push_back(in.reads.rd->h_pre_qlen[r]);
        if (in.head.size() < 1000 && (uint64_t)ps.size() < in.R) { in.head.clear(); local_rc = host_cols(run, in); }
    }
    if (local_rc == 0 && in.have_cols) for (uint64_t r = 0; r < in.R && in.head.size() < 1000; ++r) if (in.sp_idx[r] >= 0) in.head.push_back(in.hr.qlen[r]);
    if (!run.p.sharded) return run.comm.agree(local_rc);
    // the sharded counter merge: {S (must agree), reads per rank, the four counters per species, every rank's head} in one all-reduce behind the failure flag
    const int W = run.comm.W, rk = run.comm.rk;
    double s_chk[2] = {local_rc != 0 ? 1.0 : 0.0, 0.0};
    PTX_TRY(run.comm.allreduce(s_chk, 1));   // S is only known to ranks that got through: settle the failure first
    if (s_chk[0] != 0.0) return local_rc ? local_rc : run.comm.others_failed();
    const uint32_t S = in.S;
    const size_t o_rank = 2, o_cnt = o_rank + W, o_head = o_cnt + 4 * (size_t)S;
    std::vector<double> x(o_head + (size_t)W * 1001, 0.0);
    x[o_rank + rk] = (double)in.R;
    for (uint32_t s = 0; s < S; ++s) { x[o_cnt + s] = (double)in.rc[s]; x[o_cnt + S + s] = (double)in.bs[s]; x[o_cnt + 2 * (size_t)S + s] = (double)in.lm[s]; x[o_cnt + 3 * (size_t)S + s] = (double)in.uq[s]; }
    x[o_head + (size_t)rk * 1001] = (double)in.head.size();
    for (size_t i = 0; i < in.head.size(); ++i) x[o_head + (size_t)rk * 1001 + 1 + i] = (double)in.head[i];
    PTX_TRY(run.comm.allreduce(x.data(), x.size()));
    in.R_all = 0;
    for (int q = 0; q < W; ++q) { if (q < rk) in.read_base += (uint64_t)x[o_rank + q]; in.R_all += (uint64_t)x[o_rank + q]; }
    for (uint32_t s = 0; s < S; ++s) { in.rc[s] = (int64_t)x[o_cnt + s]; in.bs[s] = (int64_t)x[o_cnt + S + s]; in.lm[s] = (int64_t)x[o_cnt + 2 * (size_t)S + s]; in.uq[s] = (int64_t)x[o_cnt + 3 * (size_t)S + s]; }
    in.head.clear();
    for (int q = 0; q < W && in.head.size() < 1000; ++q) {
        const size_t n = (size_t)x[o_head + (size_t)q * 1001];
        for (size_t i = 0; i < n && in.head.size() < 1000; ++i) in.head.push_back((uint32_t)x[o_head + (size_t)q * 1001 + 1 + i]);
    }
    return 0;
}
// species level of a full run: the optional binning report, species_abundance.txt
int species_from_counters(Run &run, const Ingest &in, std::vector<SpeciesProfileRow> &sp_profile) {
    const uint32_t S = in.S;
    // optional binning report: read_id, mapq, species, read_len; no header (profile.rs:3337-3351).  Sharded: every rank
    // writes the rows of its byte range to a part file, rank 0 joins them in rank (= file) order (join_report_parts).
    if (run.p.want_report && (run.comm.rk == 0 || run.p.sharded)) {
        const std::string path = run.p.sharded ? run.p.report + ".part" + std::to_string(run.comm.rk) : run.p.report;
        std::ofstream f(path);
        if (!f) return fail(run.ctx, PANTAX_HIP_E_IO, "cannot write %s", path.c_str());
        for (uint64_t r = 0; r < in.R; ++r) {
            f.write(in.mf.data + in.text_begin + in.hr.id_span[r].first, in.hr.id_span[r].second);
            f << '\t';
            if (in.hr.mapq[r] != 255) f << (int)in.hr.mapq[r];
            f << '\t' << (in.sp_idx[r] >= 0 ? in.ranges[in.sp_idx[r]].species : std::string("U")) << '\t' << in.hr.qlen[r] << '\n';
        }
        f.close();
        if (!f) return fail(run.ctx, PANTAX_HIP_E_IO, "cannot write %s", path.c_str());
    }
    const std::string len_path = choose(opt(run.cfg->species_len_file), path_join(run.p.db_dir, "species_genomes_stats.txt"));
    if (len_path.empty()) return fail(run.ctx, PANTAX_HIP_E_IO, "Neither species length file '%s' nor '%s' is a valid file path", opt(run.cfg->species_len_file).c_str(), path_join(run.p.db_dir, "species_genomes_stats.txt").c_str());
    std::vector<std::pair<std::string, double>> lens;
    std::string err = read_species_len(len_path, lens);
    if (!err.empty()) return fail(run.ctx, PANTAX_HIP_E_IO, "%s", err.c_str());
    std::unordered_map<std::string, double> len_of(lens.begin(), lens.end());
    std::vector<double> avg(S, 0.0);
    for (uint32_t s = 0; s < S; ++s) { auto it = len_of.find(in.ranges[s].species); if (it != len_of.end()) avg[s] = it->second; }
    std::vector<uint8_t> keep(S);
    std::vector<double> absolute(S), abundance(S);
    species_profile_host(S, in.head.data(), in.head.size(), in.rc.data(), in.bs.data(), in.lm.data(), in.uq.data(), avg.data(), run.cfg->filtered, keep.data(), absolute.data(), abundance.data());
    for (uint32_t s = 0; s < S; ++s) if (keep[s]) sp_profile.push_back({in.ranges[s].species, abundance[s], absolute[s]});
    std::stable_sort(sp_profile.begin(), sp_profile.end(), [](const SpeciesProfileRow &a, const SpeciesProfileRow &b) { return a.abundance > b.abundance; });   // :344
    if (run.comm.rk == 0) {
        std::ofstream f(path_join(run.p.out_dir, "species_abundance.txt"));
        if (!f) return fail(run.ctx, PANTAX_HIP_E_IO, "cannot write %s", path_join(run.p.out_dir, "species_abundance.txt").c_str());
        f << "species_taxid\tpredicted_abundance\tpredicted_coverage\n";
        for (auto &r : sp_profile) f << r.species << '\t' << fmt_f64(r.abundance) << '\t' << fmt_f64(r.coverage) << '\n';
    }
    return 0;
}
// strain only (profile.rs:3365-3417): species column comes from the saved binning file (positional join); a rank
// of the sharded ingest takes the rows of its own reads.  The species table is read back.
int species_from_files(Run &run, Ingest &in, std::vector<SpeciesProfileRow> &sp_profile) {
    std::string rb = choose(opt(run.cfg->reads_binning_file), path_join(run.p.wd, "reads_classification.tsv"));   // profile.rs:179-182
    if (rb.empty()) return fail(run.ctx, PANTAX_HIP_E_IO, "reads binning file '%s' is not a valid file path", path_join(run.p.wd, "reads_classification.tsv").c_str());
    std::unordered_map<std::string, int32_t> idx_of;
    for (uint32_t s = 0; s < in.S; ++s) idx_of.emplace(in.ranges[s].species, (int32_t)s);
    std::ifstream f(rb);
    std::string line;
    uint64_t row = 0;
    while (std::getline(f, line)) {
        if (row >= in.R_all) return fail(run.ctx, PANTAX_HIP_E_IO, "%s has more rows than the GAF (%llu)", rb.c_str(), (unsigned long long)in.R_all);
        if (row >= in.read_base && row < in.read_base + in.R) {
            size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1), t3 = t2 == std::string::npos ? t2 : line.find('\t', t2 + 1);
            if (t2 == std::string::npos) return fail(run.ctx, PANTAX_HIP_E_IO, "malformed row in %s", rb.c_str());
            std::string spn = line.substr(t2 + 1, t3 == std::string::npos ? std::string::npos : t3 - t2 - 1);
            auto it = idx_of.find(spn);
            in.sp_idx[row - in.read_base] = it == idx_of.end() ? -1 : it->second;
        }
        ++row;
    }
    if (row != in.R_all) return fail(run.ctx, PANTAX_HIP_E_IO, "%s has %llu rows but the GAF has %llu (the join is positional, profile.rs:3381-3384)", rb.c_str(), (unsigned long long)row, (unsigned long long)in.R_all);
    if (!is_file(run.p.species_file)) return fail(run.ctx, PANTAX_HIP_E_IO, "species abundance file '%s' is not a valid file path", run.p.species_file.c_str());
    std::ifstream sf(run.p.species_file);
    bool header = true;
    while (std::getline(sf, line)) {
        if (header) { header = false; continue; }
        const size_t t1 = line.find('\t');
        const size_t t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
        if (t1 == std::string::npos || t2 == std::string::npos) continue;
        const std::string c1 = line.substr(t1 + 1, t2 - t1 - 1), c2 = line.substr(t2 + 1);
        char *e1 = nullptr, *e2 = nullptr;
        const double v1 = std::strtod(c1.c_str(), &e1), v2 = std::strtod(c2.c_str(), &e2);
        if (e1 == c1.c_str() || e2 == c2.c_str()) return fail(run.ctx, PANTAX_HIP_E_IO, "malformed row in %s: '%s'", run.p.species_file.c_str(), line.c_str());
        sp_profile.push_back({line.substr(0, t1), v1, v2});
    }
    return 0;
}
// rank 0 of a sharded run, behind the barrier: the parts of the binning report in rank order = file order
int join_report_parts(Run &run) {
    if (!(run.p.want_report && run.p.sharded && run.comm.rk == 0)) return 0;
    std::ofstream out(run.p.report, std::ios::binary);
    bool ok = (bool)out;
    for (int r = 0; r < run.comm.W && ok; ++r) {
        const std::string part = run.p.report + ".part" + std::to_string(r);
        std::ifstream in(part, std::ios::binary);
        ok = (bool)in;
        if (ok && in.peek() != std::ifstream::traits_type::eof()) out << in.rdbuf();
        in.close();
        std::remove(part.c_str());
    }
    out.close();
    return !ok || !out ? fail(run.ctx, PANTAX_HIP_E_IO, "cannot join the parts of %s", run.p.report.c_str()) : 0;
}
// ---- a4: load_species_range (profile.rs:553-656).  false: no species is left behind the mode / designated filter
bool select_species(const pantax_hip_profiling_config *cfg, const Ingest &in, const std::vector<SpeciesProfileRow> &sp_profile, Selection &sn) {
    std::set<std::string> ds;
    const std::string ds_s = opt(cfg->designated_species);
    if (!ds_s.empty() && ds_s != "None") {
        std::stringstream ss(ds_s);
        std::string tok;
        while (std::getline(ss, tok, ',')) {
            size_t b = tok.find_first_not_of(" \t"), e = tok.find_last_not_of(" \t");
            if (b != std::string::npos) ds.insert(tok.substr(b, e - b + 1));
        }
    }
    std::unordered_map<std::string, uint32_t> range_idx;
    for (uint32_t s = 0; s < in.S; ++s) range_idx.emplace(in.ranges[s].species, s);
    bool any_after_ds = false;
    for (auto &row : in.ranges) any_after_ds = any_after_ds || species_wanted(cfg->mode, ds, row);
    if (!any_after_ds) return false;
    for (auto &row : sp_profile) {
        if (!(row.abundance > cfg->min_species_abundance)) continue;                 // :602
        auto it = range_idx.find(row.species);
        if (it == range_idx.end()) continue;                                         // inner join :604-605
        if (!species_wanted(cfg->mode, ds, in.ranges[it->second])) continue;
        sn.sel.push_back(it->second);
        sn.sel_cov.push_back(row.coverage);
    }
    return true;
}
// (hash, value) records by hash: beyond 65536 on the device (stable LSD radix sort, the payload word rides along)
int sort_id_records(pantax_hip_ctx *ctx, std::vector<uint64_t> &kh, std::vector<uint64_t> &kv) {
    const uint64_t n = kh.size();
    if (n > 65536) {
        DevBuf<uint64_t> a0, a1, b0, b1;
        DevBuf<uint32_t> table, tmp;
        PTX_TRY(upload(ctx, a0, kh.data(), n)); PTX_TRY(upload(ctx, a1, kv.data(), n));
        PTX_HIP(ctx, b0.alloc(n)); PTX_HIP(ctx, b1.alloc(n)); PTX_HIP(ctx, table.alloc(sort_table_elems(n))); PTX_HIP(ctx, tmp.alloc(16));
        SortBufs A, B;
        A.nw = B.nw = 2; A.k[0] = a0.p; A.k[1] = a1.p; B.k[0] = b0.p; B.k[1] = b1.p;
        std::vector<SortPass> passes;
        add_passes(passes, 0, 0, 64);
        bool in_b = false;
        PTX_TRY(radix_sort(ctx, A, B, n, passes.data(), (int)passes.size(), table.p, tmp.p, &in_b, nullptr));
        PTX_TRY(download(ctx, kh.data(), in_b ? b0.p : a0.p, n)); PTX_TRY(download(ctx, kv.data(), in_b ? b1.p : a1.p, n));
        PTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        std::vector<uint32_t> ord(n);
        for (uint64_t i = 0; i < n; ++i) ord[i] = (uint32_t)i;
        std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return kh[a] < kh[b]; });
        std::vector<uint64_t> h2(n), v2(n);
        for (uint64_t i = 0; i < n; ++i) { h2[i] = kh[ord[i]]; v2[i] = kv[ord[i]]; }
        kh.swap(h2); kv.swap(v2);
    }
    return 0;
}
// The same rule over N byte ranges: the alignments of one read id may sit in different ranks' slices, so every binned read sends (id hash, species, complete?)
// to the rank its hash selects; that rank sees ALL records of the id, decides "some id repeats" (the reference's `unique` flag, which covers incomplete rows too)
// and "this id spans species" (over complete rows); only when some id does repeat, the ids to drop are made known to every rank.
int duplicate_ids_sharded(Run &run, const Ingest &in, Selection &sn) {
    const int W = run.comm.W, rk = run.comm.rk;
    const HostReads &hr = in.hr;
    struct IdRec { uint64_t hash; int32_t sp; uint32_t complete; };
    auto dest_of = [W](uint64_t h) { return (int)(((h * 0x9E3779B97F4A7C15ull) >> 33) % (uint64_t)W); };
    std::vector<uint64_t> send_off(W + 1, 0), recv_off, cur(W, 0);
    for (uint64_t r = 0; r < in.R; ++r) if (in.sp_idx[r] >= 0) ++cur[dest_of(hr.id_hash[r])];
    for (int j = 0; j < W; ++j) { send_off[j + 1] = send_off[j] + cur[j] * sizeof(IdRec); cur[j] = send_off[j] / sizeof(IdRec); }
    std::vector<IdRec> sendv(send_off[W] / sizeof(IdRec));
    for (uint64_t r = 0; r < in.R; ++r)
        if (in.sp_idx[r] >= 0) sendv[cur[dest_of(hr.id_hash[r])]++] = IdRec{hr.id_hash[r], in.sp_idx[r], sn.flags[r] ? 0u : 1u};
    PTX_TRY(run.comm.exchange_sizes(send_off.data(), recv_off, 0));
    std::vector<uint8_t> recvb;
    PTX_TRY(run.comm.a2a_host(sendv.data(), send_off.data(), recvb, recv_off.data()));
    const uint64_t n = recv_off[W] / sizeof(IdRec);
    std::vector<uint64_t> kh(n), kv(n), mixed;
    const IdRec *rec = reinterpret_cast<const IdRec *>(recvb.data());
    for (uint64_t i = 0; i < n; ++i) { kh[i] = rec[i].hash; kv[i] = ((uint64_t)rec[i].complete << 32) | (uint32_t)rec[i].sp; }
    const int local_rc = sort_id_records(run.ctx, kh, kv);   // travels in y[0]
    const bool dup_any = local_rc == 0 && mixed_ids(kh, kv, mixed);
    std::vector<double> y(2 + (size_t)W, 0.0);
    y[0] = local_rc != 0 ? 1.0 : 0.0; y[1] = dup_any ? 1.0 : 0.0; y[2 + rk] = (double)mixed.size();
    PTX_TRY(run.comm.allreduce(y.data(), y.size()));
    if (y[0] != 0.0) return local_rc ? local_rc : run.comm.others_failed();
    uint64_t n_mixed_all = 0;
    for (int q = 0; q < W; ++q) n_mixed_all += (uint64_t)y[2 + q];
    if (y[1] != 0.0 && n_mixed_all) {   // process_with_duplicates: ids whose complete alignments span species are dropped everywhere
        std::vector<uint64_t> so2(W + 1, 0), ro2(W + 1, 0), mine((size_t)W * mixed.size());
        for (int j = 0; j < W; ++j) {
            so2[j + 1] = so2[j] + mixed.size() * 8; ro2[j + 1] = ro2[j] + (uint64_t)y[2 + j] * 8;
            std::copy(mixed.begin(), mixed.end(), mine.begin() + (size_t)j * mixed.size());
        }
        std::vector<uint8_t> allb;
        PTX_TRY(run.comm.a2a_host(mine.data(), so2.data(), allb, ro2.data()));
        const uint64_t *am = reinterpret_cast<const uint64_t *>(allb.data());
        std::unordered_set<uint64_t> drop(am, am + n_mixed_all);
        for (uint64_t r = 0; r < in.R; ++r) if (in.sp_idx[r] >= 0 && drop.count(hr.id_hash[r])) sn.flags[r] |= PANTAX_HIP_READ_DUPDROP;
    }
    return 0;
}
// ---- a5: rows with a null field are dropped; duplicate read ids (profile.rs:361-463).  When no two reads share an id hash -- short reads -- the flags the
// tokenizer left on the device stand and no per-read column visits the host.  `pending`: this rank's status since the last collective, settled here.
int duplicate_ids(Run &run, Ingest &in, Selection &sn, int pending) {
    if (pending == 0 && !run.p.sharded && in.hr.ids_distinct != 1) pending = host_cols(run, in);
    PTX_TRY(run.comm.agree(pending));
    sn.flags = in.hr.flags;
    if (run.p.strain_only) { sn.flags_dirty = true; for (uint64_t r = 0; r < in.R; ++r) if (in.sp_idx[r] < 0) sn.flags[r] |= PANTAX_HIP_READ_NULLFIELD; }   // "U" in the saved report
    if (run.p.sharded) return duplicate_ids_sharded(run, in, sn);
    const HostReads &hr = in.hr;
    const std::vector<int32_t> &sp_idx = in.sp_idx;
    if (hr.ids_distinct == 1) return 0;   // the device tokenizer has already sorted the id hashes: when no two reads share one, nothing can repeat
    std::unordered_set<uint64_t> seen;
    seen.reserve(in.R * 2);
    bool unique = true;
    for (uint64_t r = 0; r < in.R && unique; ++r) if (sp_idx[r] >= 0 && !seen.insert(hr.id_hash[r]).second) unique = false;
    if (unique) return 0;   // else process_with_duplicates: an id is kept only if all of its (complete) alignments sit in one species
    std::unordered_map<uint64_t, int32_t> first;
    std::unordered_set<uint64_t> mixed;
    for (uint64_t r = 0; r < in.R; ++r) {
        if (sp_idx[r] < 0 || sn.flags[r]) continue;
        auto ins = first.emplace(hr.id_hash[r], sp_idx[r]);
        if (!ins.second && ins.first->second != sp_idx[r]) mixed.insert(hr.id_hash[r]);
    }
    for (uint64_t r = 0; r < in.R; ++r) if (sp_idx[r] >= 0 && mixed.count(hr.id_hash[r])) { sn.flags[r] |= PANTAX_HIP_READ_DUPDROP; sn.flags_dirty = true; }
    return 0;
}
// ---- the packed records of this rank's slice travel to the rank that owns their species; what arrives becomes this rank's resident reads
// (one-process read order restricted to its species).  Dropped rows, "U" reads and reads of unselected species stay behind -- none of them reaches
// get_node_abundances in the reference either.  *unpack_rc: the status of the unpacking, for the next collective.
int route_reads(Run &run, Ingest &in, const Selection &sn, int *unpack_rc) {
    const int W = run.comm.W, rk = run.comm.rk;
    Route rt;
    std::vector<uint64_t> send_off(W + 1, 0);
    auto pack = [&]() -> int {
        std::vector<int32_t> owner_all(in.S, -1);
        for (size_t i = 0; i < sn.sel.size(); ++i) owner_all[sn.sel[i]] = sn.owner[i];
        if (in.R) PTX_TRY(upload(run.ctx, in.reads.rd->d_flags, sn.flags.data(), in.R));
        in.reads.rd->state.flags_replaced(in.R != 0);   // plain columns: the flags travel beside the species array, the binning stands (the rule: reads_state.hpp)
        PTX_TRY(route_pack(run.ctx, in.bin_db.db, in.reads.rd, owner_all.data(), W, rt));
        for (int j = 0; j <= W; ++j) send_off[j] = rt.word_off[j] * 4;
        return 0;
    };
    const int local_rc = pack();
    // {failure flag, bytes, reads, steps} of every (source, owner) pair in one all-reduce
    std::vector<double> m(3 * (size_t)W * W + 1, 0.0);
    if (local_rc == 0)
        for (int j = 0; j < W; ++j) {
            m[(size_t)rk * W + j] = (double)(send_off[j + 1] - send_off[j]);
            m[(size_t)W * W + (size_t)rk * W + j] = (double)rt.n_reads[j];
            m[2 * (size_t)W * W + (size_t)rk * W + j] = (double)rt.n_steps[j];
        }
    m[3 * (size_t)W * W] = local_rc != 0 ? 1.0 : 0.0;
    PTX_TRY(run.comm.allreduce(m.data(), m.size()));
    if (m[3 * (size_t)W * W] != 0.0) return local_rc ? local_rc : run.comm.others_failed();
    std::vector<uint64_t> recv_off(W + 1, 0), nr_from(W), nt_from(W);
    for (int i = 0; i < W; ++i) {
        recv_off[i + 1] = recv_off[i] + (uint64_t)m[(size_t)i * W + rk];
        nr_from[i] = (uint64_t)m[(size_t)W * W + (size_t)i * W + rk];
        nt_from[i] = (uint64_t)m[2 * (size_t)W * W + (size_t)i * W + rk];
    }
    DevBuf<uint32_t> d_recv;
    PTX_HIP(run.ctx, d_recv.alloc(recv_off[W] / 4 + 1));
    PTX_TRY(run.comm.a2a_dev(rt.d_send.p, send_off.data(), d_recv.p, recv_off.data()));
    auto unpack = [&]() -> int {
        std::unique_ptr<pantax_hip_reads> routed(new pantax_hip_reads());
        PTX_TRY(reads_from_routed(run.ctx, d_recv.p, W, nr_from.data(), nt_from.data(), true, routed.get()));
        pantax_hip_reads_free(run.ctx, in.reads.rd);
        in.reads.rd = routed.release();
        return 0;
    };
    *unpack_rc = unpack();   // carried by the {failure flag, sums} all-reduce of the tables
    run.lap("route reads to owners");
    return 0;
}
// rows keep (species position in the selection, running number) so that any merge reproduces the one-process order
struct OutRow { double key; uint32_t k, seq; std::string line; };
bool write_part(const std::string &path, const std::vector<OutRow> &rows) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = true;
    for (const OutRow &r : rows) {
        const uint32_t len = (uint32_t)r.line.size();
        ok = ok && std::fwrite(&r.key, 8, 1, f) == 1 && std::fwrite(&r.k, 4, 1, f) == 1 && std::fwrite(&r.seq, 4, 1, f) == 1 && std::fwrite(&len, 4, 1, f) == 1 &&
             (len == 0 || std::fwrite(r.line.data(), 1, len, f) == len);
    }
    return std::fclose(f) == 0 && ok;
}
bool read_part(const std::string &path, std::vector<OutRow> &rows) {   // appends; the part is removed behind its last row
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    for (;;) {
        OutRow r; uint32_t len = 0;
        if (std::fread(&r.key, 8, 1, f) != 1) break;
        if (std::fread(&r.k, 4, 1, f) != 1 || std::fread(&r.seq, 4, 1, f) != 1 || std::fread(&len, 4, 1, f) != 1) { std::fclose(f); return false; }
        r.line.resize(len);
        if (len && std::fread(&r.line[0], 1, len, f) != len) { std::fclose(f); return false; }
        rows.push_back(std::move(r));
    }
    std::fclose(f);
    std::remove(path.c_str());
    return true;
}
// rows of the other ranks reach rank 0 through part files in the work directory (one node, one file system), behind an all-reduce as the barrier.
int gather_rows(Run &run, std::vector<OutRow> &ori_rows, std::vector<OutRow> &final_rows) {
    auto part_name = [&run](const char *what, int r) { return run.p.strain_file + "." + what + ".part" + std::to_string(r); };
    const bool wrote = write_part(part_name("ori", run.comm.rk), ori_rows) && write_part(part_name("final", run.comm.rk), final_rows);
    double bar[1] = {wrote ? 0.0 : 1.0};
    PTX_TRY(run.comm.allreduce(bar, 1));                      // every part is on disk (or somebody could not write)
    if (bar[0] != 0.0) return fail(run.ctx, PANTAX_HIP_E_IO, "profile: a rank could not write its part of the strain table under %s", run.p.wd.c_str());
    if (run.comm.rk != 0) return 0;
    ori_rows.clear(); final_rows.clear();
    for (int r = 0; r < run.comm.W; ++r)
        if (!read_part(part_name("ori", r), ori_rows) || !read_part(part_name("final", r), final_rows))
            return fail(run.ctx, PANTAX_HIP_E_IO, "profile: cannot read the part of rank %d under %s", r, run.p.wd.c_str());
    auto by_pos = [](const OutRow &a, const OutRow &b) { return a.k != b.k ? a.k < b.k : a.seq < b.seq; };
    std::sort(ori_rows.begin(), ori_rows.end(), by_pos);
    std::sort(final_rows.begin(), final_rows.end(), by_pos);
    return 0;
}
// ---- a15: abundance_est (profile.rs:3091-3289).  local_rc: this rank's status since the last collective (routing, shard); it travels in the one
// exchange of the strain level.  Collectives: {failure flag, the two normalisers} (all-reduce), [the barrier behind the part files (all-reduce)].
int strain_tables(Run &run, const Ingest &in, const Selection &sn, const ShardResult &sh, int local_rc, std::vector<GenomeRow> &genomes, std::vector<TrackRow> &track_rows) {
    const uint32_t Su = (uint32_t)sh.use.size();
    if (local_rc == 0) {
        const std::string err = read_genomes_info(path_join(run.p.db_dir, "genomes_info.txt"), genomes);   // the reference always reads <db>/genomes_info.txt (:3099)
        if (!err.empty()) local_rc = fail(run.ctx, PANTAX_HIP_E_IO, "%s", err.c_str());
    }
    std::unordered_multimap<std::string, size_t> by_hap;
    for (size_t i = 0; i < genomes.size(); ++i) by_hap.emplace(genomes[i].hap_id, i);
    std::vector<uint8_t> reported(Su, 0), pass(sh.hap_names.size() ? sh.hap_names.size() : 1, 0);
    double sum_all = 0.0, sum_pass = 0.0;
    if (local_rc == 0) {
        for (uint32_t k = 0; k < Su; ++k) {
            reported[k] = (sh.info[k].status1 == 0 && sh.info[k].status2 == 0) ? 1 : 0;
            // (a limit of the solver's tables -- none is tied to the number of candidate strains -- drops the species like a failed
            // solve in the reference, profile.rs:2999-3003: say so)
            if (sh.info[k].status1 == PANTAX_HIP_E_LIMIT || sh.info[k].status2 == PANTAX_HIP_E_LIMIT)
                std::fprintf(stderr, "[pantax_hip_profile] warning: species %s (%d candidate strains after the first filter) exceeds a table of this "
                                     "build's LP solver; it is left out of strain_abundance.txt\n",
                             in.ranges[sn.sel[sh.use[k]]].species.c_str(), sh.info[k].n_candidates);
        }
        if (Su) local_rc = pantax_hip_abundance_filter(Su, sh.hap_off.data(), sh.met.data(), reported.data(), run.cfg->single_cov_diff, run.cfg->min_cov, pass.data(), &sum_all, &sum_pass, nullptr, nullptr);
    }
    double ex[3] = {local_rc != 0 ? 1.0 : 0.0, sum_all, sum_pass};   // the one exchange of the strain level: did every rank get through, and the two normalisers
    PTX_TRY(run.comm.allreduce(ex, 3));
    if (ex[0] != 0.0) return local_rc ? local_rc : fail(run.ctx, PANTAX_HIP_E_STATE, "profile: another rank failed on its species; no strain table was written");
    sum_all = ex[1]; sum_pass = ex[2];
    const char *header = "species_taxid\tstrain_taxid\tgenome_ID\tpredicted_coverage\tpredicted_abundance\tpath_base_cov\tunique_trio_fraction\tuniq_trio_cov_mean\tfirst_sol\tstrain_cov_diff\ttotal_cov_diff\n";
    std::vector<OutRow> ori_rows, final_rows;
    for (uint32_t k = 0; k < Su; ++k) {
        if (!reported[k]) continue;
        const std::string &species = in.ranges[sn.sel[sh.use[k]]].species;
        uint32_t seq = 0;
        for (uint64_t h = sh.hap_off[k]; h < sh.hap_off[k + 1]; ++h) {
            auto range = by_hap.equal_range(sh.hap_names[h]);
            std::vector<const GenomeRow *> grs;
            for (auto it = range.first; it != range.second; ++it) grs.push_back(&genomes[it->second]);
            if (grs.empty()) grs.push_back(nullptr);          // left join keeps the row with null metadata
            const pantax_hip_hap_metrics &m = sh.met[h];
            const bool hs = m.has & PANTAX_HIP_HAS_SECOND;
            for (const GenomeRow *gr : grs) {
                ori_rows.push_back({0.0, sh.use[k], seq, strain_row_text(species, gr, m, hs ? m.second_sol / sum_all : 0.0, hs, false)});
                if (pass[h]) final_rows.push_back({m.second_sol / sum_pass, sh.use[k], seq, strain_row_text(species, gr, m, m.second_sol / sum_pass, true, !run.cfg->full)});   // :3250-3284
                if (pass[h] && run.p.rep.rows_run()) track_rows.push_back({m.second_sol / sum_pass, k, h, gr});   // (one rank: already in the order of final_rows)
                ++seq;
            }
        }
    }
    if (run.comm.use_comm) {
        PTX_TRY(gather_rows(run, ori_rows, final_rows));
        if (run.comm.rk != 0) { run.lap("tables"); return 0; }
    }
    {
        std::ofstream ori("ori_strain_abundance.txt");   // written to the current directory (profile.rs:3217)
        if (ori) { ori << header; for (auto &r : ori_rows) ori << r.line << '\n'; }
    }
    std::stable_sort(final_rows.begin(), final_rows.end(), [](const OutRow &a, const OutRow &b) { return a.key > b.key; });   // :3247-3248
    std::ofstream f(run.p.strain_file);
    if (!f) return fail(run.ctx, PANTAX_HIP_E_IO, "cannot write %s", run.p.strain_file.c_str());
    f << header;
    for (auto &r : final_rows) f << r.line << '\n';
    run.lap("tables");
    return 0;
}
// The phases in order.  `rc` is this rank's status since the last collective (RankComm's rule): PTX_TRY where a phase has ended in the collective
// that carried it, an assignment where the next collective carries it.
int profile_impl(pantax_hip_ctx *ctx, const pantax_hip_profiling_config *cfg, const pantax_hip_profile_ext *ext) {
    PTX_ENTER(ctx);
    Run run{ctx, cfg, ext, RunPlan(), RankComm{ctx, cfg}, Lap()};
    const RunPlan &p = run.p;
    PTX_TRY(check_args(run));
    PTX_TRY(decide_resume(run));                                                             // all-reduce: rank 0's decision
    if (!p.full_path && !p.strain_only) { rs_skipped(p); return 0; }                         // profile.rs:3419-3427: outputs already present
    mkdir(p.out_dir.c_str(), 0777);
    run.lap = Lap{ctx->cfg.trace, run.comm.rk};

    // ---- what depends on the sample
    Ingest in(ctx);
    PTX_TRY(ingest(run, in));                                                                // all-reduce(s): status [+ counters]
    std::vector<SpeciesProfileRow> sp_profile;   // species_taxid, predicted_abundance, predicted_coverage
    int rc = p.full_path ? species_from_counters(run, in, sp_profile) : species_from_files(run, in, sp_profile);
    PTX_TRY(run.comm.agree(rc));                                                             // also the barrier behind the report parts
    rc = join_report_parts(run);
    if (p.full_path && (!cfg->strain || p.strain_done)) { rs_skipped(p); return run.comm.agree(rc); }
    run.lap("species table / report");
    Selection sn;
    if (!select_species(cfg, in, sp_profile, sn)) { rs_skipped(p); return run.comm.agree(rc); }   // reference: warn + exit(0) (profile.rs:595-598); the same decision on every rank
    PTX_TRY(duplicate_ids(run, in, sn, rc));                                                 // agree(rc), then the id exchange when sharded
    run.lap("select + duplicate ids");
    // which rank takes which selected species: longest-processing-time packing on (reads binned to the species + its graph nodes)
    std::vector<double> weight(sn.sel.size());
    for (size_t i = 0; i < weight.size(); ++i) weight[i] = (double)in.rc[sn.sel[i]] * 8.0 + (double)(in.ranges[sn.sel[i]].end - in.ranges[sn.sel[i]].start + 1);   // ~8 walk steps per read
    sn.owner = lpt_owner(weight, run.comm.W);
    rc = 0;
    if (p.sharded) PTX_TRY(route_reads(run, in, sn, &rc));                                   // all-reduce + alltoallv; rc: the unpacking

    // ---- what depends on the DB: this rank's species through the device; a failure travels in the exchange of the tables
    ShardResult sh;
    if (rc == 0) sh = run_shard(run, in, sn, /*use_images=*/true);
    if (sh.rc && sh.image_fault) {
        // said once per run, trace or not: the image stays where it is (image_cache 1 writes none), and every run pays this detour until it is removed
        std::fprintf(stderr, "pantax-hip: warning: a graph image among [%s] failed its load-time checks (%s); the graph files are loaded instead. "
                             "Remove the damaged image, or run once with image_cache 2 to write it afresh.\n", sh.fault_images.c_str(), pantax_hip_last_error(ctx));
        sh = run_shard(run, in, sn, /*use_images=*/false);
    }
    std::vector<GenomeRow> genomes;
    std::vector<TrackRow> track_rows;
    PTX_TRY(strain_tables(run, in, sn, sh, rc ? rc : sh.rc, genomes, track_rows));           // all-reduce: status + normalisers [+ barrier]
    return reports::write(run, in, sn, sh, genomes, track_rows);                              // the files of the per-strain reports
}

}  // namespace

// nothing throws across the boundary: an allocation failure or a parser exception becomes a status + message
extern "C" int pantax_hip_profile_with_ext(pantax_hip_ctx *ctx, const pantax_hip_profiling_config *cfg, const pantax_hip_profile_ext *ext) {
    if (!ctx || !cfg) return PANTAX_HIP_E_INVALID;
    try {
        return profile_impl(ctx, cfg, ext);
    } catch (const std::bad_alloc &) {
        return fail(ctx, PANTAX_HIP_E_LIMIT, "profile: out of host memory");
    } catch (const std::exception &e) {
        return fail(ctx, PANTAX_HIP_E_STATE, "profile: %s", e.what());
    } catch (...) {
        return fail(ctx, PANTAX_HIP_E_STATE, "profile: unknown exception");
    }
}
extern "C" int pantax_hip_profile(pantax_hip_ctx *ctx, const pantax_hip_profiling_config *cfg) { return pantax_hip_profile_with_ext(ctx, cfg, nullptr); }
