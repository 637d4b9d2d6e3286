// profile_shard.cpp -- run_shard (profile_run.hpp): a6 - a14 of the file seam for this rank's selected species.  Where every graph comes from
// (headers only), the cut into groups, the loader thread, the device sequence per group with the per-strain reports' turn behind the strain step
// (reports::collect_group, profile_reports.cpp), image write-back.
#include <algorithm>
#include <chrono>
#include <memory>
#include <thread>
#include "db_image.hpp"
#include "profile_run.hpp"

namespace ptx {
namespace {

// optimize_otu's file choice (profile.rs:2888-2932): container 1 <otu>.bin, 2 .bin.lz4, 3 .bin.zst (read_graph_zip's codec), 0 GFA text (which may be missing)
std::pair<int, std::string> source_of(const RunPlan &p, const std::string &otu) {
    const std::string bin = path_join(path_join(p.db_dir, "species_graph_info"), otu + ".bin");
    if (p.zip == "serialize" && is_file(bin)) return {1, bin};
    if (p.zip == "lz" && is_file(bin + ".lz4")) return {2, bin + ".lz4"};
    if (p.zip == "zstd" && is_file(bin + ".zst")) return {3, bin + ".zst"};
    return {0, path_join(path_join(p.db_dir, "species_gfa"), otu + ".gfa")};
}
std::string image_of(const RunPlan &p, const std::string &otu) { return path_join(path_join(p.db_dir, "species_graph_info"), otu + ".hipdb"); }

struct Source { int kind = 0; /* 0 none, 1 image, 2 streamed .bin, 3 host graph */ SpeciesImage img; BinIndex bin; std::string bin_path; std::vector<uint64_t> path_off; };
struct Group { uint32_t k0, k1; std::vector<GraphPart> gparts; };

// Where every selected species' graph comes from, decided species by species on a few dozen threads that read HEADERS only: image_cache >= 1 and a device-ready
// image <otu>.hipdb not older than its source (db_image.cpp): the arrays stream from the image; zip "serialize" and <otu>.bin: they stream from the
// bincode file itself, 64-bit values narrowed on their way into the pinned ring; "lz" / "zstd" containers and GFA text: decoded / parsed into host memory first.
int choose_sources(Run &run, const Ingest &in, const Selection &sn, bool use_images, std::vector<Source> &src, std::vector<HostGraph> &graphs, std::vector<uint8_t> &loaded) {
    const uint32_t Ss = (uint32_t)sn.sel.size();
    std::vector<std::string> hard(Ss);   // errors that end the run; the first one in species order is reported
    const int n_thr = (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency() / (unsigned)std::max(1, run.comm.W)));
    parallel_for(Ss, n_thr, [&](uint64_t i0, uint64_t i1) {
        for (uint64_t i = i0; i < i1; ++i) {
            if (sn.owner[i] != run.comm.rk) { loaded[i] = 0; continue; }                                 // another rank's species
            const std::string &otu = in.ranges[sn.sel[i]].species;
            const int64_t nvert = in.ranges[sn.sel[i]].end - in.ranges[sn.sel[i]].start + 1;
            Source &sc = src[i];
            if (run.cfg->image_cache >= 1 && use_images) {
                const std::string img = image_of(run.p, otu);
                if (is_file(img) && file_mtime(img) >= file_mtime(source_of(run.p, otu).second) && sc.img.open(img).empty() && (int64_t)sc.img.V == nvert) { sc.kind = 1; continue; }
            }
            const auto [container, gpath] = source_of(run.p, otu);
            std::string e2;
            uint64_t n_nodes = 0;
            if (container == 1) {
                e2 = scan_graph_bin(gpath, sc.bin);
                if (e2.empty() && sc.bin.names_ascending) {
                    sc.kind = 2; sc.bin_path = gpath; n_nodes = sc.bin.V;
                    sc.path_off.assign(sc.bin.walk_len.size() + 1, 0);
                    for (size_t h = 0; h < sc.bin.walk_len.size(); ++h) sc.path_off[h + 1] = sc.path_off[h] + sc.bin.walk_len[h];
                } else if (e2.empty()) { e2 = read_graph_bin(gpath, graphs[i]); sc.kind = 3; n_nodes = graphs[i].node_len.size(); }   // keys out of order: the general parser sorts them
            } else if (container) { e2 = read_graph_zip(gpath, container, graphs[i]); sc.kind = 3; n_nodes = graphs[i].node_len.size(); }
            else if (is_file(gpath)) { e2 = read_gfa(gpath, graphs[i]); sc.kind = 3; n_nodes = graphs[i].node_len.size(); }
            else { hard[i] = "gfa information file " + gpath + " does not exist. Please check database."; continue; }
            if (!e2.empty()) { loaded[i] = 0; sc.kind = 0; continue; }            // "GFA read error" => species skipped (.ok()?)
            if ((int64_t)n_nodes != nvert)
                hard[i] = "species " + otu + ": graph has " + std::to_string(n_nodes) + " nodes but its range spans " + std::to_string((long long)nvert);
        }
    });
    for (uint32_t i = 0; i < Ss; ++i) if (!hard[i].empty()) return fail(run.ctx, PANTAX_HIP_E_IO, "%s", hard[i].c_str());
    return 0;
}
// the groups of cut_groups with their parts; the file indices of a group's segments are relative to the group's file list
std::vector<Group> make_groups(const pantax_hip_ctx *ctx, const std::vector<GraphPart> &parts) {
    std::vector<uint64_t> steps(parts.size()), nodes(parts.size());
    for (size_t k = 0; k < parts.size(); ++k) { steps[k] = parts[k].path_off[parts[k].n_haps] - parts[k].path_off[0]; nodes[k] = parts[k].n_nodes; }
    std::vector<Group> groups;
    for (const auto &cut : cut_groups(steps, nodes, ctx->cfg.db_path_steps_max ? ctx->cfg.db_path_steps_max : 3000000000ull, ctx->cfg.db_groups)) {
        const uint32_t k0 = cut.first;
        Group g{k0, cut.second, std::vector<GraphPart>(parts.begin() + k0, parts.begin() + cut.second)};
        if (k0)
            for (GraphPart &pt : g.gparts) {
                if (pt.len_seg.file >= 0) pt.len_seg.file -= (int32_t)k0;
                for (UploadSeg &w : pt.walk_segs) if (w.file >= 0) w.file -= (int32_t)k0;
                for (UploadSeg *w : {&pt.pk.first_seg, &pt.pk.off_seg, &pt.pk.payload_seg}) if (w->file >= 0) w->file -= (int32_t)k0;
            }
        groups.push_back(std::move(g));
    }
    return groups;
}
// the loader: ONE group in flight.  begin() on the calling thread (small uploads through the ctx's staging), the arrays on the loader thread.
struct Loader {
    std::thread th;
    DbHolder db;
    int rc = 0; std::string err; double ms = 0;
    explicit Loader(pantax_hip_ctx *c) : db{c} {}
    void join() { if (th.joinable()) th.join(); }
    ~Loader() { join(); }
};
int start_load(pantax_hip_ctx *ctx, const int64_t *g_rs, const int64_t *g_re, const std::string *files, const Group &g, bool piped, Loader &L) {
    PTX_TRY(db_upload_begin(ctx, g.k1 - g.k0, g_rs + g.k0, g_re + g.k0, g.gparts.data(), &L.db.db));
    const GraphPart *gp = g.gparts.data();
    const std::string *gf = files + g.k0;
    pantax_hip_db *dbp = L.db.db;
    if (!piped) {
        const auto t0 = std::chrono::steady_clock::now();
        L.rc = db_upload_arrays(ctx, dbp, gp, gf, nullptr);
        L.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return L.rc;
    }
    L.th = std::thread([this_ctx = ctx, dbp, gp, gf, &L] {
        const auto t0 = std::chrono::steady_clock::now();
        if (hipSetDevice(this_ctx->device) != hipSuccess) L.rc = fail(this_ctx, PANTAX_HIP_E_HIP, "hipSetDevice on the graph loader thread");
        else L.rc = db_upload_arrays(this_ctx, dbp, gp, gf, this_ctx->stream_up);
        if (L.rc) L.err = pantax_hip_last_error(this_ctx);     // this thread's message: handed to the thread that reports
        L.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    });
    return 0;
}
// one pass: sources, parts, groups; per group the loader hand-over, then binning against the selected ranges, index, coverage, strain step
int shard_pass(Run &run, Ingest &in, const Selection &sn, bool use_images, ShardResult &sh) {
    const uint32_t Ss = (uint32_t)sn.sel.size();
    std::vector<HostGraph> graphs(Ss);
    std::vector<uint8_t> loaded(Ss, 1);
    std::vector<Source> src(Ss);
    PTX_TRY(choose_sources(run, in, sn, use_images, src, graphs, loaded));
    run.lap("graph headers");
    for (uint32_t i = 0; i < Ss; ++i) if (loaded[i] && sn.owner[i] == run.comm.rk) sh.use.push_back(i);
    const uint32_t Su = (uint32_t)sh.use.size();
    sh.info.assign(Su, pantax_hip_solve_info{});
    sh.hap_off.assign(Su + 1, 0);
    // one part per used species (where its two arrays lie), its range, its file, its coverage; the haplotype names of the shard in species order
    std::vector<int64_t> g_rs(Su), g_re(Su); std::vector<double> cov(Su);
    std::vector<GraphPart> parts(Su); std::vector<std::string> files(Su);
    for (uint32_t k = 0; k < Su; ++k) {
        const uint32_t i = sh.use[k];
        g_rs[k] = in.ranges[sn.sel[i]].start; g_re[k] = in.ranges[sn.sel[i]].end; cov[k] = sn.sel_cov[i];
        const Source &sc = src[i];
        GraphPart &pt = parts[k];
        const std::vector<std::string> *names = nullptr;
        if (sc.kind == 1) {
            files[k] = sc.img.path; names = &sc.img.hap_names;
            sc.img.fill_part(pt, (int32_t)k);
        } else if (sc.kind == 2) {
            files[k] = sc.bin_path; names = &sc.bin.hap_names;
            pt.n_nodes = sc.bin.V; pt.n_haps = sc.bin.hap_names.size(); pt.path_off = sc.path_off.data();
            pt.len_seg.file = (int32_t)k; pt.len_seg.file_off = sc.bin.off_node_len; pt.len_seg.out_bytes = 4 * sc.bin.V; pt.len_seg.narrow = true;
            for (size_t h = 0; h < sc.bin.walk_len.size(); ++h) {
                UploadSeg w; w.file = (int32_t)k; w.file_off = sc.bin.walk_off[h]; w.out_bytes = 4 * sc.bin.walk_len[h]; w.narrow = true;
                pt.walk_segs.push_back(w);
            }
        } else {
            const HostGraph &hg = graphs[i];
            names = &hg.hap_names;
            pt.n_nodes = hg.node_len.size(); pt.n_haps = hg.hap_names.size(); pt.path_off = hg.path_off.data();
            pt.len_seg.src = hg.node_len.data(); pt.len_seg.out_bytes = 4 * hg.node_len.size(); pt.len_seg.narrow = true;
            UploadSeg w; w.src = hg.path_nodes.data(); w.out_bytes = 4 * hg.path_nodes.size();
            pt.walk_segs.push_back(w);
        }
        sh.hap_names.insert(sh.hap_names.end(), names->begin(), names->end());
        sh.hap_off[k + 1] = sh.hap_names.size();
    }
    sh.met.resize(sh.hap_names.size());
    reports::begin(run.p.rep, Su, sh.hap_names.size(), in.R, sh.rep);
    if (!Su) return 0;
    const std::vector<Group> groups = make_groups(run.ctx, parts);
    const bool piped = groups.size() > 1;
    if (piped && !run.ctx->stream_up) PTX_HIP(run.ctx, hipStreamCreateWithFlags(&run.ctx->stream_up, hipStreamNonBlocking));
    bool flags_set = false;
    std::unique_ptr<Loader> cur(new Loader(run.ctx)), next;
    PTX_TRY(start_load(run.ctx, g_rs.data(), g_re.data(), files.data(), groups[0], piped, *cur));
    if (!in.reads.rd->state.grouped()) { PTX_TRY(reads_group(run.ctx, in.reads.rd)); run.lap("locus-grouped copy of the reads"); }   // built once, beside the first graph load (sharded: reads_from_routed grouped what arrived)
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const uint32_t k0 = groups[gi].k0, k1 = groups[gi].k1, Sg = k1 - k0;
        cur->join();
        if (cur->rc) return piped ? fail(run.ctx, cur->rc, "%s", cur->err.c_str()) : cur->rc;
        if (run.ctx->cfg.trace) std::fprintf(stderr, "[db_upload]            %-28s %9.3f ms%s\n", "graph arrays -> HBM", cur->ms, piped ? " (loader thread, beside the group before)" : "");
        if (gi + 1 < groups.size()) { next.reset(new Loader(run.ctx)); PTX_TRY(start_load(run.ctx, g_rs.data(), g_re.data(), files.data(), groups[gi + 1], piped, *next)); }
        pantax_hip_db *const db = cur->db.db;
        // An image is a cache: one whose header passes but whose arrays fail the load-time checks on the device (a damaged block offset, a walk that
        // leaves its graph) must end where a truncated one ends, in the graph files: the caller runs the shard again without images.
        // (the load-time refusals alone -- a node of length 0, a walk outside its graph, both E_INVALID from the checks on the device: a HIP error, a
        // limit or a failed allocation is reported as it is, never followed by a second pass over the same device)
        if (const int rc_fin = db_upload_finish(run.ctx, db)) {
            bool has_image = false;
            for (const GraphPart &pt : groups[gi].gparts) has_image = has_image || pt.packed;
            sh.image_fault = has_image && rc_fin == PANTAX_HIP_E_INVALID;
            uint32_t n_named = 0;
            for (uint32_t k = k0; k < k1 && sh.image_fault; ++k)
                if (src[sh.use[k]].kind == 1 && ++n_named <= 8) sh.fault_images += (sh.fault_images.empty() ? "" : ", ") + src[sh.use[k]].img.path;
            if (n_named > 8) sh.fault_images += ", ... (" + std::to_string(n_named) + " images in the group)";
            return rc_fin;
        }
        run.lap(Sg == Su ? "db upload" : "db upload (a group of the species)");
        // the same resident reads with the strain-level drop flags, binned against the selected ranges: reads of unselected species fall outside every range => "U" =>
        // skipped (profile.rs:3301-3303); strain only: species from the saved report decide membership -- rows it calls "U" carry a drop flag, see a5
        if (!run.p.sharded && sn.flags_dirty && !flags_set) { PTX_TRY(pantax_hip_reads_set_flags(run.ctx, in.reads.rd, sn.flags.data())); flags_set = true; }   // sharded: flagged rows were not routed; else the tokenizer's flags stand
        PTX_TRY(pantax_hip_bin_reads(run.ctx, db, in.reads.rd, nullptr, nullptr, nullptr, nullptr, nullptr));
        run.lap("  flags + bin selected");
        uint64_t nU = 0, n_abort = 0;
        PTX_TRY(pantax_hip_trio_index(run.ctx, db, &nU));
        run.lap("  trio index");
        PTX_TRY(pantax_hip_node_coverage(run.ctx, db, in.reads.rd, nullptr, nullptr, nullptr, nullptr, &n_abort));
        run.lap("  node coverage");
        // --sample_test: 500 rows whatever --sample says (profile.rs:1387-1393)
        pantax_hip_strain_config sc{run.cfg->unique_trio_nodes_fraction, run.cfg->unique_trio_nodes_mean_count_f, run.cfg->single_cov_ratio, run.cfg->min_depth, run.cfg->shift,
                                    run.cfg->sample_test ? 500 : run.cfg->sample_nodes, run.cfg->solver_semantics};
        PTX_TRY(pantax_hip_strain_profile(run.ctx, db, &sc, nullptr, cov.data() + k0, sh.met.data() + sh.hap_off[k0], sh.info.data() + k0));
        run.lap("strain step");
        PTX_TRY(reports::collect_group(run, in, sn, db, k0, k1, sh));   // the per-strain reports take what they need while the group is resident
        if (run.cfg->image_cache == 2) {   // leave images behind for the next run
            for (uint32_t k = k0; k < k1; ++k)
                if (src[sh.use[k]].kind != 1) {
                    const std::vector<std::string> names(sh.hap_names.begin() + (ptrdiff_t)sh.hap_off[k], sh.hap_names.begin() + (ptrdiff_t)sh.hap_off[k + 1]);
                    PTX_TRY(db_save_image(run.ctx, db, k - k0, names, image_of(run.p, in.ranges[sn.sel[sh.use[k]]].species)));
                }
            run.lap("graph images written");
        }
        cur = std::move(next);
    }
    return 0;
}

}  // namespace
ShardResult run_shard(Run &run, Ingest &in, const Selection &sn, bool use_images) { ShardResult sh; sh.rc = shard_pass(run, in, sn, use_images, sh); return sh; }
}  // namespace ptx
