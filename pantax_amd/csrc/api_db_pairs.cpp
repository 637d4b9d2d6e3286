// api_db_pairs.cpp -- the --db-pairs mode: pantax_hip_db_pairs(cfg), pairwise strain distinguishability of a db as one table (include/pantax_hip.h,
// DESIGN.md "Pairwise strain distinguishability").  Files in (species_range.txt, the species' graphs, genomes_info.txt), one TSV out; no GAF, no work
// directory, no strain step.  Host orchestration only: the sums come from pantax_hip_db_hap_pairs, one call per group of species.
#include <algorithm>
#include <fstream>
#include <set>
#include <sstream>
#include <unordered_map>
#include "hap_pairs_plan.hpp"
#include "profile_run.hpp"

using namespace ptx;

namespace {

std::string opt(const char *s) { return s ? std::string(s) : std::string(); }
bool is_dir(const std::string &p) { struct stat st; return !p.empty() && stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }

struct PairsSpecies { std::string taxid; int64_t start, end; uint64_t n_haps = 0; bool skipped = false; uint64_t sp[6] = {0, 0, 0, 0, 0, 0}; uint64_t min_dist = ~0ull; bool has_dist = false; };

// the graph of one species by the file seam's choice of container (profile_shard.cpp source_of): <otu>.bin / .bin.lz4 / .bin.zst per zip, else GFA text
std::string load_graph(const std::string &db_dir, const std::string &zip, const std::string &otu, HostGraph &g) {
    const std::string bin = path_join(path_join(db_dir, "species_graph_info"), otu + ".bin");
    if (zip == "serialize" && is_file(bin)) return read_graph_bin(bin, g);
    if (zip == "lz" && is_file(bin + ".lz4")) return read_graph_zip(bin + ".lz4", 2, g);
    if (zip == "zstd" && is_file(bin + ".zst")) return read_graph_zip(bin + ".zst", 3, g);
    const std::string gfa = path_join(path_join(db_dir, "species_gfa"), otu + ".gfa");
    if (!is_file(gfa)) return "gfa information file " + gfa + " does not exist. Please check database.";
    return read_gfa(gfa, g);
}

// one group of species resident: upload, every haplotype selected, one call, the group's pair rows -> `out`, its species sums -> sp
int run_group(pantax_hip_ctx *ctx, const pantax_hip_db_pairs_config *cfg, std::vector<PairsSpecies> &sp, const std::vector<uint32_t> &members, const std::vector<HostGraph> &graphs,
              const std::unordered_map<std::string, std::string> &genome_of, std::ostream &out) {
    const uint32_t Sg = (uint32_t)members.size();
    if (!Sg) return 0;
    std::vector<int64_t> rs(Sg), re(Sg);
    std::vector<pantax_hip_graph_part> parts(Sg);
    std::vector<uint64_t> sel_off(Sg + 1, 0), pair_off(Sg + 1, 0);
    std::vector<uint32_t> sel_hap;
    for (uint32_t k = 0; k < Sg; ++k) {
        const HostGraph &g = graphs[k];
        rs[k] = sp[members[k]].start; re[k] = sp[members[k]].end;
        parts[k] = pantax_hip_graph_part{g.node_len.size(), g.hap_names.size(), g.node_len.data(), g.path_off.data(), g.path_nodes.data()};
        for (uint32_t h = 0; h < g.hap_names.size(); ++h) sel_hap.push_back(h);
        sel_off[k + 1] = sel_hap.size();
    }
    DbHolder db{ctx};
    PTX_TRY(pantax_hip_db_upload_parts(ctx, Sg, rs.data(), re.data(), parts.data(), &db.db));
    const pantax_hip_evidence_set set{Sg, sel_off.data(), sel_hap.data()};
    const int rc_size = pantax_hip_db_hap_pairs(ctx, db.db, &set, pair_off.data(), 0, nullptr, nullptr);   // sizes: E_LIMIT unless there is no entry
    if (rc_size != 0 && rc_size != PANTAX_HIP_E_LIMIT) return rc_size;
    std::vector<uint64_t> pair(pair_off[Sg] * 2 ? pair_off[Sg] * 2 : 1), sums((size_t)Sg * 6);
    PTX_TRY(pantax_hip_db_hap_pairs(ctx, db.db, &set, pair_off.data(), pair_off[Sg], pair.data(), sums.data()));
    for (uint32_t k = 0; k < Sg; ++k) {
        PairsSpecies &s = sp[members[k]];
        const HostGraph &g = graphs[k];
        const uint64_t K = g.hap_names.size();
        std::copy(sums.begin() + 6 * k, sums.begin() + 6 * k + 6, s.sp);
        const uint64_t *P = pair.data() + pair_off[k] * 2;
        const auto name = [&](uint64_t h) -> const std::string & { const auto it = genome_of.find(g.hap_names[h]); return it != genome_of.end() ? it->second : g.hap_names[h]; };
        for (uint64_t a = 0; a < K; ++a)
            for (uint64_t b = a + 1; b < K; ++b) {
                const uint64_t *aa = P + (a * K + a) * 2, *bb = P + (b * K + b) * 2, *ab = P + (a * K + b) * 2;
                const uint64_t only_a = aa[1] - ab[1], only_b = bb[1] - ab[1], dist = only_a + only_b, uni = aa[1] + bb[1] - ab[1];
                s.min_dist = std::min(s.min_dist, dist); s.has_dist = true;
                if (cfg->max_distance >= 0 && dist > (uint64_t)cfg->max_distance) continue;
                out << s.taxid << '\t' << name(a) << '\t' << name(b) << '\t' << hap_pair_class(only_a, only_b) << '\t' << aa[0] << '\t' << aa[1] << '\t' << bb[0] << '\t' << bb[1] << '\t'
                    << ab[0] << '\t' << ab[1] << '\t' << only_a << '\t' << only_b << '\t' << dist << '\t' << (uni ? fmt_f64((double)ab[1] / (double)uni) : std::string("-")) << '\n';
            }
    }
    return 0;
}

int db_pairs_impl(pantax_hip_ctx *ctx, const pantax_hip_db_pairs_config *cfg) {
    const std::string db_dir = opt(cfg->db), out_path = opt(cfg->out_file), zip = opt(cfg->zip);
    if (!is_dir(db_dir)) return fail(ctx, PANTAX_HIP_E_IO, "Specified PanTax database directory '%s' is not a valid directory path", db_dir.c_str());
    if (out_path.empty()) return fail(ctx, PANTAX_HIP_E_INVALID, "db_pairs: no output file");
    if (zip == "h5") return fail(ctx, PANTAX_HIP_E_LIMIT, "db_pairs: graph container '%s' is not available in this build; use serialize / lz / zstd or GFA", zip.c_str());
    const std::string range_path = is_file(opt(cfg->range_file)) ? opt(cfg->range_file) : path_join(db_dir, "species_range.txt");
    if (!is_file(range_path)) return fail(ctx, PANTAX_HIP_E_IO, "Neither species range file '%s' nor '%s' is a valid file path", opt(cfg->range_file).c_str(), range_path.c_str());
    std::vector<RangeRow> ranges;
    std::string err = read_species_range(range_path, ranges);
    if (!err.empty()) return fail(ctx, PANTAX_HIP_E_IO, "%s", err.c_str());
    // the named species, each once, in range-file order; an unknown taxid is refused before anything is loaded
    std::set<std::string> named;
    {
        std::stringstream ss(opt(cfg->species));
        for (std::string t; std::getline(ss, t, ',');) if (!t.empty()) named.insert(t);
        for (const std::string &t : named)
            if (std::none_of(ranges.begin(), ranges.end(), [&](const RangeRow &r) { return r.species == t; }))
                return fail(ctx, PANTAX_HIP_E_INVALID, "db_pairs: species %s is not in %s", t.c_str(), range_path.c_str());
    }
    // genome_ID of a haplotype: its first row of <db>/genomes_info.txt, as in the strain table; without one (or without the file) the haplotype's own name
    std::unordered_map<std::string, std::string> genome_of;
    if (is_file(path_join(db_dir, "genomes_info.txt"))) {
        std::vector<GenomeRow> genomes;
        err = read_genomes_info(path_join(db_dir, "genomes_info.txt"), genomes);
        if (!err.empty()) return fail(ctx, PANTAX_HIP_E_IO, "%s", err.c_str());
        for (size_t i = genomes.size(); i-- > 0;) genome_of[genomes[i].hap_id] = genomes[i].genome_id;
    }
    const uint64_t steps_max = ctx->cfg.db_path_steps_max ? ctx->cfg.db_path_steps_max : 3000000000ull;   // the hard limits of the file seam's groups (cut_groups)
    std::vector<PairsSpecies> sp;
    std::ostringstream rows;
    std::vector<uint32_t> members;
    std::vector<HostGraph> graphs;
    uint64_t steps = 0, nodes = 0;
    for (const RangeRow &r : ranges) {
        if (!named.empty() && !named.count(r.species)) continue;
        HostGraph g;
        err = load_graph(db_dir, zip, r.species, g);
        if (!err.empty()) return fail(ctx, PANTAX_HIP_E_IO, "%s", err.c_str());
        if ((int64_t)g.node_len.size() != r.end - r.start + 1)
            return fail(ctx, PANTAX_HIP_E_IO, "species %s: graph has %llu nodes but its range spans %lld", r.species.c_str(), (unsigned long long)g.node_len.size(), (long long)(r.end - r.start + 1));
        if (named.empty() && g.hap_names.size() < 2) continue;   // by default: the species that have a pair
        PairsSpecies s;
        s.taxid = r.species; s.start = r.start; s.end = r.end; s.n_haps = g.hap_names.size();
        if (s.n_haps > HAP_PAIRS_MAX_K) {
            s.skipped = true;
            std::fprintf(stderr, "[pantax_hip_db_pairs] species %s has %llu haplotypes, more than the %llu the pair sums serve: skipped\n", r.species.c_str(), (unsigned long long)s.n_haps,
                         (unsigned long long)HAP_PAIRS_MAX_K);
            sp.push_back(s);
            continue;
        }
        const uint64_t ps = g.path_nodes.size(), nn = g.node_len.size();
        if (!members.empty() && (steps + ps > steps_max || nodes + nn > 0xF0000000ull)) {
            PTX_TRY(run_group(ctx, cfg, sp, members, graphs, genome_of, rows));
            members.clear(); graphs.clear(); steps = nodes = 0;
        }
        members.push_back((uint32_t)sp.size());
        sp.push_back(s);
        graphs.push_back(std::move(g));
        steps += ps; nodes += nn;
    }
    PTX_TRY(run_group(ctx, cfg, sp, members, graphs, genome_of, rows));
    std::ofstream f(out_path);
    if (!f) return fail(ctx, PANTAX_HIP_E_IO, "cannot write %s", out_path.c_str());
    f << "species_taxid\tgenome_ID_a\tgenome_ID_b\tclass\tn_nodes_a\tlen_a\tn_nodes_b\tlen_b\tshared_nodes\tshared_len\tonly_a_len\tonly_b_len\tdistance\tjaccard\n" << rows.str();
    for (const PairsSpecies &s : sp) {
        f << s.taxid << '\t' << s.n_haps << "\t-\t";
        if (s.skipped) f << "skipped\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
        else {
            f << "species\t" << s.sp[0] << '\t' << s.sp[1] << "\t-\t-\t" << s.sp[4] << '\t' << s.sp[5] << "\t-\t-\t";
            if (s.has_dist) f << s.min_dist; else f << '-';
            f << "\t-\n";
        }
    }
    f.close();
    if (!f) return fail(ctx, PANTAX_HIP_E_IO, "cannot write %s", out_path.c_str());
    return 0;
}

}  // namespace

extern "C" int pantax_hip_db_pairs(pantax_hip_ctx *ctx, const pantax_hip_db_pairs_config *cfg) {
    if (!ctx) return PANTAX_HIP_E_INVALID;
    if (!cfg) return fail(ctx, PANTAX_HIP_E_INVALID, "db_pairs: null argument");
    PTX_ENTER(ctx);
    try {   // nothing throws across the boundary (allocation failures of a large graph included)
        return db_pairs_impl(ctx, cfg);
    } catch (const std::exception &ex) {
        return fail(ctx, PANTAX_HIP_E_IO, "db_pairs: %s", ex.what());
    }
}
