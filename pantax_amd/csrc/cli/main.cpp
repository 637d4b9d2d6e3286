// pantax-hip -- command-line front end of the pipeline seam.  Takes the profiling flags of the
// reference CLI (cli.rs:114-164, 222-240; defaults resolved as in main.rs:102-171) and calls
// pantax_hip_profile_with_ext, i.e. it stands where `pantax ... --species --strain` calls profile::profile.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../../include/pantax_hip.h"
#include "rccl_comm.hpp"

static void usage() {
    fprintf(stderr,
            "usage: pantax-hip -db <db_dir> --gaf <gfa_mapped.gaf> [-T <work_dir>] [--species] [--strain]\n"
            "       pantax-hip -db <db_dir> --db-pairs <out.tsv> [--db-pairs-species a,b] [--db-pairs-max-distance N] [--gfa | --zip ...] [--range-file F] [--device N]\n"
            "  --short-read | --long-read     (sets --fr default 0.3 / 0.5)\n"
            "  --fr F  --fc F(0.46)  -a F(1e-4)  --sr F(0.85)  --sd F(0.2)  --shift true|false\n"
            "  --min_cov N  --min_depth N  --sample N (default 500000)  --sample_test  --ds a,b,c  --smode 0|1  --no-filter\n"
            "  --solver gurobi|highs|cplex|cbc|glpk   whose second-solve semantics to reproduce (the LP optimum is the same; default gurobi)\n"
            "  --force  -R <reads_classification.tsv>  --range-file F  --species-len-file F  --reads-binning-file F\n"
            "  --read-strains F   per-read strain report: one row per GAF record (the -R order) with read_id, species_taxid, genome_ID,\n"
            "                     strain_taxid, n_compatible, posterior of the reported strain that contains the read's nodes (one rank only)\n"
            "  --strain-coverage F   per-strain coverage track: for every row of strain_abundance.txt the windows along its genome with species_taxid,\n"
            "                     strain_taxid, genome_ID, start, end, n_nodes, len, covered, bases, depth, breadth (a node counts where it starts; one rank only)\n"
            "  --strain-coverage-window N   its window in bases (default 10000)\n"
            "  --strain-evidence F   per-strain node evidence: for every row of strain_abundance.txt the nodes it walks (class all) and the nodes no other\n"
            "                     reported strain of its species walks (private), then per species every node (total), the nodes no reported strain walks\n"
            "                     (orphan) and the nodes all of them walk (core): n_nodes, len, covered, bases, depth, breadth (one rank only)\n"
            "  --strain-read-support F   per-strain read support: for every row of strain_abundance.txt the reads compatible with it, compatible with it alone\n"
            "                     (unique) and assigned to it, then per species the counted reads, those no reported strain explains (unexplained), those of\n"
            "                     several strains (ambiguous) and of all of them (uninformative), then the reads every pair of strains shares (one rank only)\n"
            "  --strain-depth F   per-strain depth distribution: for every row of strain_abundance.txt the histogram of node depth over the nodes it walks\n"
            "                     (class all) and over those no other reported strain of its species walks (private), then per species over every node\n"
            "                     (total) and over the nodes no reported strain walks (orphan): n_nodes, len, len at depth 0, the length-weighted quantiles\n"
            "                     q05 q25 q50 q75 q95 as the lower bound of their bin, and the upper bound of the median's bin (one rank only)\n"
            "  --strain-near-miss F   unreported-strain near misses: per species the unreported haplotypes of the db that walk the most aligned bases on nodes\n"
            "                     no row of strain_abundance.txt walks (class novel), the part no other candidate walks (exclusive) and their whole walk (all),\n"
            "                     with the filter that dropped them; then per species the orphan nodes, those some candidate walks (claimed), those\n"
            "                     several do (contested) (one rank only)\n"
            "  --strain-near-miss-top N   candidates printed per species (default 5)\n"
            "  --strain-pair-evidence F   pairwise strain evidence: for every two rows of strain_abundance.txt of a species the nodes both walk (class shared)\n"
            "                     and the nodes only the one, only the other walks (only): n_nodes, len, covered, bases, depth, breadth, and whether the\n"
            "                     two are identical, nested or distinct on the graph (one rank only)\n"
            "  --strain-fit F   model fit: for every row of strain_abundance.txt over the nodes it walks (class all) and the nodes no other reported strain of\n"
            "                     its species walks (private) the aligned bases, the bases its predicted coverages put there (expected), what the sample has\n"
            "                     beyond them (excess), what it lacks (deficit) and the part of that on nodes without any coverage (blind), with\n"
            "                     fit = 1 - (excess + deficit) / (bases + expected); then per species every node (total), the nodes some reported strain walks\n"
            "                     (explained) and the nodes none walks (orphan) (one rank only)\n"
            "  --strain-bootstrap F   bootstrap of the strain fit: for every row of strain_abundance.txt the coverage a refit of the reported strains gives it and\n"
            "                     its mean, sd, quantiles and zero fraction over N Poisson resamples of the LP's rows, its share of the species and the share's\n"
            "                     0.025 and 0.975 quantiles; per species the rows and the objective (one rank only)\n"
            "  --strain-bootstrap-replicates N   resamples (default 100)     --strain-bootstrap-seed N   their seed (default 42)\n"
            "  --strain-dropout F   leave-one-out test of the strain fit: for every row of strain_abundance.txt the objective of a refit of the reported strains\n"
            "                     with and without it (delta), the rows it walks, walks alone, that fit worse and better without it, and the strain that takes\n"
            "                     over its coverage (substitute); per species the rows and the objective (one rank only)\n"
            "  --strain-addin F   add-one test of the strain fit: for the unreported haplotypes of a species that rank highest in the near-miss report the\n"
            "                     objective of a refit of the reported strains with the candidate in the LP (gain), the coverage it gets, the rows it walks,\n"
            "                     walks without a reported strain, that fit better and worse with it, and the reported strain it takes coverage from (donor);\n"
            "                     per species the rows, the objective and the rows no reported strain walks (one rank only)\n"
            "  --strain-addin-top N   candidates tested per species (default 5)\n"
            "  --strain-em F      read classes and a read-based estimate: the reads of a species grouped by the set of reported strains they are compatible\n"
            "                     with (reads, steps and aligned bases per set), and per row of strain_abundance.txt the depth that EM over those sets gives\n"
            "                     it, beside predicted_coverage; per species the unexplained reads and the iterations (one rank only)\n"
            "  --strain-em-classes N   sets printed per species, by bases (default 10)     --strain-em-iterations N   EM iterations at most (default 1000)\n"
            "  --strain-segments F   absent and amplified segments: per row of strain_abundance.txt the exact stretches of its genome, in path coordinates, that the\n"
            "                     sample does not cover at all (gap) and those at F times its predicted coverage and more (peak), with the totals of either class\n"
            "                     (one rank only)\n"
            "  --strain-segments-min N   bases a stretch spans at least (default 1000)     --strain-segments-bridge N   bases of another class that do not end a\n"
            "                     stretch (default 100; 0 is allowed)     --strain-segments-peak F|off   integer factor of a peak (default 10; off: gaps only)\n"
            "  --strain-mosaic F   mosaic reads: the reads of a species that fit no single row of strain_abundance.txt, cut into the fewest stretches that each\n"
            "                     fit one -- per species the reads by number of switches, per strain the stretches assigned to it, per pair of strains the\n"
            "                     switches between them, and the node pairs (junctions) where the reads switch (one rank only)\n"
            "  --strain-mosaic-top N|off   junctions printed per species, by count (default 10; off: none)\n"
            "  --strain-rescue F   read rescue: for the reads of a species that fit no row of strain_abundance.txt, whether a single unreported haplotype of\n"
            "                     the db walks all of a read's nodes -- per candidate the reads it rescues, per species the reads by class (one rank only)\n"
            "  --strain-rescue-top N   candidates printed per species, by rescued span (default 5)\n"
            "  --strain-links F    link support: which adjacencies (node u followed by node v) of every row of strain_abundance.txt the reads cross -- per\n"
            "                     strain its links crossed, open and broken (reads reach both sides, none goes across) and its deepest breaks, per species\n"
            "                     the read crossings that are a link of a reported strain, skip within one, switch between two or are foreign (one rank only)\n"
            "  --strain-links-top N   breaks printed per strain, by flank depth (default 10)\n"
            "  --strain-rarefy F   rarefaction: the strain fit again on nested subsamples of the READS (1/2, 1/4, ..) -- per row of strain_abundance.txt and level\n"
            "                     the refitted coverage over the replicates, scaled back to full depth, and how often it drops to 0 (one rank only)\n"
            "  --strain-rarefy-levels N   thinned levels 1/2 .. 2^-N (default 5, at most 16)\n"
            "  --strain-rarefy-replicates N   replicates per level (default 5)\n"
            "  --strain-rarefy-seed N   seed of the thinning rule (default 42)\n"
            "  --strain-fragments F   fragment support: read pairs (ids X/1 and X/2, or one id twice) as the unit of strain compatibility -- per row of\n"
            "                     strain_abundance.txt the fragments it is compatible with, alone, alone only as a pair, and assigned; per species the fragments\n"
            "                     concordant, discordant (each mate fits a reported strain, no common one), half and unexplained, the reads single, multi and\n"
            "                     with their mate elsewhere, and which two strains the discordant fragments sit between (one rank only)\n"
            "  --strain-growth F   replication index: per row of strain_abundance.txt the slope of the strain's OWN depth (nodes only it walks among the reported\n"
            "                     strains of its species) over its windows sorted by depth -- n_windows, n_kept, n_zero, n_fit, own_len, own_fraction, median_depth,\n"
            "                     slope, intercept, r2, index = 2^slope and status (ok, few_windows, low_depth, flat, empty); no origin is located (one rank only)\n"
            "  --strain-growth-window N   its window in bases (default 5000)     --strain-growth-min-own P   own bases a window needs, in thousandths of the\n"
            "                     window (default 500)     --strain-growth-trim P   windows trimmed from each end of the sorted range, in thousandths (default 100)\n"
            "  --image-cache 0|1|2  device-ready graph images <db>/species_graph_info/<otu>.hipdb: 1 = use, 2 = use and write\n"
            "  --filter-gaf  first replace the GAF by its best alignment per read (long reads; alignment.rs:171-175, gaf_filter.rs)\n"
            "  --filter-only <in.gaf> [<out.gaf>]   just write <stem>_filtered.gaf (or <out.gaf>) and exit\n"
            "  --db-pairs <out.tsv>   no sample: which strains of the db the strain step's LP can ever separate.  Per species every pair of haplotypes with the\n"
            "                     nodes and bases both walk, the bases only one of them walks and their sum (distance), class identical / nested / distinct,\n"
            "                     then per species its total, its core and its smallest distance; needs -db only (--gfa, --zip, --range-file, --device apply)\n"
            "  --db-pairs-species a,b,c   only these species (default: every species with more than one haplotype)\n"
            "  --db-pairs-max-distance N   only the pairs at most N bases apart (0: the identical ones)\n"
            "  --gfa (read species_gfa/*.gfa instead of species_graph_info/*.bin)  --zip serialize|lz|zstd  --round (2-decimal output)  --device N\n"
            "  --ranks N --rank r   one process per GPU (start N of them; device = r unless --device): every rank tokenises 1/N of the\n"
            "                       GAF, reads travel to the owner of their species over RCCL, rank 0 writes the tables\n"
            "                       (defaults from WORLD_SIZE / RANK / LOCAL_RANK when set); --comm-id-file F (default <wd>/.pantax_hip_rccl_id),\n"
            "                       --comm-nonce N (the same for all ranks of one launch; default from $TORCHELASTIC_RUN_ID / $MASTER_PORT; the id file must also be fresh),\n"
            "                       --comm-timeout S (default 300: a rank whose peers do not complete the RCCL bootstrap in time aborts it and exits non-zero)\n");
}

int main(int argc, char **argv) {
    pantax_hip_profiling_config c;
    memset(&c, 0, sizeof(c));
    std::string wd = "pantax_db_tmp";
    c.min_species_abundance = 1e-4; c.unique_trio_nodes_fraction = -1; c.unique_trio_nodes_mean_count_f = 0.46;
    c.single_cov_ratio = 0.85; c.single_cov_diff = 0.2; c.filtered = 1; c.full = 1; c.mode = 2; c.sample_nodes = 500000;
    c.zip = "serialize"; c.world_size = 1;
    bool long_read = false, filter_gaf = false;
    const char *filter_in = nullptr, *filter_out = nullptr;
    pantax_hip_profile_ext12 ext12;   // the outputs added behind the config's last field
    memset(&ext12, 0, sizeof(ext12));
    pantax_hip_profile_ext11 &ext11 = ext12.v11;
    pantax_hip_profile_ext10 &ext10 = ext11.v10;
    pantax_hip_profile_ext9 &ext9 = ext10.v9;
    pantax_hip_profile_ext8 &ext8 = ext9.v8;
    pantax_hip_profile_ext7 &ext7 = ext8.v7;
    pantax_hip_profile_ext6 &ext6 = ext7.v6;
    pantax_hip_profile_ext5 &ext5 = ext6.v5;
    pantax_hip_profile_ext4 &ext4 = ext5.v4;
    pantax_hip_profile_ext3 &ext3 = ext4.v3;
    pantax_hip_profile_ext2 &ext = ext3.v2;
    ext.v1.struct_size = sizeof(ext12);
    ext.strain_bootstrap_seed = 42;
    ext10.strain_rarefy_seed = 42;
    pantax_hip_db_pairs_config pairs;
    memset(&pairs, 0, sizeof(pairs));
    pairs.max_distance = -1;
    int device = -1, ranks = 0, rank = -1;
    std::string id_file;
    // per-launch nonce of the id file (rccl_comm.hpp): something that changes from one launch to the next where the launcher offers it
    // (torchrun: the run id + the restart count), else the rendezvous port; the file's age is checked in every case
    // (the launcher's variables are read here, once, before any thread exists: the one place the CLI looks at the environment)
    auto env = [](const char *name) -> const char * { return std::getenv(name); };
    uint64_t nonce = env("MASTER_PORT") ? strtoull(env("MASTER_PORT"), nullptr, 10) : 0;
    double comm_timeout = 300.0;     // --comm-timeout: seconds the whole RCCL bootstrap may take before this rank gives up and exits non-zero
    if (const char *rid = env("TORCHELASTIC_RUN_ID")) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (const char *q = rid; *q; ++q) { h ^= (uint64_t)(unsigned char)*q; h *= 0x100000001b3ull; }
        if (const char *rc = env("TORCHELASTIC_RESTART_COUNT")) h = h * 31 + strtoull(rc, nullptr, 10);
        nonce ^= h ? h : 1;
    }
    if (const char *ev = env("WORLD_SIZE")) ranks = atoi(ev);
    if (const char *ev = env("RANK")) rank = atoi(ev);
    if (const char *ev = env("LOCAL_RANK")) device = atoi(ev);
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char * { if (i + 1 >= argc) { usage(); exit(2); } return argv[++i]; };
        if (a == "-db" || a == "--db") c.db = next();
        else if (a == "--gaf") c.input_aln_file = next();
        else if (a == "-T") wd = next();
        else if (a == "--species" || a == "-s") c.species = 1;
        else if (a == "--strain" || a == "-S") c.strain = 1;
        else if (a == "--short-read") long_read = false;
        else if (a == "--long-read") long_read = true;
        else if (a == "--fr") c.unique_trio_nodes_fraction = atof(next());
        else if (a == "--fc") c.unique_trio_nodes_mean_count_f = atof(next());
        else if (a == "-a") c.min_species_abundance = atof(next());
        else if (a == "--sr") c.single_cov_ratio = atof(next());
        else if (a == "--sd") c.single_cov_diff = atof(next());
        else if (a == "--shift") c.shift = !strcasecmp(next(), "true");
        else if (a == "--min_cov") c.min_cov = atoll(next());
        else if (a == "--min_depth") c.min_depth = atoll(next());
        else if (a == "--sample") c.sample_nodes = atoi(next());
        else if (a == "--sample_test" || a == "--sample-test") c.sample_test = 1;      // cli.rs:230-232
        else if (a == "--solver") {                                                    // cli.rs:158-160: whose handling of the second solve is reproduced
            const char *sv = next();
            c.solver_semantics = !strcasecmp(sv, "highs") ? PANTAX_HIP_SEMANTICS_HIGHS : PANTAX_HIP_SEMANTICS_GUROBI;   // gurobi, cplex, cbc, glpk agree (profile.rs:1500, :1906, :2125, :2672)
        }
        else if (a == "--ds") c.designated_species = next();
        else if (a == "--smode") c.mode = atoi(next());
        else if (a == "--no-filter") c.filtered = 0;
        else if (a == "--force") c.force = 1;
        else if (a == "-R" || a == "--report") c.out_binning_file = next();
        else if (a == "--range-file") c.range_file = next();
        else if (a == "--species-len-file") c.species_len_file = next();
        else if (a == "--reads-binning-file") c.reads_binning_file = next();
        else if (a == "--read-strains") c.read_strain_file = next();
        else if (a == "--strain-coverage") c.strain_coverage_file = next();
        else if (a == "--strain-coverage-window") c.strain_coverage_window = atoll(next());
        else if (a == "--strain-evidence") c.strain_evidence_file = next();
        else if (a == "--strain-read-support") c.strain_read_support_file = next();
        else if (a == "--strain-depth") c.strain_depth_file = next();
        else if (a == "--strain-near-miss") c.strain_near_miss_file = next();
        else if (a == "--strain-near-miss-top") c.strain_near_miss_top = atoi(next());
        else if (a == "--strain-pair-evidence") c.strain_pair_evidence_file = next();
        else if (a == "--strain-fit") ext.v1.strain_fit_file = next();
        else if (a == "--strain-bootstrap") ext.strain_bootstrap_file = next();
        else if (a == "--strain-bootstrap-replicates") ext.strain_bootstrap_replicates = strtoull(next(), nullptr, 10);
        else if (a == "--strain-bootstrap-seed") ext.strain_bootstrap_seed = strtoull(next(), nullptr, 10);
        else if (a == "--strain-dropout") ext3.strain_dropout_file = next();
        else if (a == "--strain-addin") ext4.strain_addin_file = next();
        else if (a == "--strain-addin-top") ext4.strain_addin_top = strtoull(next(), nullptr, 10);
        else if (a == "--strain-em") ext5.strain_em_file = next();
        else if (a == "--strain-em-classes") ext5.strain_em_classes = strtoull(next(), nullptr, 10);
        else if (a == "--strain-em-iterations") ext5.strain_em_iterations = strtoull(next(), nullptr, 10);
        else if (a == "--strain-segments") ext6.strain_segments_file = next();
        else if (a == "--strain-segments-min") ext6.strain_segments_min = strtoull(next(), nullptr, 10);
        else if (a == "--strain-segments-bridge") ext6.strain_segments_bridge = strtoull(next(), nullptr, 10) + 1;   // the field holds bridge + 1 (0: the default)
        else if (a == "--strain-segments-peak") { const std::string v = next(); ext6.strain_segments_peak = v == "off" ? PANTAX_HIP_SEGMENTS_PEAK_OFF : strtoull(v.c_str(), nullptr, 10); }
        else if (a == "--strain-mosaic") ext7.strain_mosaic_file = next();
        else if (a == "--strain-mosaic-top") { const std::string v = next(); ext7.strain_mosaic_top = v == "off" ? PANTAX_HIP_MOSAIC_TOP_OFF : strtoull(v.c_str(), nullptr, 10); }
        else if (a == "--strain-rescue") ext8.strain_rescue_file = next();
        else if (a == "--strain-rescue-top") ext8.strain_rescue_top = strtoull(next(), nullptr, 10);
        else if (a == "--strain-links") ext9.strain_links_file = next();
        else if (a == "--strain-links-top") ext9.strain_links_top = strtoull(next(), nullptr, 10);
        else if (a == "--strain-rarefy") ext10.strain_rarefy_file = next();
        else if (a == "--strain-rarefy-levels") ext10.strain_rarefy_levels = strtoull(next(), nullptr, 10);
        else if (a == "--strain-rarefy-replicates") ext10.strain_rarefy_replicates = strtoull(next(), nullptr, 10);
        else if (a == "--strain-rarefy-seed") ext10.strain_rarefy_seed = strtoull(next(), nullptr, 10);
        else if (a == "--strain-fragments") ext11.strain_fragments_file = next();
        else if (a == "--strain-growth") ext12.strain_growth_file = next();
        else if (a == "--strain-growth-window") ext12.strain_growth_window = strtoull(next(), nullptr, 10);
        else if (a == "--strain-growth-min-own") ext12.strain_growth_min_own_permille = strtoull(next(), nullptr, 10);
        else if (a == "--strain-growth-trim") ext12.strain_growth_trim_permille = strtoull(next(), nullptr, 10);
        else if (a == "--gfa") c.zip = nullptr;
        else if (a == "--zip") c.zip = next();        // serialize | lz | zstd (main.rs: --zip)
        else if (a == "--round") c.full = 0;
        else if (a == "--filter-gaf") filter_gaf = true;
        else if (a == "--image-cache") c.image_cache = atoi(next());
        else if (a == "--filter-only") { filter_in = next(); if (i + 1 < argc && argv[i + 1][0] != '-') filter_out = argv[++i]; }
        else if (a == "--db-pairs") pairs.out_file = next();
        else if (a == "--db-pairs-species") pairs.species = next();
        else if (a == "--db-pairs-max-distance") pairs.max_distance = atoll(next());
        else if (a == "--device") device = atoi(next());
        else if (a == "--ranks") ranks = atoi(next());
        else if (a == "--rank") rank = atoi(next());
        else if (a == "--comm-id-file") id_file = next();
        else if (a == "--comm-nonce") nonce = strtoull(next(), nullptr, 10);
        else if (a == "--comm-timeout") comm_timeout = atof(next());
        else { usage(); return 2; }
    }
    const bool use_rccl = ranks >= 1 && rank >= 0;   // also a one-rank world goes through the communicator when asked for
    if (use_rccl && rank >= ranks) { fprintf(stderr, "pantax-hip: --rank %d of --ranks %d\n", rank, ranks); return 2; }
    if (device < 0) device = use_rccl ? rank : 0;
    if (filter_in) {
        pantax_hip_ctx *fctx = nullptr;
        if (pantax_hip_init(&fctx, &device, 1) != 0) { fprintf(stderr, "pantax-hip: %s\n", pantax_hip_last_error(nullptr)); return 1; }
        uint64_t nl = 0, nr = 0, nw = 0;
        const int frc = pantax_hip_gaf_filter(fctx, filter_in, filter_out, &nl, &nr, &nw);
        if (frc != 0) fprintf(stderr, "pantax-hip: error %d: %s\n", frc, pantax_hip_last_error(fctx));
        else printf("Filtered GAF: %llu lines, %llu alignment records, %llu written\n", (unsigned long long)nl, (unsigned long long)nr, (unsigned long long)nw);
        pantax_hip_destroy(fctx);
        return frc == 0 ? 0 : 1;
    }
    if (pairs.out_file) {   // a mode of its own, beside --filter-only: no GAF, no work directory, one rank
        if (!c.db) { usage(); return 2; }
        if (pairs.max_distance < -1) { fprintf(stderr, "pantax-hip: --db-pairs-max-distance %lld\n", (long long)pairs.max_distance); return 2; }
        pairs.db = c.db; pairs.range_file = c.range_file; pairs.zip = c.zip;
        pantax_hip_ctx *pctx = nullptr;
        if (pantax_hip_init(&pctx, &device, 1) != 0) { fprintf(stderr, "pantax-hip: %s\n", pantax_hip_last_error(nullptr)); return 1; }
        const int prc = pantax_hip_db_pairs(pctx, &pairs);
        if (prc != 0) fprintf(stderr, "pantax-hip: error %d: %s\n", prc, pantax_hip_last_error(pctx));
        pantax_hip_destroy(pctx);
        return prc == 0 ? 0 : 1;
    }
    if (!c.db || !c.input_aln_file) { usage(); return 2; }
    if (c.unique_trio_nodes_fraction < 0) c.unique_trio_nodes_fraction = long_read ? 0.5 : 0.3;   // main.rs:108-114
    c.wd = wd.c_str(); c.output_dir = wd.c_str();
    pantax_hip_ctx *ctx = nullptr;
    int rc = pantax_hip_init(&ctx, &device, 1);
    if (rc != 0) { fprintf(stderr, "pantax-hip: %s\n", pantax_hip_last_error(nullptr)); return 1; }
    // the communicator first: with --filter-gaf only rank 0 rewrites the shared GAF, and the others must not open it before
    // the rename (the sharded ingest assumes ONE immutable file) -- the all-reduce below is that barrier and carries a failure
    // of the filter to every rank, so all of them leave together
    RcclComm comm;
    if (use_rccl) {
        if (id_file.empty()) id_file = wd + "/.pantax_hip_rccl_id";
        if (!comm.init(rank, ranks, id_file, nonce, comm_timeout)) {
            fprintf(stderr, "pantax-hip: rank %d: %s\n", rank, comm.err.c_str());
            if (comm.abandoned) { if (rank == 0) ::unlink(id_file.c_str()); fflush(stderr); _exit(3); }   // the bootstrap thread is still inside RCCL: no teardown may wait for it
            pantax_hip_destroy(ctx);
            return 1;
        }
        c.rank = rank; c.world_size = ranks; c.comm_user = &comm;
        c.allreduce_sum = &RcclComm::allreduce_sum; c.alltoallv = &RcclComm::alltoallv; c.comm_device_buffers = 1;
    }
    if (filter_gaf) {   // alignment.rs:171-175: filter, then the filtered file takes the GAF's place
        int frc = 0;
        if (!use_rccl || rank == 0) {
            const std::string filtered = std::string(c.input_aln_file) + ".best.tmp";
            frc = pantax_hip_gaf_filter(ctx, c.input_aln_file, filtered.c_str(), nullptr, nullptr, nullptr);
            if (frc != 0) fprintf(stderr, "pantax-hip: error %d: %s\n", frc, pantax_hip_last_error(ctx));
            else if (rename(filtered.c_str(), c.input_aln_file) != 0) { fprintf(stderr, "pantax-hip: cannot replace %s\n", c.input_aln_file); frc = 1; }
        }
        double failed = frc != 0 ? 1.0 : 0.0;
        if (use_rccl && RcclComm::allreduce_sum(&comm, &failed, 1) != 0) { fprintf(stderr, "pantax-hip: rank %d: the exchange behind --filter-gaf failed\n", rank); failed = 1.0; }
        if (failed != 0.0) { if (use_rccl) comm.destroy(id_file); pantax_hip_destroy(ctx); return 1; }
    }
    rc = pantax_hip_profile_with_ext(ctx, &c, &ext.v1);
    if (rc != 0) fprintf(stderr, "pantax-hip: %serror %d: %s\n", use_rccl ? ("rank " + std::to_string(rank) + ": ").c_str() : "", rc, pantax_hip_last_error(ctx));
    if (use_rccl) comm.destroy(id_file);
    pantax_hip_destroy(ctx);
    return rc == 0 ? 0 : 1;
}
