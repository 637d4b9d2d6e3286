/*
 * pantax_hip.h -- C ABI of the MI355X-native PanTax profiling path.
 *
 * This is the drop-in boundary: a Rust `extern "C"` block
 * (or cgo / ctypes) binds to exactly these symbols.  Plain pointers and sizes
 * only; every array is caller-owned and only read unless marked [out].
 * Conventions: 0 = success, negative = pantax_hip_status; nothing aborts or
 * throws across the boundary; one ctx per process per GPU; calls on one ctx are
 * serialised on its HIP stream.
 *
 * Reference seams this replaces (paths relative to pantax/src):
 *   - pipeline seam:  profile::profile(ProfilingConfig)            profile.rs:3325 (called main.rs:51-54)
 *   - solver seam:    match args.solver { "gurobi" | "highs" ... } profile.rs:2969-3009
 *                     fn X_opt(&mut GurobiOptVar, nvert, paths, node_abundance_vec,
 *                              node_base_cov, node_len, args)        profile.rs:2690-2698
 *   - histogram seam: get_node_abundances(...)                      profile.rs:743-750
 *   - binning seam:   rcls::rcls_profile / process_single_read_simple  rcls.rs:452-458, 237-258
 * INTEGRATION.md shows the Rust-side binding for each.
 */
#ifndef PANTAX_HIP_H
#define PANTAX_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PANTAX_HIP_OK = 0,
    PANTAX_HIP_E_INVALID = -1,       /* bad argument */
    PANTAX_HIP_E_HIP = -2,           /* HIP runtime error (message in last_error) */
    PANTAX_HIP_E_NO_DEVICE = -3,     /* no usable gfx950 device: the product never falls back to CPU */
    PANTAX_HIP_E_LIMIT = -4,         /* size limit of this build (32-bit node / step / row positions; > 30000 haplotypes in one species) */
    PANTAX_HIP_E_SOLVER = -5,        /* LP did not reach optimality (reference: Err(e) => species dropped, profile.rs:2999-3003) */
    PANTAX_HIP_E_IO = -6,            /* file missing / malformed (pipeline seam) */
    PANTAX_HIP_E_STATE = -7          /* stage called before its prerequisite */
} pantax_hip_status;

typedef struct pantax_hip_ctx pantax_hip_ctx;     /* owns the HIP stream, scratch, timers */
typedef struct pantax_hip_db pantax_hip_db;       /* device-resident graphs of the species this rank owns */
typedef struct pantax_hip_reads pantax_hip_reads; /* device-resident packed alignment records */

/* Threading: every entry point may be called from any host thread; calls that share a ctx are serialised inside
 * (the reference calls its solver from rayon workers, profile.rs:3297-3304).  Error text is per calling thread. */
/* ONE ctx drives ONE GPU, and a process holds one ctx per GPU it uses: the design is one process per GPU (a Rust host starts N
 * processes, or N threads with one ctx each).  device_ids / n_devices keep SURVEY 8b's signature; n_devices must be 1, anything
 * else is PANTAX_HIP_E_INVALID.  The environment is read HERE and nowhere else: every PANTAX_<OPTION> variable sets the option of
 * that name (lower case) once; afterwards options change only through pantax_hip_set_option -- no entry point calls getenv on its
 * way, so a host thread that changes the environment beside a running call cannot race with the library. */
int pantax_hip_init(pantax_hip_ctx **out, const int *device_ids, int n_devices);
void pantax_hip_destroy(pantax_hip_ctx *ctx);
/* options of a ctx: "hip_trace" (phase times on stderr), "stage_threads" (host threads that fill the pinned upload ring),
 * "gaf_piece_bytes", and the switches that force one of the in-tree HIP paths for tests and measurements (pantax_amd/csrc/common.hpp
 * CtxConfig lists them).  value NULL = the default.  PANTAX_HIP_E_INVALID for an unknown name or an unparsable value. */
int pantax_hip_set_option(pantax_hip_ctx *ctx, const char *name, const char *value);
/* Which LDS shape ("roomy" / "compact") the LAD solver takes under the ctx's option "lad_shape" for a batch of n_species LPs of at most max_columns
 * columns on this ctx's device: the host rule the solver launches follow, for tests and logs.  NULL for a NULL ctx. */
const char *pantax_hip_lad_shape_name(const pantax_hip_ctx *ctx, uint32_t n_species, int max_columns);
const char *pantax_hip_last_error(const pantax_hip_ctx *ctx); /* ctx may be NULL: init errors */
const char *pantax_hip_version(void);

/* ---- DB side: types.rs:51-55 `Graph` of every species, concatenated ---------------------- */
typedef struct {
    uint32_t n_species;
    const int64_t *range_start; /* [S] first global node id, 1-based (species_range.txt col 2) */
    const int64_t *range_end;   /* [S] last global node id (col 3) */
    const uint64_t *node_off;   /* [S+1] species s owns node_len[node_off[s] .. node_off[s+1]) */
    const int64_t *node_len;    /* [V] Graph::nodes_len */
    const uint64_t *hap_off;    /* [S+1] species s owns haplotypes [hap_off[s] .. hap_off[s+1]) in BTreeMap (byte) order */
    const uint64_t *path_off;   /* [H+1] walk of hap h = path_nodes[path_off[h] .. path_off[h+1]) */
    const uint32_t *path_nodes; /* [P] species-local 0-based node ids (Graph::paths values) */
} pantax_hip_graphs;

int pantax_hip_db_upload(pantax_hip_ctx *ctx, const pantax_hip_graphs *g, pantax_hip_db **out);
/* the same db from one `Graph` per species as the host holds them after load_from_zip_graph (zip.rs:236-283) -- nothing is
 * concatenated on the host: the arrays travel species by species through one pinned chunk pipeline, lengths and walks are checked
 * on the device (length > 0, profile.rs:494; every walk inside its graph, :849) */
typedef struct {
    uint64_t n_nodes, n_haps;
    const int64_t *node_len;    /* [n_nodes] Graph::nodes_len */
    const uint64_t *path_off;   /* [n_haps+1] local CSR of the walks, haplotypes in BTreeMap (byte) order */
    const uint32_t *path_nodes; /* [path_off[n_haps] - path_off[0]] species-local 0-based node ids */
} pantax_hip_graph_part;
int pantax_hip_db_upload_parts(pantax_hip_ctx *ctx, uint32_t n_species, const int64_t *range_start, const int64_t *range_end,
                               const pantax_hip_graph_part *parts, pantax_hip_db **out);
void pantax_hip_db_free(pantax_hip_ctx *ctx, pantax_hip_db *db);

/* ---- read side: packed form of the GAF columns rcls.rs:127-137 selects ------------------- */
#define PANTAX_HIP_READ_NULLFIELD 1u /* a selected column was `*`: dropped at strain level, profile.rs:380-399 */
#define PANTAX_HIP_READ_DUPDROP 2u   /* duplicate read id spanning >1 species, profile.rs:406-437 */
typedef struct {
    uint64_t n_reads;
    uint64_t n_steps;
    const uint32_t *step_off; /* [R+1] */
    const uint32_t *node_id;  /* [T] node ids exactly as written in GAF col 6 */
    const uint32_t *pstart;   /* [R] GAF col 8 (read_start) */
    const uint32_t *pend;     /* [R] GAF col 9 (read_end) */
    const uint32_t *qlen;     /* [R] GAF col 2 (read_len) */
    const uint8_t *mapq;      /* [R] GAF col 12; 255 = null */
    const uint8_t *flags;     /* [R] PANTAX_HIP_READ_* or NULL */
} pantax_hip_packed_reads;

int pantax_hip_reads_upload(pantax_hip_ctx *ctx, const pantax_hip_packed_reads *r, pantax_hip_reads **out);
void pantax_hip_reads_free(pantax_hip_ctx *ctx, pantax_hip_reads *reads);

/* ---- a2 + a3: read -> species binning (rcls.rs:237-258) and the species counters
 * (profile.rs:208-297).  species_idx_out[r] = index into the db's species or -1 ("U").
 * Counter arrays are [n_species]; any out pointer may be NULL. */
int pantax_hip_bin_reads(pantax_hip_ctx *ctx, const pantax_hip_db *db, pantax_hip_reads *reads,
                         int32_t *species_idx_out, int64_t *read_count_out, int64_t *base_sum_out,
                         int64_t *less_multi_out, int64_t *uniq_count_out);

/* a3 finishing (species_profiling, profile.rs:299-349): equal-length test on the first 1000 reads
 * with species != "U" (:312-319), the MAPQ filter when `filtered` (:239-245), absolute =
 * base_count / avg_len (:336), abundance = absolute / sum (:341).  avg_len[s] <= 0 = species missing
 * from species_genomes_stats.txt.  Outputs [n_species]; rows are in db order (callers sort by
 * abundance, :344).  Requires bin_reads of `reads` against `db` (else PANTAX_HIP_E_STATE). */
int pantax_hip_species_profile(pantax_hip_ctx *ctx, const pantax_hip_db *db, pantax_hip_reads *reads,
                               const int64_t *read_count, const int64_t *base_sum, const int64_t *less_multi,
                               const int64_t *uniq_count, const double *avg_len, int filtered,
                               uint8_t *keep_out, double *absolute_out, double *abundance_out);

/* drop everything derived from the graphs (trio index, coverage state) so the next calls rebuild it:
 * the reference recomputes trio_nodes_info inside every optimize_otu call (profile.rs:2936). */
int pantax_hip_db_reset(pantax_hip_ctx *ctx, pantax_hip_db *db);

/* ---- a7: unique-trio index (profile.rs:658-740), built on device once per db.
 * Rows are ordered (species, hap, window position). */
int pantax_hip_trio_index(pantax_hip_ctx *ctx, pantax_hip_db *db, uint64_t *n_unique_total_out);
/* copy the table out: abc [3*U] canonical species-local keys, hap [U] hap index within
 * its species, len [U], hap_trio_off [H+1] (global hap numbering). NULLs are skipped. */
int pantax_hip_trio_get(pantax_hip_ctx *ctx, const pantax_hip_db *db, uint32_t *abc_out, uint32_t *hap_out,
                        int64_t *len_out, uint64_t *hap_trio_off_out);

/* ---- a8: get_node_abundances integer part (profile.rs:743-1026).  Requires bin_reads of `reads` against `db`
 * (else PANTAX_HIP_E_STATE: the slot records of binned reads hold species indices and node bases of ONE db; and trio_index if trio_bases_out != NULL).  species_active: [S] 0/1 or NULL = all
 * (the species load_species_range keeps, profile.rs:553-656).  Outputs: [V], [V], [U].
 * n_abort_out counts reads on which the reference would abort (assert profile.rs:854 /
 * index panic :849); they contribute nothing. */
int pantax_hip_node_coverage(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads,
                             const uint8_t *species_active, int64_t *bases_per_node_out,
                             uint64_t *node_base_cov_out, int64_t *trio_bases_out, uint64_t *n_abort_out);

/* ---- a9..a14: strain level for every active species (optimize_otu profile.rs:2884-3026,
 * abundace_constraint :3028-3070).  Requires node_coverage to have run on (db, reads). */
#define PANTAX_HIP_HAS_FRACTION 1u
#define PANTAX_HIP_HAS_FREQ_MEAN 2u
#define PANTAX_HIP_HAS_RATIO 4u
#define PANTAX_HIP_HAS_FIRST 8u
#define PANTAX_HIP_HAS_DIVERGENCE 16u
#define PANTAX_HIP_HAS_SECOND 32u
#define PANTAX_HIP_HAS_RESCUE 64u
#define PANTAX_HIP_HAS_TOTAL_DIFF 128u
typedef struct { /* HapMetrics, profile.rs:1065-1078; `has` bit = Option::is_some() */
    uint32_t has;
    int32_t is_rescue;
    double unique_trio_nodes_fraction, frequencies_mean, path_cov_ratio, first_sol, divergence, second_sol,
        total_cov_diff;
} pantax_hip_hap_metrics;

typedef struct { /* the ProfilingConfig fields optimize_otu reads (types.rs:57-91, defaults main.rs:102-171) */
    double unique_trio_nodes_fraction;     /* --fr: 0.3 short / 0.5 long */
    double unique_trio_nodes_mean_count_f; /* --fc 0.46 */
    double single_cov_ratio;               /* --sr 0.85 */
    int64_t min_depth;                     /* --min_depth 0 */
    int32_t shift;                         /* --shift */
    int32_t sample_nodes;                  /* --sample (cli.rs:227 default 500000; pass 500 for --sample_test): a species with more valid
                                            * LP rows keeps the rows of sample_sorted (profile.rs:1287-1295); 0 = never sample */
    int32_t solver_semantics;              /* which backend's handling of the SECOND solve's solution is reproduced (the LP and its optimum are the same for all):
                                            * PANTAX_HIP_SEMANTICS_GUROBI (0, default; also cplex / cbc / glpk): every candidate that survives
                                            * second_filter_paths takes its own x of the second solve (profile.rs:1500-1508);
                                            * PANTAX_HIP_SEMANTICS_HIGHS (1): highs_opt first cuts the solution to its first K columns, K = number of
                                            * survivors, and zips THAT with the candidates (profile.rs:2865-2879) -- a survivor at candidate position
                                            * >= K is left without a second_sol (it then counts as 0, :3036, and is dropped from the table, :3237).
                                            * What a maintainer without a Gurobi licence can diff against is `--solver highs`: this switch makes that
                                            * diff come out empty. */
} pantax_hip_strain_config;
#define PANTAX_HIP_SEMANTICS_GUROBI 0
#define PANTAX_HIP_SEMANTICS_HIGHS 1

typedef struct { /* per species solver report */
    int32_t n_candidates, status1, status2, iters1, iters2;
    uint32_t n_rows, n_patterns;
    double obj1, obj2;
} pantax_hip_solve_info;

int pantax_hip_strain_profile(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_strain_config *cfg,
                              const uint8_t *species_active /*[S] or NULL*/,
                              const double *species_coverage /*[S] predicted_coverage, profile.rs:3044-3047*/,
                              pantax_hip_hap_metrics *metrics_out /*[H]*/, pantax_hip_solve_info *info_out /*[S] or NULL*/);

/* a15 core (abundance_est, profile.rs:3219-3245), host only: pass_out[h] = (group_size > 1 ||
 * total_cov_diff <= single_cov_diff) && predicted_coverage >= min_cov && predicted_coverage != 0;
 * sum_all_out = sum of every non-null predicted_coverage (the :3198 normaliser), sum_pass_out = the
 * same over passing rows (:3243).  These two numbers are the only cross-GPU reduction of the path. */
int pantax_hip_abundance_filter(uint32_t n_species, const uint64_t *hap_off, const pantax_hip_hap_metrics *metrics,
                                const uint8_t *species_reported /*[S] 0 = species dropped (solver error / inactive)*/,
                                double single_cov_diff, int64_t min_cov, uint8_t *pass_out,
                                double *sum_all_out, double *sum_pass_out,
                                double *species_sum_all_out /*[S] or NULL*/, double *species_sum_pass_out /*[S] or NULL*/);

/* ---- per-read strain assignment (the --read-strains report; not a stage of the reference): which candidate strain of its species
 * every read supports.  N(r) = the distinct nodes of the walk of read r; C(r) = the candidates of r's species whose walk visits every
 * node of N(r) (node-set containment: order and orientation ignored, the node-level model of the LP, profile.rs:1333-1342).  The
 * assigned strain is the argmax of the weight over C(r), ties to the smallest species-local haplotype index; posterior = w_assigned /
 * the sum of w over C(r), summed in f64 in ascending haplotype index.  The file seam takes the rows of strain_abundance.txt as the
 * candidates (the a15 filter, pantax_hip_abundance_filter's pass_out) and their unrounded predicted_coverage as the weights.
 * Requires pantax_hip_bin_reads of `reads` against `db` (else PANTAX_HIP_E_STATE).  Outputs are host arrays of R entries in file order;
 * ONLY the entries of reads binned to a species of `db` are written (every other entry keeps what the caller put there, so a caller
 * can loop over groups of species):
 *   counted reads (the coverage pass uses them): hap_out = species-local haplotype index of the assigned strain, n_out = |C(r)|,
 *     post_out = posterior; C(r) empty: 0xFFFFFFFF, 0, 0.0;
 *   reads dropped by their flags (null field, duplicate-id rule) and reads of a species without candidates: 0xFFFFFFFF, -1, 0.0. */
typedef struct {
    uint32_t n_species;         /* must equal the db's */
    const uint64_t *cand_off;   /* [S+1] species s owns candidates [cand_off[s], cand_off[s+1]) */
    const uint32_t *cand_hap;   /* [C] species-local haplotype index (any order, no repeats) */
    const double *cand_w;       /* [C] weight of the candidate */
} pantax_hip_read_strain_set;
int pantax_hip_read_strains(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand,
                            uint32_t *hap_out /*[R]*/, int32_t *n_out /*[R]*/, double *post_out /*[R]*/);

/* ---- per-strain read support (the --strain-read-support report; not a stage of the reference): how many reads support every candidate strain, how many
 * support it alone, how many reads of the species fit no candidate, and which candidates the reads cannot tell apart.  The inputs, a counted read, N(r),
 * C(r) and the assigned strain are those of pantax_hip_read_strains above (argmax of w over C(r), ties to the smallest haplotype index; node-set
 * containment).  K_s = the candidates of species s.  For a counted read r of species s:
 *   Q(r) = (1, n_steps(r), span(r)), all u64: n_steps = the steps of the read's walk, span = pend - pstart of the read (0 if pend < pstart).
 * Every output is a sum of Q(r), its three numbers in the order { n_reads, n_steps, span }:
 *   per candidate entry c (haplotype h of species s), hap_out [C][3][3] in the order of cand_hap:
 *     compatible[c] = sum over h in C(r);   unique[c] = sum over C(r) = {h};   assigned[c] = sum over the reads assigned to h;
 *   per species, species_out [S][4][3]:
 *     counted[s] = sum over every counted read of s (also when K_s = 0);   unexplained[s] = sum over C(r) empty;   ambiguous[s] = sum over |C(r)| >= 2;
 *     uninformative[s] = sum over |C(r)| = K_s;   the last three are three zeros each when K_s = 0;
 *   shared reads, pair_out [pair_off[S]] (n_reads only): pair_out[pair_off[s] + a * K_s + b] = the counted reads with the candidates at positions a and b of
 *     the species' candidate list both in C(r); symmetric, the diagonal equals compatible.n_reads.  A species of K_s > 64 owns no block (pair_off does not
 *     advance for it).  pair_off_out [S+1] is computed on the host and always written; more than pair_cap entries: PANTAX_HIP_E_LIMIT with nothing else
 *     touched (call with pair_cap = 0 to size pair_out).
 * Integers only: results are exact and independent of any order.  For every species of K_s >= 1: counted = unexplained + sum of assigned;
 * sum of unique + ambiguous + unexplained = counted; unique <= assigned <= compatible.  State rules and PANTAX_HIP_E_INVALID cases of
 * pantax_hip_read_strains.  An empty candidate set is fine: counted is still written. */
int pantax_hip_strain_read_support(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand,
                                   uint64_t *hap_out /*[C][3][3]: compatible, unique, assigned*/,
                                   uint64_t *species_out /*[S][4][3]: counted, unexplained, ambiguous, uninformative*/,
                                   uint64_t *pair_off_out /*[S+1]*/, uint64_t pair_cap /* entries pair_out holds */, uint64_t *pair_out);

/* ---- read classes and the read-based estimate (the --strain-em report; not a stage of the reference): the reads of a species grouped by the set of
 * candidate strains they are compatible with, and a depth per candidate from EM over those groups -- an estimate that does not come from the LP.  A counted
 * read, N(r), C(r), Q(r) = (1, n_steps, span) and the state rules are exactly those of pantax_hip_strain_read_support above.  The candidate set is a
 * pantax_hip_read_strain_set with cand_len (the graph bases G of the candidate, u64) in place of the weights, max_iter >= 1 and tol >= 0, finite (else
 * PANTAX_HIP_E_INVALID).
 *   Canonical order: the candidates of a species are taken in ascending haplotype index, whatever the caller's order; bit i of a class mask is the candidate
 *   with the i-th smallest haplotype index.  The caller's order decides only where a candidate's x lands in x_out.
 *   Read classes, for a species of 1 <= K_s <= 64: a class is a distinct non-zero mask m = C(r) with the u64 sums of Q(r) over its reads; classes are listed
 *   in ascending mask (unsigned), species after species.  species_out [S][2][3] = counted and unexplained (C(r) empty) as in read support, both also written
 *   for K_s = 0 (unexplained = 0 there).  Integers only: exact and independent of any order.  K_s > 64: the species is skipped -- no classes, no estimate,
 *   x = 0; the call still succeeds and counted is still written.
 *   Sizing: cls_off_out [S+1] is always written.  cls_mask_out [cls_off[S]] and cls_q_out [cls_off[S]][3] are written when cls_cap holds them; cls_cap > 0
 *   but too small: PANTAX_HIP_E_LIMIT with nothing else touched; cls_cap = 0 (the arrays may be null) is fine: a caller that only wants the estimate, or
 *   wants to size the arrays, calls it this way.
 *   The estimate, per species over its classes j = 0 .. J-1 in that order, b_j = span of class j, G_k = cand_len of the candidate at bit k, in f64 with IEEE
 *   add, mul, div and u64 -> f64 conversion only (no contraction, no reassociation):
 *     x_k = 1.0 if G_k > 0 else 0.0
 *     for t = 1 .. max_iter:
 *       D_j = sum of x_k over the set bits k of m_j, ascending k, from 0.0;      r_j = (double)b_j / D_j if D_j > 0.0, else 0.0
 *       R_k = sum of r_j over the classes j with bit k set, ascending j, from 0.0
 *       y_k = (x_k * R_k) / (double)G_k;  0.0 if G_k == 0;  0.0 if y_k < 1e-200
 *       delta = max_k |y_k - x_k|;  top = max_k y_k;  x = y;  n_iter = t;  if delta <= tol * top: converged = 1, stop
 *   This is the EM of the Poisson model "class j collects bases at rate sum_{k in m_j} x_k, strain k spreads over G_k bases"; its fixed point maximises
 *   sum_j b_j log D_j - sum_k G_k x_k, and identical strains get equal depth.  The 1e-200 floor keeps the iteration out of denormals; it is part of the
 *   contract.  x_out [C] in the caller's order, iter_out / converged_out / delta_out [S]; a species of K_s = 0, a skipped one or one without classes gets
 *   zeros and n_iter = 0.  The same inputs give the same bits, whatever the membership route (option read_strain_route=walk), the table size (option
 *   read_class_slots) and where the classes are kept (option read_em_lds_classes). */
typedef struct {
    uint32_t n_species;         /* must equal the db's */
    const uint64_t *cand_off;   /* [S+1] */
    const uint32_t *cand_hap;   /* [C] species-local haplotype index (any order, no repeats) */
    const uint64_t *cand_len;   /* [C] graph bases of the candidate, G */
    uint32_t max_iter;          /* >= 1 */
    double tol;                 /* >= 0, finite */
} pantax_hip_read_em_set;
int pantax_hip_strain_read_em(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_em_set *cand,
                              uint64_t *species_out /*[S][2][3]: counted, unexplained*/, uint64_t *cls_off_out /*[S+1]*/,
                              uint64_t cls_cap /* classes cls_mask_out and cls_q_out hold */, uint64_t *cls_mask_out, uint64_t *cls_q_out /*[][3]*/,
                              double *x_out /*[C]*/, uint32_t *iter_out /*[S]*/, int32_t *converged_out /*[S]*/, double *delta_out /*[S]*/);
/* host helper, no ctx and no GPU: the estimate above for one species.  mask / b [J] in ascending mask, len [K] in canonical order, K <= 64, every mask over
 * the K low bits; x_out [K].  The same arithmetic, compiled with contraction off: equal to the device bit for bit.  It follows the iteration as written also
 * for J = 0 (zeros after two iterations).  PANTAX_HIP_E_INVALID for a null argument, K > 64, max_iter = 0, a tol that is negative or not finite, a mask bit
 * at or above K. */
int pantax_hip_read_em(uint32_t K, uint64_t J, const uint64_t *mask, const uint64_t *b, const uint64_t *len, uint32_t max_iter, double tol, double *x_out,
                       uint32_t *n_iter_out, int32_t *converged_out, double *delta_out);

/* ---- mosaic reads (the --strain-mosaic report; not a stage of the reference): which candidate strains a read that fits no single candidate switches
 * between, and where.  Inputs, state rules, PANTAX_HIP_E_INVALID cases, a counted read, Q(r) = (1, n_steps, span), K_s and the rule "argmax of w, ties to
 * the smallest species-local haplotype index" are those of pantax_hip_strain_read_support above.  For a counted read r of a species with 1 <= K_s <= 64:
 *   v_1 .. v_n = its steps in walk order (a node visited twice is two steps);  M(v) = the species' candidates whose walk visits v.
 *   r is FOREIGN if some M(v_i) is empty: it is not cut and gives no segments, switches or junctions; foreign_steps sums its steps with empty M.
 *   Otherwise r is cut greedily from the left: a segment grows while the intersection of its steps' M stays non-empty, the step that would empty it opens
 *   the next segment.  k(r) = the number of segments, A_j = the intersection over segment j, and segment j is ASSIGNED the argmax of w over A_j.  k(r) is
 *   the smallest number of stretches that each fit one candidate (a stretch of a compatible stretch is compatible), the same in either walk direction, and
 *   k(r) = 1 exactly when C(r) is not empty.  A read of k >= 2 is MOSAIC.  Two consecutive segments never share their assigned strain.
 * Outputs, u64 unless stated, exact integers independent of any order:
 *   species_out [S][6][3] = the sums of Q over { counted, compatible (k = 1), mosaic1 (k = 2), mosaic2 (k = 3), mosaic3plus (k >= 4), foreign }; a species
 *     of K_s = 0 or K_s > 64 gets counted only (a candidate word is one u64, as in pantax_hip_strain_read_em);
 *   extra_out [S][3] = { n_segments = sum of k over the mosaic reads, n_breaks = sum of k - 1, foreign_steps };
 *   hap_out [C][2] in the order of cand_hap = { the segments of mosaic reads assigned to the candidate, the steps in those segments };
 *   pair_out[pair_off[s] + a * K_s + b] = the breaks whose left segment is assigned to the candidate at position a of the species' list and whose right
 *     segment to the one at position b: in walk order, NOT mirrored, zero diagonal.  pair_off_out [S+1] and pair_cap as in read support;
 *   junctions: a break between the last step a of its left segment and the first step b of its right segment is the junction (species, node_a, node_b),
 *     nodes as species-local indices.  junction_out [junction_cap][3] (u32) and junction_count_out [junction_cap] hold the DISTINCT junctions with their
 *     numbers of breaks in ascending (species, node_a, node_b); *n_junctions_out = how many; *n_breaks_total_out = the breaks of the call, always
 *     written.  junction_cap = 0: junctions are not collected (the two arrays may be null, *n_junctions_out = 0).  junction_cap > 0 but below the breaks
 *     of the call: PANTAX_HIP_E_LIMIT with *n_breaks_total_out and pair_off_out written and nothing else touched; size by it and repeat.
 *     The greedy cut puts a break as LATE in walk order as it can, so reads of the two strands that cross one recombination point report junctions that
 *     bracket the point from either side, not one junction.
 * For every species of 1 <= K_s <= 64: counted = compatible + mosaic1 + mosaic2 + mosaic3plus + foreign (all three numbers); compatible = counted -
 * unexplained and mosaic* + foreign = unexplained of pantax_hip_strain_read_support on the same candidates; sum of hap_out.segments = n_segments; sum of
 * hap_out.steps = the n_steps of the three mosaic classes; sum of the species' pair block = n_breaks = the sum of its junction counts = n_segments - the
 * n_reads of the three mosaic classes; K_s = 1 gives no mosaic read. */
#define PANTAX_HIP_MOSAIC_CLASSES 6
int pantax_hip_strain_mosaic(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand,
                             uint64_t *species_out /*[S][6][3]*/, uint64_t *extra_out /*[S][3]*/, uint64_t *hap_out /*[C][2]*/,
                             uint64_t *pair_off_out /*[S+1]*/, uint64_t pair_cap /* entries pair_out holds */, uint64_t *pair_out,
                             uint64_t junction_cap /* junctions the two arrays hold; 0 = do not collect */, uint32_t *junction_out /*[][3]*/,
                             uint64_t *junction_count_out, uint64_t *n_junctions_out, uint64_t *n_breaks_total_out);
/* host helper, no ctx and no GPU: the greedy cut above for ONE walk.  masks [n]: bit p of masks[i] = the candidate at position p walks step i (bits at and
 * above K are ignored); w, hap [K] = weight and species-local haplotype index of position p (no repeats), 1 <= K <= 64.  *k_out = k (0 for a foreign or an
 * empty walk), *foreign_steps_out = the steps with an empty mask; segment j < min(k, cap) is the steps [seg_end_out[j-1], seg_end_out[j]) (seg_end_out[-1]
 * = 0) and is assigned position seg_pos_out[j].  PANTAX_HIP_E_LIMIT when k > cap (k, foreign_steps and the first cap segments are written);
 * PANTAX_HIP_E_INVALID for a null argument, K = 0, K > 64 or a haplotype twice. */
int pantax_hip_mosaic_walk(uint64_t n, const uint64_t *masks, uint32_t K, const double *w, const uint32_t *hap, uint64_t *seg_end_out,
                           uint32_t *seg_pos_out, uint64_t cap, uint64_t *k_out, uint64_t *foreign_steps_out);
/* host helper, no ctx and no GPU: the junctions a report prints -- idx_out [min(n, top)] = the indices of the first `top` of n junctions in the order
 * count descending, then node_a, then node_b ascending; *n_out = how many.  PANTAX_HIP_E_INVALID for a null argument with n > 0. */
int pantax_hip_mosaic_top(uint64_t n, const uint32_t *node_a, const uint32_t *node_b, const uint64_t *count, uint64_t top, uint64_t *idx_out,
                          uint64_t *n_out);

/* ---- per-strain coverage track (the --strain-coverage report; not a stage of the reference): coverage along the genome of selected haplotypes,
 * in windows of W bases, from what pantax_hip_node_coverage leaves on the device.  For a species s, a species-local haplotype h and W >= 1:
 *   v_0 .. v_{n-1} = the walk of h as global node indices (a node visited twice counts at both visits);
 *   o_i = sum_{j<i} node_len[v_j] (u64) = the path offset of step i;  G_h = sum_i node_len[v_i];
 *   step i belongs to window w_i = o_i / W: the window that holds the node's FIRST base (the model's walks carry no orientation,
 *     profile.rs:1333-1342, types.rs:51-55: a node cannot be cut at a window border, and it is not);
 *   h has n_win(h) = ceil(G_h / W) windows (none when G_h = 0); window w carries
 *     n_nodes (u32) = the number of its steps,            len (u64)   = sum of node_len[v_i] over them,
 *     covered (u64) = sum of node_base_cov[v_i],          bases (u64) = sum of bases_per_node[v_i]   (both as pantax_hip_node_coverage hands them out);
 *   a window in which no node starts (a node longer than W runs through it) holds four zeros.
 * Integers only: results are exact and independent of any order.
 * win_off_out [C+1] = the prefix of n_win in the order of sel_hap; it is ALWAYS written.  When its total exceeds `cap` (the windows the four arrays
 * hold) the call returns PANTAX_HIP_E_LIMIT with win_off_out filled and nothing else touched: a caller sizes its arrays by calling once with cap = 0.
 * Requires that the db holds the coverage result of a pantax_hip_node_coverage call (a pantax_hip_strain_profile behind it changes nothing).  A resident
 * step (pantax_hip_profile_step / _enqueue) counts the covered bases inside its own passes and may already have zeroed the coverage arena: behind one,
 * and before any coverage pass, the call returns PANTAX_HIP_E_STATE.  PANTAX_HIP_E_INVALID: W = 0, a haplotype index out of range, a haplotype twice
 * within a species, n_species different from the db's.  An empty selection, or a species without selected haplotypes, is fine. */
typedef struct {
    uint32_t n_species;       /* must equal the db's */
    const uint64_t *sel_off;  /* [S+1] species s owns the selection entries [sel_off[s], sel_off[s+1]) */
    const uint32_t *sel_hap;  /* [C] species-local haplotype index, any order, no repeats within a species */
    uint64_t window;          /* W >= 1 */
} pantax_hip_cov_track_set;
int pantax_hip_strain_cov_track(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_cov_track_set *sel,
                                uint64_t *win_off_out /*[C+1]*/, uint64_t cap /* windows the four arrays hold */,
                                uint32_t *n_nodes_out, uint64_t *len_out, uint64_t *covered_out, uint64_t *bases_out);

/* ---- own-node windows and the replication index of a strain (the --strain-growth report; not a stage of the reference): the strain's OWN depth along
 * its genome, and the slope of that depth between the deepest and the shallowest part of it (the order-free formulation of iRep: sort the windows by depth,
 * trim, fit a line to log2 depth against rank).  Selection, walk, o_i, G_h, w_i = o_i / W and n_win(h) as for pantax_hip_strain_cov_track above.  Step i of
 * selection entry c is OWN when, among the selected haplotypes of its species, only c's haplotype walks v_i (in a species with one selected haplotype every
 * step is own; a node the haplotype alone walks twice is own at both visits).  Window w carries
 *     n_own (u32)     = the number of its own steps,        len (u64)       = sum of node_len[v_i] over ALL its steps, as the track has it,
 *     len_own (u64)   = sum of node_len[v_i] over own steps,  bases_own (u64) = sum of bases_per_node[v_i] over own steps.
 * Integers only: results are exact and independent of any order.  win_off_out, `cap`, validation and state rules are those of pantax_hip_strain_cov_track
 * (pantax_hip_cov_track_set is the selection).  The option growth_route=walk (pantax_hip_set_option) takes every species' membership from its selected
 * walks, as evidence_route=walk does. */
int pantax_hip_strain_growth(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_cov_track_set *sel,
                             uint64_t *win_off_out /*[C+1]*/, uint64_t cap /* windows the four arrays hold */,
                             uint32_t *n_own_out, uint64_t *len_out, uint64_t *len_own_out, uint64_t *bases_own_out);
/* host helper, no ctx and no GPU: the fit over the n windows of ONE entry.
 *   1. a window is kept if len_own >= min_own; n_zero = the kept windows with bases_own = 0, which take no further part;
 *   2. the others are sorted ascending by depth bases_own / len_own as an exact rational (128-bit cross products), ties by window index;
 *   3. median_depth = the lower median as f64 bases / len; windows outside [median / 8, median x 8] are dropped, n_f remain;
 *   4. floor(n_f x trim_permille / 1000) windows are trimmed from each end, n_fit remain;
 *   5. least squares of y_j = log2(bases_j / len_j) against x_j = (t_lo + j + 0.5) / n_f (t_lo = the windows trimmed from the low end), centred two-pass
 *      sums in ascending j, in f64: slope, intercept, r2; index = 2^slope = the ratio of the fitted depth between the two ends of the sorted range.
 * status: the first that applies of EMPTY (no window is left to fit: n_fit = 0), FEW_WINDOWS (n_fit < min_windows), LOW_DEPTH (median_depth < min_depth),
 * FLAT (all y equal: slope 0, r2 0, index 1), else OK.  With EMPTY slope, intercept and r2 are 0 and index is 1; median_depth is 0 when no window
 * carries bases.  The report's min_windows and min_depth are the two constants below: choices of this contract, not measurements.
 * PANTAX_HIP_E_INVALID: a null array with n > 0, a null `out`, trim_permille >= 500, min_own = 0. */
#define PANTAX_HIP_GROWTH_OK 0
#define PANTAX_HIP_GROWTH_EMPTY 1
#define PANTAX_HIP_GROWTH_FEW_WINDOWS 2
#define PANTAX_HIP_GROWTH_LOW_DEPTH 3
#define PANTAX_HIP_GROWTH_FLAT 4
#define PANTAX_HIP_GROWTH_MIN_WINDOWS 20
#define PANTAX_HIP_GROWTH_MIN_DEPTH 5.0
typedef struct {
    uint64_t n_kept, n_zero, n_f, n_fit, own_len;   /* own_len = sum of len_own over the kept windows */
    double median_depth, slope, intercept, r2, index;
    int32_t status;                                  /* PANTAX_HIP_GROWTH_* */
    int32_t pad;
} pantax_hip_growth_fit_result;
int pantax_hip_growth_fit(uint64_t n, const uint64_t *len_own, const uint64_t *bases_own, uint64_t min_own, uint64_t trim_permille, uint64_t min_windows,
                          double min_depth, pantax_hip_growth_fit_result *out);
const char *pantax_hip_growth_status_name(int32_t status);   /* "ok", "empty", "few_windows", "low_depth", "flat"; "?" otherwise */

/* ---- absent and amplified segments along a strain (the --strain-segments report; not a stage of the reference): the exact stretches of the genome of
 * selected haplotypes that the sample does not cover at all, and those far deeper than a given depth, from what pantax_hip_node_coverage leaves on the
 * device.  Walk, o_i and G_h as for the coverage track above.  With min_len >= 1 and one peak_depth[c] <= 2^31 per selection entry c (0: no peak class
 * for that entry), step i of entry c has the class
 *     1 (PANTAX_HIP_SEGMENT_GAP)   if node_base_cov[v_i] == 0;
 *     2 (PANTAX_HIP_SEGMENT_PEAK)  else if peak_depth[c] > 0 and bases_per_node[v_i] >= peak_depth[c] * node_len[v_i] (u64 product);
 *     0                            else.
 * A segment is a maximal run [i, j) of consecutive steps of one walk with the same non-zero class (a gap directly followed by a peak is two segments);
 * it carries class (u8), step = i (u64, walk-local), n_steps = j - i (u32), start = o_i, len = sum of node_len, bases = sum of bases_per_node (u64).
 * Per selection entry, always written: hap_len [C] = G_h; and for the classes k = gap, peak over ALL runs of the class whatever their length,
 * n_runs [2C], run_len [2C] (the sum of len) and run_max [2C] (the longest len), entry c's gap at 2c and its peak at 2c + 1.
 * seg_off_out [C+1] = the prefix, in the order of sel_hap, of the number of segments with len >= min_len; it is ALWAYS written.  The six segment arrays
 * hold exactly those segments, per entry in ascending start.  The cap protocol is that of pantax_hip_strain_cov_track: with more than `cap` segments the
 * call returns PANTAX_HIP_E_LIMIT with seg_off_out and the per-entry summaries filled and the segment arrays untouched; a caller sizes them by calling
 * once with cap = 0.  Integers only: results are exact and independent of any order.
 * Validation and state rules of pantax_hip_strain_cov_track.  PANTAX_HIP_E_INVALID also for min_len = 0 and a peak_depth above 2^31. */
#define PANTAX_HIP_SEGMENT_GAP 1
#define PANTAX_HIP_SEGMENT_PEAK 2
typedef struct {
    uint32_t n_species;          /* must equal the db's */
    const uint64_t *sel_off;     /* [S+1] */
    const uint32_t *sel_hap;     /* [C] species-local haplotype index, any order, no repeats within a species */
    const uint64_t *peak_depth;  /* [C] 0 = no peak class for the entry; at most 2^31 */
    uint64_t min_len;            /* >= 1: segments shorter than this are counted in the summaries only */
} pantax_hip_segment_set;
int pantax_hip_strain_segments(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_segment_set *sel,
                               uint64_t *seg_off_out /*[C+1]*/, uint64_t cap /* segments the six arrays hold */,
                               uint64_t *hap_len_out /*[C]*/, uint64_t *n_runs_out /*[2C]*/, uint64_t *run_len_out /*[2C]*/, uint64_t *run_max_out /*[2C]*/,
                               uint8_t *seg_class_out, uint64_t *seg_step_out, uint32_t *seg_n_steps_out, uint64_t *seg_start_out, uint64_t *seg_len_out,
                               uint64_t *seg_bases_out);
/* host helper, no ctx and no GPU: chains of the segments of ONE haplotype, given in ascending start (disjoint: start[i] >= start[i-1] + len[i-1]; class 1
 * or 2).  Per class separately, ignoring the segments of the other class: consecutive segments with start_next - (start_prev + len_prev) <= bridge form
 * one chain (a stretch of at most `bridge` bases decides nothing, in either direction; a peak between two gaps does not break their chain).  Chain m with
 * span >= min_span is returned, in ascending start: chain_class [n], chain_first / chain_last [n] = the index of its first and last member in the input,
 * chain_q [n][PANTAX_HIP_SEGMENT_CHAIN_N] = { start, end, span = end - start, in_class = the sum of its members' len, n_segments, n_steps, bases }.  The
 * output arrays hold n entries (there are at most n chains); *n_chains_out = how many were written.  PANTAX_HIP_E_INVALID: a null argument with n > 0, a
 * class other than 1 or 2, segments that are not ascending and disjoint. */
#define PANTAX_HIP_SEGMENT_CHAIN_N 7
int pantax_hip_segment_chain(uint64_t n, const uint8_t *seg_class, const uint64_t *seg_start, const uint64_t *seg_len, const uint32_t *seg_n_steps,
                             const uint64_t *seg_bases, uint64_t bridge, uint64_t min_span, uint64_t *n_chains_out, uint8_t *chain_class,
                             uint64_t *chain_first, uint64_t *chain_last, uint64_t *chain_q);

/* ---- per-strain node evidence (the --strain-evidence report; not a stage of the reference): what in the sample separates a selected haplotype from
 * the other selected haplotypes of its species, and the coverage of the species that no selected haplotype explains, from what pantax_hip_node_coverage
 * leaves on the device.  For a species s of the db, Sel_s = its selected species-local haplotype indices, K_s = |Sel_s|.  Every node v of s is counted
 * once, whether or not any walk visits it:
 *   M(v) = { h in Sel_s : the walk of h visits v at least once } -- node-level membership, the 0/1 matrix of the LP (profile.rs:1333-1342): a node
 *          walked twice by h counts once (the coverage track above counts visits);   m(v) = |M(v)|;
 *   Q(v) = (1, node_len[v], node_base_cov[v], bases_per_node[v]), the last two as pantax_hip_node_coverage hands them out; all four u64.
 * Every output is a sum of Q(v), its four numbers in the order { n_nodes, len, covered, bases }:
 *   per selection entry c (haplotype h of species s):   all[c] = sum over v with h in M(v);   private[c] = sum over v with M(v) = {h};
 *   per species s:   total[s] = sum over every node;   orphan[s] = sum over m(v) = 0;   core[s] = sum over m(v) = K_s when K_s >= 1, four zeros when K_s = 0.
 * Integers only: results are exact and independent of any order.
 * hap_out [C][2][4] = { all, private } of every selection entry in the order of sel_hap; species_out [S][3][4] = { total, orphan, core } of every species.
 * The caller knows both sizes: there is no sizing call.  An empty selection, or a species without selected haplotypes, is fine: total and orphan are
 * written for every species.  State rules of pantax_hip_strain_cov_track: the db must hold the coverage result of a pantax_hip_node_coverage call (a
 * pantax_hip_strain_profile behind it changes nothing); behind a resident step (pantax_hip_profile_step / _enqueue), and before any coverage pass, the
 * call returns PANTAX_HIP_E_STATE and says why.  PANTAX_HIP_E_INVALID: n_species different from the db's, a haplotype index out of range, a haplotype
 * twice within a species. */
typedef struct {
    uint32_t n_species;       /* must equal the db's */
    const uint64_t *sel_off;  /* [S+1] species s owns the selection entries [sel_off[s], sel_off[s+1]) */
    const uint32_t *sel_hap;  /* [C] species-local haplotype index, any order, no repeats within a species */
} pantax_hip_evidence_set;
int pantax_hip_strain_evidence(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel,
                               uint64_t *hap_out /*[C][2][4]: all, private*/, uint64_t *species_out /*[S][3][4]: total, orphan, core*/);

/* ---- per-strain depth distribution (the --strain-depth report; not a stage of the reference): every depth of the reports above is a mean, bases / len
 * over a set of nodes, and a mean is what fails where a mobile element at 400x lifts a strain whose other private nodes sit at 3x, or where a strain
 * called from its core genome has a private genome that is mostly empty.  This call hands out the DISTRIBUTION of depth over the same sets of nodes.
 * Selection, Sel_s, K_s, M(v), m(v), the inputs (node_len; bases_per_node as pantax_hip_node_coverage leaves it) and the state rules are exactly those
 * of pantax_hip_strain_evidence, whose selection type it takes: every node of a species is counted once, membership is node-level (a node walked twice
 * counts once); PANTAX_HIP_E_STATE behind a resident step and before any coverage pass; PANTAX_HIP_E_INVALID for an n_species different from the db's, a
 * haplotype index out of range, a haplotype twice within a species.  On an error the output arrays are left as given.
 *   depth of a node   d(v) = bases_per_node[v] / node_len[v] in u64 integer division; d(v) = 0 when node_len[v] = 0.
 *   bin of a depth    PANTAX_HIP_DEPTH_BINS = 96 of them.  d < 32: bin = d (exact).  Otherwise, with e = floor(log2 d),
 *                     bin = min(95, 32 + 4 (e - 5) + ((d >> (e - 2)) & 3)): four bins per octave from 2^5, and bin 95 also takes everything from 2^21 up.
 *   bounds of a bin   lo(b) = b for b < 32, lo(b) = (4 + (b - 32) % 4) << (3 + (b - 32) / 4) for b >= 32; hi(b) = lo(b + 1), hi(95) = 2^64 - 1.  A depth d
 *                     of bin b has lo(b) <= d < hi(b) (bin 95: d <= hi, the largest u64).
 * Every output is a histogram [96][2]: per bin the u64 sums of (1, node_len[v]), in the order { n_nodes, len }, over the nodes of a class whose depth
 * falls into the bin:
 *   hap_out [C][2][96][2]      per selection entry, in the order of sel_hap: class all (h in M(v)), then private (M(v) = {h});
 *   species_out [S][2][96][2]  per species: class total (every node), then orphan (m(v) = 0).  NULL: not computed.
 * Integers only: results are exact and independent of any order.  An empty selection, or a species with nothing selected, is fine: total and orphan
 * are still written for it.  Summed over its bins a histogram gives { n_nodes, len } of the same class of pantax_hip_strain_evidence.
 * The option depth_route=walk (pantax_hip_set_option) takes every species' membership from its selected walks, as evidence_route=walk does. */
#define PANTAX_HIP_DEPTH_BINS 96
int pantax_hip_strain_depth(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel,
                            uint64_t *hap_out /*[C][2][96][2]: all, private*/, uint64_t *species_out /*[S][2][96][2]: total, orphan; or NULL*/);
/* Host-only helpers of the histograms (no ctx, no GPU; the bin function is the one source text the kernel compiles):
 *   pantax_hip_depth_bin        the bin of a depth;
 *   pantax_hip_depth_bin_range  lo(bin) and hi(bin); PANTAX_HIP_E_INVALID for bin >= 96 or a null pointer;
 *   pantax_hip_depth_quantile   the length-weighted quantile of one histogram hist [96][2]: with T = the sum of len over the bins, the smallest bin whose
 *                               cumulative len is at least max(1, ceil(T per_mille / 1000)) -> *bin_out, return 0.  T = 0: there is none, the return value
 *                               is PANTAX_HIP_DEPTH_NONE and *bin_out is left alone.  per_mille > 1000 or a null pointer: PANTAX_HIP_E_INVALID. */
#define PANTAX_HIP_DEPTH_NONE 1
uint32_t pantax_hip_depth_bin(uint64_t d);
int pantax_hip_depth_bin_range(uint32_t bin, uint64_t *lo, uint64_t *hi);
int pantax_hip_depth_quantile(const uint64_t *hist /*[96][2]*/, uint32_t per_mille, uint32_t *bin_out);

/* ---- unreported-strain near misses (the --strain-near-miss report; not a stage of the reference): the evidence call's `orphan` is coverage on nodes
 * that no reported strain walks, "the sign of a strain that is in the sample and not in the table".  This call says which unreported haplotypes of the
 * db would explain it.  For a species s of the db:
 *   Sel_s  = the reported haplotypes, K_s = |Sel_s|;   Cand_s = the candidates, J_s = |Cand_s|.  Both hold species-local haplotype indices in any
 *            order; a haplotype may not repeat within Sel_s or within Cand_s, and no haplotype may be in both.
 * Every node v of s is counted once, whether or not any walk visits it:
 *   M(v) = { h in Sel_s : the walk of h visits v at least once },  m(v) = |M(v)| -- exactly the node-level membership of pantax_hip_strain_evidence
 *          (a node walked twice counts once);
 *   N(v) = { h in Cand_s : the walk of h visits v at least once }, n(v) = |N(v)|;
 *   Q(v) = (1, node_len[v], node_base_cov[v], bases_per_node[v]), the last two as pantax_hip_node_coverage leaves them; all four u64.
 * Every output is a sum of Q(v), its four numbers in the order { n_nodes, len, covered, bases }:
 *   per candidate entry c (haplotype h), cand_out [J][2][4] in the order of cand_hap:
 *     novel[c]     = sum over m(v) = 0 and h in N(v)   -- the nodes h walks that no reported strain walks;
 *     exclusive[c] = sum over m(v) = 0 and N(v) = {h}  -- the orphan nodes that, among the candidates, only h walks;
 *   per species s, species_out [S][3][4]:
 *     orphan[s]    = sum over m(v) = 0                 -- the evidence call's orphan, element for element;
 *     claimed[s]   = sum over m(v) = 0 and n(v) >= 1;
 *     contested[s] = sum over m(v) = 0 and n(v) >= 2.
 * Integers only: results are exact and independent of any order.  Identities: exclusive <= novel; claimed = contested + the sum of exclusive over the
 * species' candidates; contested <= claimed <= orphan; J_s = 1 gives novel = exclusive = claimed and contested = 0; novel[c] is at most the evidence
 * call's all of the same haplotype; with Sel_s empty every node of the species is an orphan.
 * The caller knows both sizes (J = cand_off[S]): there is no sizing call.  An empty Sel, an empty Cand, both empty, a species with neither: all fine,
 * orphan is always written.  State rules of pantax_hip_strain_evidence: PANTAX_HIP_E_STATE behind a resident step and before any coverage pass.
 * PANTAX_HIP_E_INVALID: n_species different from the db's, a haplotype index out of range, a haplotype twice within Sel_s or within Cand_s, a
 * haplotype in both.  On an error the output arrays are left as given.
 * The option near_miss_route=walk (pantax_hip_set_option) takes every species' membership from the walks of Sel_s ++ Cand_s, as evidence_route=walk
 * does; near_miss_words=N (1 .. 4) caps the candidate mask words a wave counts in one pass over its nodes (default 4: 256 candidates). */
typedef struct {
    uint32_t n_species;        /* must equal the db's */
    const uint64_t *sel_off;   /* [S+1] species s owns the reported entries [sel_off[s], sel_off[s+1]) */
    const uint32_t *sel_hap;   /* species-local haplotype index, any order, no repeats within a species */
    const uint64_t *cand_off;  /* [S+1] species s owns the candidate entries [cand_off[s], cand_off[s+1]) */
    const uint32_t *cand_hap;  /* [J] species-local haplotype index, any order, no repeats within a species, none of sel_hap's of the species */
} pantax_hip_near_miss_set;
int pantax_hip_strain_near_miss(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_near_miss_set *sel,
                                uint64_t *cand_out /*[J][2][4]: novel, exclusive*/, uint64_t *species_out /*[S][3][4]: orphan, claimed, contested*/);
/* Host-only helper (no ctx, no GPU): the order in which one species' candidates are reported.  cand_hap [n_cand] and cand_out [n_cand][2][4] are the
 * species' stretch of the call above.  rank_out [n_cand] receives candidate positions (0 .. n_cand - 1) ordered by novel.bases descending, then
 * novel.covered descending, then haplotype index ascending; candidates with novel.bases = 0 are left out; only the first `top` are kept (0 keeps
 * all); *n_out = the number written.  A null pointer among the four (whatever n_cand): PANTAX_HIP_E_INVALID, nothing written. */
int pantax_hip_near_miss_rank(uint32_t n_cand, const uint32_t *cand_hap, const uint64_t *cand_out /*[n_cand][2][4]*/, uint32_t top,
                              uint32_t *rank_out /*[n_cand]*/, uint32_t *n_out);

/* ---- read rescue (the --strain-rescue report; not a stage of the reference): for every read that fits no reported strain, whether a single unreported
 * candidate of the db walks all of its nodes, and which one.  Sel_s, Cand_s, K_s, J_s and the PANTAX_HIP_E_INVALID cases are those of
 * pantax_hip_strain_near_miss above; the state rule (reads binned against db, else PANTAX_HIP_E_STATE), a counted read and Q(r) = (1, n_steps, span) are
 * those of pantax_hip_strain_read_support.  On any error the outputs are left as given.
 * A species is OPEN when K_s + J_s <= 64 (K_s = 0 and J_s = 0 are both allowed); a wider species is SKIPPED: only `counted` is written for it.
 * For a counted read r of an open species with steps v_1 .. v_n in walk order (a node visited twice is two steps):
 *   M(v) = the members of Sel_s whose walk visits v,  N(v) = the same over Cand_s (containment over node sets, as everywhere else);
 *   C(r) = the intersection of M(v_i),  D(r) = the intersection of N(v_i).
 * Every counted read of an open species is exactly one of
 *   compatible  C(r) is not empty;
 *   foreign     some M(v_i) is empty (with K_s = 0: every counted read);
 *   mosaic      C(r) is empty and no M(v_i) is: the k >= 2 of pantax_hip_strain_mosaic.
 * Unexplained = foreign or mosaic.  An unexplained read is RESCUED when D(r) is not empty and also CONTESTED when |D(r)| >= 2.  A foreign read that is
 * not rescued is foreign_novel when some step has M(v_i) and N(v_i) both empty (a node nobody of either list walks), else foreign_patchwork (every node
 * is walked by a reported strain or a candidate, but no single haplotype walks them all).
 * Outputs, all u64, exact integers independent of any order, Q in the order { n_reads, n_steps, span }:
 *   species_out [S][9][3] = the sums of Q over { counted, compatible, foreign, foreign_rescued, foreign_patchwork, foreign_novel, mosaic, mosaic_rescued,
 *     contested };
 *   step_out [S][3] = { foreign_steps = the steps with M empty, claimed_steps = those of them with N not empty, novel_steps = those with N empty };
 *   cand_out [J][3][3] in the order of cand_hap = { rescued[c] = the sum of Q over unexplained reads with c in D(r), alone[c] = over D(r) = {c},
 *     from_foreign[c] = over foreign reads with c in D(r) };
 *   cand_steps_out [J] = the steps with M(v) empty and c in N(v).
 * For every open species: counted = compatible + foreign + mosaic; foreign = foreign_rescued + foreign_patchwork + foreign_novel; the sum of alone over
 * the species' candidates + contested = foreign_rescued + mosaic_rescued (all three numbers of Q); alone <= rescued and from_foreign <= rescued;
 * foreign_steps = claimed_steps + novel_steps; the sum of cand_steps >= claimed_steps, equal when J_s = 1; J_s = 0 gives foreign = foreign_novel and no
 * rescue; novel_steps > 0 exactly when foreign_novel.n_reads > 0.  On the same Sel: counted, compatible, foreign and foreign_steps are those of
 * pantax_hip_strain_mosaic with cand = Sel (whatever the weights), mosaic = its mosaic1 + mosaic2 + mosaic3plus; compatible + foreign_rescued +
 * mosaic_rescued = counted - unexplained of pantax_hip_strain_read_support over the list Sel ++ Cand.
 * The option read_strain_route=walk takes every species' membership from the walks of Sel_s ++ Cand_s. */
#define PANTAX_HIP_RESCUE_CLASSES 9
int pantax_hip_strain_read_rescue(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_near_miss_set *sel,
                                  uint64_t *species_out /*[S][9][3]*/, uint64_t *step_out /*[S][3]*/, uint64_t *cand_out /*[J][3][3]*/,
                                  uint64_t *cand_steps_out /*[J]*/);
/* host helper, no ctx and no GPU: the classes above for ONE walk of n steps.  Bit p of sel_masks[i] = the member at position p of Sel walks step i, bit p
 * of cand_masks[i] the same over Cand; bits at and above K or J are ignored.  *class_out = one of the six values below, *d_out = D(r) (bit p = position
 * p of Cand), steps_out [3] = { foreign_steps, claimed_steps, novel_steps } of the walk.  PANTAX_HIP_E_INVALID for a null argument, n = 0 or K + J > 64. */
enum {
    PANTAX_HIP_RESCUE_COMPATIBLE = 0,
    PANTAX_HIP_RESCUE_FOREIGN_RESCUED = 1,
    PANTAX_HIP_RESCUE_FOREIGN_PATCHWORK = 2,
    PANTAX_HIP_RESCUE_FOREIGN_NOVEL = 3,
    PANTAX_HIP_RESCUE_MOSAIC_RESCUED = 4,
    PANTAX_HIP_RESCUE_MOSAIC_UNRESCUED = 5
};
int pantax_hip_rescue_walk(uint64_t n, const uint64_t *sel_masks, const uint64_t *cand_masks, uint32_t K, uint32_t J, uint32_t *class_out, uint64_t *d_out,
                           uint64_t *steps_out /*[3]*/);
/* host helper, no ctx and no GPU: the order in which one species' candidates are printed.  cand_hap [n_cand] and cand_out [n_cand][3][3] are the species'
 * stretch of pantax_hip_strain_read_rescue.  rank_out [n_cand] receives candidate positions ordered by rescued.span descending, then rescued.n_reads
 * descending, then haplotype index ascending; candidates with rescued.n_reads = 0 are left out; only the first `top` are kept (0 keeps all); *n_out =
 * the number written.  A null pointer among the four (whatever n_cand): PANTAX_HIP_E_INVALID, nothing written. */
int pantax_hip_rescue_rank(uint32_t n_cand, const uint32_t *cand_hap, const uint64_t *cand_out /*[n_cand][3][3]*/, uint32_t top,
                           uint32_t *rank_out /*[n_cand]*/, uint32_t *n_out);

/* ---- link support (the --strain-links report; not a stage of the reference): which adjacencies of a reported strain the reads cross.  Every other
 * report treats a read and a strain as sets of nodes; this one looks at which node follows which.  The selection is a pantax_hip_read_strain_set: Sel_s
 * with K_s entries per species, the weights unused (a null cand_w is fine).  State rules of pantax_hip_strain_read_support (reads binned against db, else
 * PANTAX_HIP_E_STATE) and, for the coverage result, of pantax_hip_strain_segments (PANTAX_HIP_E_STATE behind a resident step and before any coverage
 * pass); PANTAX_HIP_E_INVALID cases of pantax_hip_read_strains.  On any error the outputs are left as given.
 * A species is OPEN when K_s <= 64: a link mask is one u64, bit p = position p of the species' list (the caller's order).  A wider one is SKIPPED.
 *   Links.  Entry c at position p of species s has the walk w_0 .. w_{n-1}; position i in [0, n-1) carries the link e_i = {w_i, w_{i+1}}, an UNORDERED pair
 *   of species-local nodes (walks carry no orientation; {u, u} is a link).  L(e) = the list positions whose walk has e at some position.
 *   Crossings.  A counted read with steps v_1 .. v_n in walk order (repeats count) makes n - 1 crossings {v_i, v_{i+1}}; support[e] = the crossings equal
 *   to e over the species' counted reads.  With M(v) as in pantax_hip_strain_mosaic a crossing is exactly one of
 *     known    L is not empty;
 *     skip     not known, and M(v_i) and M(v_{i+1}) meet: a reported strain walks both nodes, never one after the other;
 *     switch   not known, both M non-empty, and the two are disjoint;
 *     foreign  an M is empty (K_s = 0: every crossing).
 *   Position classes.  With bases[] = bases_per_node of the coverage pass, position i of entry c is exactly one of
 *     crossed  support[e_i] > 0;
 *     broken   not crossed, bases[w_i] > 0 and bases[w_{i+1}] > 0: reads reach both sides and none goes across;
 *     open     the rest;
 *   and it is also PRIVATE when L(e_i) is the single bit p.
 * Outputs, u64 unless stated, exact integers independent of any order:
 *   species_out [S][6] = { counted_reads, crossings, known, skip, switch, foreign }; a skipped species gets the first two only;
 *   link_out [S][4] = { distinct links, distinct links crossed, core links (L = all K_s bits), core links crossed };
 *   hap_out [C][8] in the order of cand_hap = { links, crossed, open, broken, private, private_crossed, private_broken, support = the sum of
 *     support[e_i] over the positions }; an entry of a skipped species gets zeros;
 *   break records, one per broken position, per entry in ascending step, under the cap protocol of pantax_hip_strain_segments: brk_off_out [C+1] is
 *     ALWAYS written; more than `cap` records: PANTAX_HIP_E_LIMIT with brk_off_out, species_out, link_out and hap_out filled and the record arrays
 *     untouched.  brk_step (i), brk_start (o_{i+1}, the junction in path coordinates, o as in the coverage track), brk_node_a / brk_node_b (u32: w_i and
 *     w_{i+1}, in walk order, species-local), brk_flank (min(bases[w_i] / node_len[w_i], bases[w_{i+1}] / node_len[w_{i+1}]), integer division; a node of
 *     length 0 counts as depth 0), brk_mask (L(e_i)).
 * For every open species: crossings = known + skip + switch + foreign = counted.n_steps - counted.n_reads of pantax_hip_strain_read_support on the same
 * selection; known = the sum of support over the distinct links; per entry links = (steps of the walk) - 1 = crossed + open + broken, private_* <= its
 * class, brk_off[c+1] - brk_off[c] = broken[c]; K_s = 1 gives private = links, switch = 0 and core = distinct.
 * The option read_strain_route=walk takes every species' membership from the walks of Sel_s. */
#define PANTAX_HIP_LINK_SPECIES_N 6
#define PANTAX_HIP_LINK_HAP_N 8
int pantax_hip_strain_links(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *sel,
                            uint64_t *species_out /*[S][6]*/, uint64_t *link_out /*[S][4]*/, uint64_t *hap_out /*[C][8]*/, uint64_t *brk_off_out /*[C+1]*/,
                            uint64_t cap /* records the six arrays hold */, uint64_t *brk_step_out, uint64_t *brk_start_out, uint32_t *brk_node_a_out,
                            uint32_t *brk_node_b_out, uint64_t *brk_flank_out, uint64_t *brk_mask_out);
/* host helper, no ctx and no GPU: the classes above for the crossings of ONE walk of n steps.  Bit p of masks[i] = the member at position p of Sel walks
 * step i (bits at and above K are ignored); known[i] != 0: the crossing {step i, step i+1} is a link of some member (known may be null when n = 1).
 * out [4] = { known, skip, switch, foreign }.  PANTAX_HIP_E_INVALID for a null argument, n = 0 or K > 64. */
int pantax_hip_link_crossings(uint64_t n, const uint64_t *masks /*[n]*/, const uint8_t *known /*[n-1]*/, uint32_t K, uint64_t *out /*[4]*/);
/* host helper, no ctx and no GPU: the breaks a report prints -- idx_out [min(n, top)] = the indices of the first `top` (0 keeps all) of n breaks in the
 * order flank descending, then start ascending (then index ascending); *n_out = how many.  PANTAX_HIP_E_INVALID for a null idx_out / n_out, or a null
 * flank / start with n > 0. */
int pantax_hip_link_top(uint64_t n, const uint64_t *flank, const uint64_t *start, uint64_t top, uint64_t *idx_out, uint64_t *n_out);

/* ---- rarefaction of the strain fit (the --strain-rarefy report; not a stage of the reference): would a strain still be there with half the reads?  Every
 * other diagnostic is conditioned on the depth the sample has; the bootstrap redraws the LP's rows (nodes) at that depth.  This call thins the READS -- one
 * read feeds several nodes, and the LP's rows move together when it goes -- and refits the LP of pantax_hip_strain_bootstrap on every nested subsample.
 *   The thinning rule.  With sm = splitmix64's output function as in the bootstrap, replicate b >= 1 and r = the read's index in the uploaded columns
 *   (the order of the outputs of pantax_hip_read_strains):  h = sm(sm(seed ^ sm(b)) + r),  depth(b, r) = min(63, leading zero bits of h).  Read r belongs
 *   to level l of replicate b iff depth(b, r) >= l: level 0 is every read, level l keeps a read with probability 2^-l, and the levels of one replicate are
 *   nested.  pantax_hip_rarefy_depth is the rule as a host helper.
 *   bases_l[v] of a level = bases_per_node of pantax_hip_node_coverage over the level's reads alone: the counted reads (binned to a species of the db, no
 *   drop flag), the aligned length of every step as in get_node_abundances, only the first occurrence of a node in a read, nothing from a read that
 *   aborts there.  Exact integers.
 *   Entries.  E = 1 + n_replicates x n_levels.  Entry 0 is the full sample: its rows come from the bases_per_node the coverage pass left on the device, and
 *   its x, obj, rows and status are the bits of pantax_hip_strain_bootstrap with n_replicates = 0 on the same selection.  Entry 1 + (b - 1) n_levels + (l - 1)
 *   is level l in 1 .. n_levels of replicate b in 1 .. n_replicates: the LP of the bootstrap's contract on bases_l -- rows a_v = bases_l[v] / len > 0 with a
 *   non-empty mask, the box 1.05 max a of the entry's own rows, no column pinned.
 * Outputs, entry-major:  x_out [E][C];  obj_out [E][S] (a sum over the rows);  rows_out [E][S];  status_out [E][S] as in the bootstrap: 0 solved, 1 nothing
 * to solve, PANTAX_HIP_E_LIMIT for K_s > 64 (the other species are served), PANTAX_HIP_E_SOLVER for that LP alone;  reads_out [E][S][2] = { counted reads
 * of the species in the entry's level, bases they added }, entry 0's from the first pass over the reads;  member_out [E][C][2] = { n_member, n_only } of
 * the selected strain in the entry's LP as pantax_hip_strain_dropout defines them for its entry 0: the rows with its bit, the rows with mask == 1 << k.
 * Only the species with 1 <= K_s <= 64 are thinned: the others get zeros in reads_out.
 * State rules of pantax_hip_strain_links: resident reads binned against this db and a coverage result of pantax_hip_node_coverage, PANTAX_HIP_E_STATE
 * otherwise.  PANTAX_HIP_E_INVALID for n_levels outside 1 .. 16, n_replicates = 0 and the argument errors of pantax_hip_strain_evidence.  On an error the
 * outputs are left as given.  Determinism: the same inputs give the same bits, whatever the number of levels a pass over the reads serves (option
 * rarefy_levels_max, 0 = from the free device memory), the membership route (option rarefy_route=walk) and the position of a species in the db. */
typedef struct {
    uint32_t n_species;       /* must equal the db's */
    const uint64_t *sel_off;  /* [S+1] as pantax_hip_evidence_set */
    const uint32_t *sel_hap;  /* [C] species-local haplotype index, any order, no repeats within a species */
    uint64_t seed;
    uint32_t n_levels;        /* the thinned levels 1 .. n_levels; 1 .. 16 */
    uint32_t n_replicates;    /* >= 1 */
} pantax_hip_rarefy_set;
int pantax_hip_strain_rarefy(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_rarefy_set *sel, double *x_out /*[E][C]*/,
                             double *obj_out /*[E][S]*/, uint64_t *rows_out /*[E][S]*/, int32_t *status_out /*[E][S]*/, uint64_t *reads_out /*[E][S][2]*/,
                             uint64_t *member_out /*[E][C][2]*/);
/* the test seam of the pass over the reads: bases_l of ONE level (0 .. 63; level 0 and replicate 0 are allowed) over every species of the db, bases_out [V].
 * State rules as above. */
int pantax_hip_rarefy_node_bases(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, uint64_t seed, uint32_t replicate, uint32_t level,
                                 uint64_t *bases_out /*[V]*/);
/* host helper, no ctx and no GPU: depth(replicate, read) of the rule above */
uint32_t pantax_hip_rarefy_depth(uint64_t seed, uint32_t replicate, uint64_t read);

/* ---- fragment support (the --strain-fragments report; not a stage of the reference): read pairs as the unit of strain compatibility.  The read passes
 * above take every alignment record as an island; a paired-end fragment of 300 to 600 bases reaches private nodes that neither 150-base mate reaches alone.
 * Three calls: the fragment key of a read id (host only), the mates of every read from the keys (device: sort and one pass), and the fragment pass over
 * the resident reads.
 *
 * Key.  An id of len >= 3 bytes whose last two bytes are "/1" or "/2" has the stem id[0 .. len - 2) and the tag 1 or 2; every other id is its own stem and
 * has the tag 0.  key = the id hash of pantax_hip_gaf_ids (FNV-1a-64 and its avalanche) over the stem bytes: for tag 0 it is the tokenizers' id_hash.
 * PANTAX_HIP_E_INVALID for a null argument.  No ctx and no GPU. */
int pantax_hip_fragment_key(const char *id, uint64_t len, uint64_t *key_out, uint8_t *tag_out);
/* Mates.  Reads i != j are mates iff key[i] == key[j], no third read has that key, and their tags are {1, 2} in either order or both 0.  For mates
 * mate_out[i] = j and mate_out[j] = i; a key seen once gives PANTAX_HIP_MATE_NONE; every read of a key seen three times or more, or seen twice with any
 * other tag pair, gives PANTAX_HIP_MATE_AMBIGUOUS.  counts_out [4] = { pairs, reads without a mate, ambiguous reads, keys seen three times or more }.
 * n >= 2^32 - 2: PANTAX_HIP_E_LIMIT; a tag above 2 or a null argument: PANTAX_HIP_E_INVALID; n = 0 is fine.  Integers only: the result is a function of
 * the inputs alone. */
#define PANTAX_HIP_MATE_NONE      0xFFFFFFFFu
#define PANTAX_HIP_MATE_AMBIGUOUS 0xFFFFFFFEu
int pantax_hip_fragment_mates(pantax_hip_ctx *ctx, uint64_t n, const uint64_t *key /*[n] host*/, const uint8_t *tag /*[n] host*/,
                              uint32_t *mate_out /*[n] host*/, uint64_t *counts_out /*[4]: pairs, none, ambiguous reads, keys seen >= 3 times*/);
/* The fragment pass.  Inputs, a counted read, N(r), C(r), the weights, the assigned strain (argmax of w, ties to the smallest species-local haplotype
 * index) and the state rule (reads binned against db, else PANTAX_HIP_E_STATE) are those of pantax_hip_read_strains; Q(r) = (1, n_steps, span) is that of
 * pantax_hip_strain_read_support, and the numbers of a fragment {r, m} are (1, n_steps(r) + n_steps(m), span(r) + span(m)).  mate [R] names, in file
 * order, the mate of every read or one of the two codes.  Every counted read r of species s falls into exactly one class:
 *   mate[r] = NONE: single;   AMBIGUOUS: multi;   m counted and binned to s too: the fragment {r, m} is paired, accounted once;   m without a walk, dropped
 *   by its flags, unbinned or of another species: mate_elsewhere (whichever species share the db).
 * species_out [S][9][3], classes in the order { counted, paired, concordant, discordant, half, unexplained, single, multi, mate_elsewhere }, each
 * { n, n_steps, span }: counted sums Q over every counted read of s; single, multi and mate_elsewhere sum Q over their reads; paired and the four classes
 * behind it sum fragments.  For a species of 1 <= K_s <= 64 (served) every paired fragment has F = C(r) & C(m) and is exactly one of concordant (F not
 * empty), discordant (both C non-empty, F empty), half (exactly one C empty), unexplained (both empty).
 * hap_out [C][4][3] in the order of cand_hap, { compatible, unique, unique_by_pair, assigned }: the fragments with h in F; with F = {h}; with F = {h} while
 * neither |C(r)| = 1 nor |C(m)| = 1 (what pairing alone resolves); whose argmax of w over F is h.
 * pair_out: a discordant fragment is filed by the assigned strains of its two mates, at positions a and b of the species' candidate list, and adds one
 * (fragments only) at pair_out[pair_off[s] + a * K_s + b] and at [b][a].  pair_off_out / pair_cap as for pantax_hip_strain_read_support: more than
 * pair_cap entries is PANTAX_HIP_E_LIMIT with nothing but pair_off_out touched.
 * status_out [S]: 0 served; 1 for K_s = 0; PANTAX_HIP_E_LIMIT for K_s > 64 -- in the last two cases counted, paired, single, multi and mate_elsewhere are
 * still written and the other four classes are zeros.
 * frag_n_out [R] or NULL: only the entries of reads binned to a species of db are written: |F| for a read of a paired fragment of a served species, else -1.
 * Validation, before anything is written: a mate[r] that is neither code must be below R, differ from r, and mate[mate[r]] must be r; otherwise
 * PANTAX_HIP_E_INVALID (counted on the device).  Other PANTAX_HIP_E_INVALID cases of pantax_hip_read_strains.
 * Identities (all three numbers unless noted): counted = counted of pantax_hip_strain_read_support on the same candidates; counted = single + multi +
 * mate_elsewhere + paired with the n of paired taken twice; for a served species paired = concordant + discordant + half + unexplained, the sum of
 * assigned = concordant, unique_by_pair <= unique <= assigned <= compatible, the sum of its pair block = 2 x discordant.n; with every mate NONE single =
 * counted and every other class is zero.  Integers only: the same bits whatever the order and the membership route. */
#define PANTAX_HIP_FRAGMENT_CLASSES 9   /* counted, paired, concordant, discordant, half, unexplained, single, multi, mate_elsewhere */
int pantax_hip_strain_fragments(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const pantax_hip_read_strain_set *cand,
                                const uint32_t *mate /*[R] host, file order*/,
                                uint64_t *hap_out /*[C][4][3]: compatible, unique, unique_by_pair, assigned*/,
                                uint64_t *species_out /*[S][9][3]*/, int32_t *status_out /*[S]*/,
                                uint64_t *pair_off_out /*[S+1]*/, uint64_t pair_cap, uint64_t *pair_out,
                                int32_t *frag_n_out /*[R] or NULL*/);

/* ---- pairwise strain distinguishability of a db (the --db-pairs mode; not a stage of the reference): the strain step's LP has one 0/1 column per haplotype
 * over the nodes of its species (profile.rs:1333-1342); two haplotypes with equal columns cannot be told apart by it, and two whose columns differ on 300
 * bases of nodes only where those 300 bases are covered.  This call says, before any sample, which selected haplotypes of the db can be separated and by how
 * many bases of graph.  It takes the selection type of pantax_hip_strain_evidence; Sel_s, K_s, M(v) and m(v) are exactly as defined there: membership is
 * node-level (a node walked twice counts once), and every node of a species is counted once whether or not any walk visits it.
 *   Q(v) = (1, node_len[v]), both u64, in the order { n_nodes, len }.  Coverage is not read.
 *   pair_out [pair_off[S]][2]:  pair_out[pair_off[s] + a * K_s + b] = sum of Q(v) over the nodes v with both sel_hap entries at positions a and b of the
 *     species' list in M(v).  The block of a species is symmetric; its diagonal is the haplotype's own node set: { n_nodes, len } of the evidence call's all.
 *   pair_off_out [S+1] (pair_off[s + 1] = pair_off[s] + K_s^2) is computed on the host and always written; more than pair_cap entries: PANTAX_HIP_E_LIMIT
 *     with nothing else touched (call with pair_cap = 0 to size pair_out, as for pantax_hip_strain_read_support).
 *   species_out [S][3][2] or NULL, { total, none, core } of every species: total = the sum over every node; none = over m(v) = 0; core = over m(v) = K_s,
 *     two zeros when K_s = 0.  In the two columns they share they are the evidence call's total, orphan and core.
 * Every K_s from 0 to 256 is served (256: the width of the four-word LAD path and of the near-miss candidates).  An empty selection, or a species with
 * nothing selected, is fine.  Integers only: results are exact and independent of any order.
 * Identities: pair[a][b] <= min(pair[a][a], pair[b][b]);  core <= pair[a][b] for all a, b;  K_s = 1 gives pair = core;  total = none + the sum over m >= 1.
 * Derived by the host (the --db-pairs table prints them):
 *   only_a(a, b) = pair[a][a] - pair[a][b]: what a walks and b does not;
 *   distance(a, b) = only_a.len + only_b.len: the length of the symmetric difference, the bases of graph on which the LP can tell a from b.
 * State: the call needs an uploaded db with its graphs and nothing else -- no reads, no coverage pass.  It is legal before or behind any other call, and it
 * neither reads nor changes the coverage result or the step's state.
 * Errors (on any of them the outputs other than pair_off_out are left as given): K_s > 256: PANTAX_HIP_E_LIMIT naming the species; PANTAX_HIP_E_INVALID:
 * n_species different from the db's, a haplotype index out of range, a haplotype twice within a species; a db uploaded without graphs: PANTAX_HIP_E_STATE.
 * The option hap_pairs_route=walk (pantax_hip_set_option) takes every species' membership from its selected walks, as evidence_route=walk does;
 * hap_pairs_chunk=N cuts the node pass into chunks of N nodes (tests). */
int pantax_hip_db_hap_pairs(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel,
                            uint64_t *pair_off_out /*[S+1]*/, uint64_t pair_cap /* entries pair_out holds */, uint64_t *pair_out /*[pair_off[S]][2]*/,
                            uint64_t *species_out /*[S][3][2]: total, none, core; or NULL*/);

/* ---- pairwise strain evidence (the --strain-pair-evidence report; not a stage of the reference): pantax_hip_db_hap_pairs says, before any sample, on how
 * many bases of graph two haplotypes differ; the evidence call says what a selected haplotype has against ALL the others.  This call says, for every two
 * selected haplotypes of a species, how much of the graph they share and of the graph that separates them the sample covered.  Selection, Sel_s, K_s, M(v)
 * and m(v) are exactly those of pantax_hip_strain_evidence: membership is node-level (a node walked twice counts once), every node is counted once.
 *   Q(v) = (1, node_len[v], node_base_cov[v], bases_per_node[v]), all four u64, in the order { n_nodes, len, covered, bases }: the evidence call's Q,
 *     element for element.
 *   pair_out [pair_off[S]][4]:  pair_out[pair_off[s] + a * K_s + b] = sum of Q(v) over the nodes v with both sel_hap entries at positions a and b of the
 *     species' list in M(v).  The block of a species is symmetric, K_s x K_s, row-major from pair_off[s]; pair_off[s + 1] = pair_off[s] + K_s^2.
 *   species_out [S][3][4] or NULL: { total, orphan, core } of every species, as the evidence call writes them.
 * Every K_s from 0 to 256 is served; more: PANTAX_HIP_E_LIMIT naming the species.  Sizing as for pantax_hip_db_hap_pairs: pair_off_out is computed on the
 * host and always written (once the selection is valid); more than pair_cap entries: PANTAX_HIP_E_LIMIT with nothing else touched (call with pair_cap = 0
 * to size pair_out).  Integers only: results are exact and independent of any order; a u64 sum that overflows wraps exactly as the evidence call's does.
 * Identities: columns 0:2 of pair_out equal pantax_hip_db_hap_pairs on the same selection;  the diagonal pair[a][a] equals the evidence call's all of the
 * entry;  species_out equals the evidence call's;  pair[a][b] <= min(pair[a][a], pair[b][b]) in every column;  core <= pair[a][b] for all a, b.
 * Derived by the host (the report prints them):
 *   only_a(a, b) = pair[a][a] - pair[a][b] in all four columns: what a walks and b does not, and what the sample put there;
 *   class(a, b) from the len column exactly as the --db-pairs table derives it: identical (only_a.len = only_b.len = 0), nested (one of them 0), distinct.
 * State rules of pantax_hip_strain_evidence: the db must hold the coverage result of a pantax_hip_node_coverage call; behind a resident step
 * (pantax_hip_profile_step / _enqueue), and before any coverage pass, the call returns PANTAX_HIP_E_STATE and says why.  PANTAX_HIP_E_INVALID as in the
 * evidence call: n_species different from the db's, a haplotype index out of range, a haplotype twice within a species.  On any error the outputs other
 * than pair_off_out are left as given.  The call obeys hap_pairs_route and hap_pairs_chunk (pantax_hip_set_option) as pantax_hip_db_hap_pairs does. */
int pantax_hip_strain_pair_evidence(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel,
                                    uint64_t *pair_off_out /*[S+1]*/, uint64_t pair_cap /* entries pair_out holds */, uint64_t *pair_out /*[pair_off[S]][4]*/,
                                    uint64_t *species_out /*[S][3][4]: total, orphan, core; or NULL*/);

/* ---- model fit per strain (the --strain-fit report; not a stage of the reference): the reports above describe the SAMPLE on sets of nodes; this call
 * describes the FIT -- how far a table of strains with their predicted coverages is from the sample, node by node.  The strain step's LP has a row only
 * for a node with coverage (profile.rs:1380-1385), so a strain reported at 8x whose private genome is empty pays nothing for that; and a node that some
 * but not all reported strains walk is judged by no other report.  Selection, Sel_s, K_s, M(v) and m(v) are exactly those of pantax_hip_strain_evidence:
 * membership is node-level (a node walked twice counts once), every node of a species is counted once.  Every selection entry carries a weight sel_w, the
 * coverage predicted for its haplotype (the LP's x_h).
 *   p(v) = the f64 sum of sel_w over M(v): it starts from +0.0 and adds in ASCENDING species-local haplotype index, whatever the order of sel_hap, with
 *          plain IEEE-754 additions (no fused operation, no reassociation);
 *   t(v) = p(v) * (double)node_len[v], one IEEE multiplication;
 *   E(v) = the bases the table predicts on v, a u64: 0 when !(t > 0);  2^62 when t >= 2^62;  otherwise t rounded to the nearest integer, ties to even;
 *   b(v) = bases_per_node[v] as pantax_hip_node_coverage leaves it;
 *   excess(v) = b > E ? b - E : 0 (the sample has more than the table explains);   deficit(v) = E > b ? E - b : 0 (the table predicts more than the sample has);
 *   blind(v) holds exactly when b == 0 && E > 0: the LP had no row for such a node;
 *   Q(v) = (1, node_len[v], b, E, excess, deficit, blind ? 1 : 0, blind ? E : 0), eight u64, in the order
 *          { n_nodes, len, bases, expected, excess, deficit, blind_nodes, blind_expected }.
 * Every output is a sum of Q(v):
 *   per selection entry c (haplotype h of species s):   all[c] = sum over v with h in M(v);   private[c] = sum over v with M(v) = {h};
 *   per species s:   total[s] = sum over every node;   explained[s] = sum over m(v) >= 1;   orphan[s] = sum over m(v) = 0 (there E = 0: excess = bases).
 * hap_out [C][2][8] = { all, private } of every selection entry in the order of sel_hap; species_out [S][3][8] = { total, explained, orphan } of every
 * species.  E(v) is a deterministic function of the inputs and the sums are integers: results are exact and independent of any order; a u64 sum that
 * overflows wraps, as the evidence call's does.  Identities, column by column, modulo 2^64:  bases + deficit == expected + excess in every class;
 * total == explained + orphan;  blind_expected <= deficit;  columns { n_nodes, len, bases } of all, private, total and orphan equal columns { 0, 1, 3 } of
 * pantax_hip_strain_evidence on the same selection;  K_s = 1 gives all == private == explained;  all weights zero gives expected == deficit ==
 * blind_nodes == blind_expected == 0.  Every K_s the evidence call serves is served; an empty selection, or a species without selected haplotypes, is
 * fine (total == orphan).  State rules of pantax_hip_strain_evidence: PANTAX_HIP_E_STATE behind a resident step and before any coverage pass.
 * PANTAX_HIP_E_INVALID as in the evidence call (n_species different from the db's, a haplotype index out of range, a haplotype twice within a species),
 * and for a weight that is NaN, infinite or negative, or a null sel_w with C > 0.  On any error the outputs are left as given.
 * The option fit_route=walk (pantax_hip_set_option) takes every species' membership from its selected walks, as evidence_route=walk does. */
typedef struct {
    uint32_t n_species;       /* must equal the db's */
    const uint64_t *sel_off;  /* [S+1] species s owns the selection entries [sel_off[s], sel_off[s+1]) */
    const uint32_t *sel_hap;  /* [C] species-local haplotype index, any order, no repeats within a species */
    const double *sel_w;      /* [C] predicted coverage of the entry: finite, >= 0 */
} pantax_hip_fit_set;
int pantax_hip_strain_fit(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_fit_set *sel,
                          uint64_t *hap_out /*[C][2][8]: all, private*/, uint64_t *species_out /*[S][3][8]: total, explained, orphan*/);

/* ---- bootstrap of the strain fit (the --strain-bootstrap report; not a stage of the reference): strain_abundance.txt gives one number per strain, the
 * x_h of one L1 fit; a least-absolute-deviation fit is a weighted median and can jump between vertices when a handful of rows change.  This call says how
 * far the number moves when the rows are drawn again: it refits the LP of the selected strains on the sample's rows (replicate 0) and on n_replicates
 * Poisson-bootstrap resamples of them, all on the device.  Selection, Sel_s, K_s and M(v) are those of pantax_hip_strain_evidence; the inputs are node_len
 * and bases_per_node as pantax_hip_node_coverage leaves them.  Selection entry c of species s is COLUMN k = c - sel_off[s] of the species' LP.
 *   Rows of species s: every node v with a_v = (double)(long long)bases[v] / (double)node_len[v] > 0 and mask_v = sum over k of [sel_hap k in M(v)] << k != 0 is
 *   the row (mask_v, a_v).  No min_depth, no --sample cut, no first or second filter: the LP of profile.rs:1333-1451 restricted to the selected columns,
 *   0 <= x_k <= 1.05 max a (the box of profile.rs:1327, from the replicate's own rows) and no column pinned.  A node with a_v > 0 and mask_v = 0 gives no row
 *   and is no part of the objective here.
 *   Weight of row v in replicate b: 1 for b = 0 (the plain refit).  For b >= 1, with sm(x) = splitmix64's output function (x += 0x9E3779B97F4A7C15;
 *   x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31, in u64):
 *       r = sm(sm(seed ^ sm(sp_key[s])) + ((uint64_t)b << 40) + v_local),   v_local = the node's index inside its species,
 *       w = #{ j in 0..15 : r >= T[j] },   T[j] = floor(2^64 * sum_{i <= j} e^-1 / i!):   a Poisson(1) weight capped at 16.
 *   sp_key is the caller's name of the species (the file seam passes the taxid): the weights do not depend on where the species sits in the db.
 *   Replicate LP: minimise sum_v w_v |a_v - sum_k x_k bit_k(mask_v)| -- the LAD of the multiset in which row v occurs w_v times; amax, the pattern tables
 *   and the solver's scratch are formed from the replicate's own rows, and a pattern whose rows all drew 0 does not exist in it.
 * Outputs, replicate-major, R = n_replicates + 1:  x_out [R][C] the solution;  obj_out [R][S] the weighted objective above at x (a sum, not a mean);
 * rows_out [R][S] = sum of the weights;  status_out [R][S]:  0 solved;  1 nothing to solve (K_s = 0 or no row: x = 0, obj = 0);  PANTAX_HIP_E_LIMIT
 * K_s > 64 (x = 0, obj = 0, rows = 0; the other species are served);  PANTAX_HIP_E_SOLVER that LP failed, the others stand.
 * The call fails as a whole only on invalid arguments, a HIP error or PANTAX_HIP_E_LIMIT of its own (32-bit row positions; a replicate that does not fit
 * the option bootstrap_rows_max, the cap on the expanded rows in flight on the device, 0 = from the free device memory); on an error the outputs are left
 * as given.  State rules of pantax_hip_strain_evidence: PANTAX_HIP_E_STATE behind a resident step and before any coverage pass; PANTAX_HIP_E_INVALID as in
 * the evidence call, and for a null sp_key with S > 0.  Determinism: the same inputs give the same bits, whatever the chunking of the replicates
 * (bootstrap_rows_max), the membership route (option bootstrap_route=walk takes every species' membership from its selected walks) and the position of the
 * species in the db; the objective is summed in an order that is a function of the replicate's rows alone. */
typedef struct {
    uint32_t n_species;       /* must equal the db's */
    const uint64_t *sel_off;  /* [S+1] as pantax_hip_evidence_set */
    const uint32_t *sel_hap;  /* [C] species-local haplotype index, any order, no repeats within a species */
    const uint64_t *sp_key;   /* [S] the species' key of the weight hash */
    uint64_t seed;
    uint32_t n_replicates;    /* 0: the refit only */
} pantax_hip_bootstrap_set;
int pantax_hip_strain_bootstrap(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_bootstrap_set *sel, double *x_out /*[R][C]*/, double *obj_out /*[R][S]*/,
                                uint64_t *rows_out /*[R][S]*/, int32_t *status_out /*[R][S]*/);
/* host helpers, no ctx and no GPU.  The weight w of the contract above (replicate 0: 1): */
uint32_t pantax_hip_bootstrap_weight(uint64_t seed, uint64_t sp_key, uint32_t replicate, uint64_t v_local);
/* The summary of one quantity over the replicates b >= 1: x and status hold its n values and the LPs' statuses in ascending b (status NULL: all solved);
 * only the entries with status 0 count, m of them.  out[10] = { n_solved = m;  mean = the f64 sum in ascending b divided by m;  sd = sqrt(sum of
 * (x - mean)^2 in ascending b / (m - 1)), 0 for m < 2;  q025, q25, q50, q75, q975 = the sorted value at index floor(p (m - 1) / 1000), p = 25, 250, 500,
 * 750, 975 in integer arithmetic;  zero_fraction = the share of the m values with x == 0.0;  min }.  m = 0: n_solved = 0 and nine zeros.
 * PANTAX_HIP_E_INVALID for a null out, or a null x with n > 0. */
int pantax_hip_bootstrap_summary(uint64_t n, const double *x, const int32_t *status, double *out /*[10]*/);

/* ---- leave-one-out test of the strain fit (the --strain-dropout report; not a stage of the reference): does the sample need a reported strain at all, or
 * is the L1 fit as good without it?  The bootstrap cannot say: a strain whose coverage another strain absorbs at no cost is as stable as a well-founded one.
 * Selection, Sel_s, K_s, M(v), the inputs, the state rules and the argument errors are those of pantax_hip_strain_bootstrap without sp_key, seed and
 * replicates; the rows of species s are the rows of its replicate 0 (every node with a_v > 0 and mask_v != 0, column k = selection entry sel_off[s] + k).
 *   Species s has E_s = K_s + 1 entries.  Entry 0 is the plain refit; entry k + 1 is the same LP with column k pinned to zero: 0 <= x_j <= 1.05 max a for
 *   j != k (max a over the species' rows, the same in every entry), x_k = 0; the rows and their masks stay, so a row with mask_v = {k} stays in the objective
 *   with prediction 0 and costs a_v.  (profile.rs:1333-1451 on the selected columns with one column's upper bound at zero.)
 * Outputs, sized by the caller; entry (s, e) has index q = sel_off[s] + s + e, Q = C + S entries exist:
 *   x_out      per species a block of E_s x K_s doubles at x_off[s] = sum over t < s of E_t K_t, entry-major; x[e][k] of entry e = k + 1 is exactly 0.0;
 *   obj_out    [Q] sum over the rows of |a_v - sum_j x_j bit_j(mask_v)| at the entry's x (a sum, as in the bootstrap);
 *   status_out [Q] 0 solved;  1 nothing to solve (no row, or K_s = 0: x = 0, obj = 0);  PANTAX_HIP_E_LIMIT K_s > 64 (the other species are served);
 *              PANTAX_HIP_E_SOLVER that LP alone failed;
 *   rows_out   [S] the species' rows;
 *   count_out  [Q][4] = { n_member, n_only, n_worse, n_better } of entry k + 1: rows with bit k; rows with mask == 1 << k; rows whose absolute residual
 *              under entry k + 1 is strictly larger / strictly smaller than under entry 0.  Entry 0 holds { rows, 0, 0, 0 }.  The residual of a row is
 *              fabs(s - a), s the f64 sum of the entry's x_j over the set bits in ascending j: the counts are a function of the delivered x.
 * The call fails as a whole only on invalid arguments, a HIP error or PANTAX_HIP_E_LIMIT of its own (32-bit row positions; one round of LPs -- entry e of
 * every species over one copy of the pattern tables -- that does not fit the option dropout_patterns_max, the cap on the replicated patterns in flight,
 * 0 = from the free device memory); on an error the outputs are left as given.  Determinism: the same inputs give the same bits, whatever the chunking
 * of the rounds (dropout_patterns_max), the membership route (option dropout_route=walk) and the position of the species in the db; the objective is summed
 * in an order that is a function of the species' sorted rows alone. */
int pantax_hip_strain_dropout(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_evidence_set *sel, double *x_out, double *obj_out /*[Q]*/,
                              int32_t *status_out /*[Q]*/, uint64_t *rows_out /*[S]*/, uint64_t *count_out /*[Q][4]*/);
/* host helper, no ctx and no GPU: who takes over when column k of K is dropped.  x_full / x_drop [K]: the x of entry 0 and of entry k + 1.
 * out[3] = { the column j != k with the largest x_drop[j] - x_full[j] (ties: the lowest j), -1 when no difference is positive;  that gain (0 when none);
 * sum over j != k of |x_drop[j] - x_full[j]| in ascending j }.  PANTAX_HIP_E_INVALID for a null argument or k >= K. */
int pantax_hip_dropout_substitute(uint32_t K, uint32_t k, const double *x_full, const double *x_drop, double *out /*[3]*/);

/* ---- add-one test of the strain fit (not a stage of the reference): the false-negative test beside the leave-one-out test.  For a haplotype that a filter
 * dropped: how much better would the L1 fit of this sample be with it in the LP, what coverage would it get, and which reported strain would it take that
 * coverage from?  The near-miss call counts bases; only the LP can say this.
 * Selection type, Sel_s, Cand_s, M(v), N(v), the state rules and the argument errors are those of pantax_hip_strain_near_miss (PANTAX_HIP_E_INVALID also for
 * a haplotype twice within Sel_s or within Cand_s, and for one in both); the inputs are those of pantax_hip_strain_bootstrap.
 *   Columns: species s has K_s reported and J_s candidate haplotypes, W_s = K_s + J_s columns.  Column k < K_s is selection entry sel_off[s] + k, column
 *   K_s + c is candidate entry cand_off[s] + c.
 *   Rows: the bootstrap's replicate-0 rows for the selection Sel_s ++ Cand_s: every node with a_v = (double)(long long)bases / (double)len > 0 and a non-empty
 *   mask over the W_s columns.  No min_depth, no sample cut, no filter.  The row set is the same in every entry of a species: the objectives are comparable.
 *   Entries: E_s = J_s + 1.  Entry 0 pins every candidate column to zero: the refit of the reported strains over these rows, in which a row that only
 *   candidates walk costs a_v.  Entry c + 1 frees candidate c and pins the other candidates; the reported columns are free in every entry.  Box:
 *   0 <= x <= 1.05 max a, max a over the species' rows, the same in every entry.  A pinned column is delivered as exactly +0.0.  K_s = 0 makes entry 0
 *   all-pinned: no LP is launched, x = 0, obj = sum of a, status 0 (the rule of the leave-one-out call's entry 1 at K_s = 1).
 * Outputs, sized by the caller; entry (s, e) has index q = cand_off[s] + s + e, Q = J + S entries exist:
 *   x_out      per species a block of E_s x W_s doubles at x_off[s] = sum over t < s of E_t W_t, entry-major;
 *   obj_out    [Q] the SUM over the rows of |a_v - sum_j x_j bit_j(mask_v)| at the entry's x;
 *   status_out [Q] 0 solved;  1 nothing to solve (no row, or W_s = 0: x = 0, obj = 0);  PANTAX_HIP_E_LIMIT W_s > 64 (the other species are served);
 *              PANTAX_HIP_E_SOLVER that LP alone failed;
 *   rows_out   [S] the species' rows;
 *   count_out  [Q][4] = { n_member, n_novel, n_better, n_worse } of entry c + 1: rows with bit K_s + c; rows with bit K_s + c and no bit below K_s; rows whose
 *              absolute residual under entry c + 1 is strictly smaller / strictly larger than under entry 0.  Entry 0 holds { rows, rows with no bit below
 *              K_s, 0, 0 }.  The residual of a row is fabs(s - a), s the f64 sum of the entry's x_j over the set bits in ascending j: the counts are a function
 *              of the delivered x.
 * The call fails as a whole only on invalid arguments, a HIP error or PANTAX_HIP_E_LIMIT of its own (32-bit row positions; one round of LPs -- entry e of
 * every species over one copy of the pattern tables -- that does not fit the option addin_patterns_max, the cap on the replicated patterns in flight,
 * 0 = from the free device memory); on an error the outputs are left as given.  Determinism: the same inputs give the same bits, whatever the chunking of
 * the rounds (addin_patterns_max), the membership route (option addin_route=walk) and the position of the species in the db; the objective is summed in an
 * order that is a function of the species' sorted rows and its column counts alone. */
int pantax_hip_strain_addin(pantax_hip_ctx *ctx, pantax_hip_db *db, const pantax_hip_near_miss_set *sel, double *x_out, double *obj_out /*[Q]*/,
                            int32_t *status_out /*[Q]*/, uint64_t *rows_out /*[S]*/, uint64_t *count_out /*[Q][4]*/);
/* host helper, no ctx and no GPU: which reported strain gives coverage up when a candidate enters.  x_base / x_add [W]: the x of entry 0 and of entry c + 1;
 * the first K columns are the reported ones.  out[3] = { the column j < K with the largest x_base[j] - x_add[j] (ties: the lowest j), -1 when no difference
 * is positive;  that loss (0 when none);  sum over j < K of |x_add[j] - x_base[j]| in ascending j }.  PANTAX_HIP_E_INVALID for a null argument or K > W. */
int pantax_hip_addin_donor(uint32_t W, uint32_t K, const double *x_base, const double *x_add, double *out /*[3]*/);

/* ---- SURVEY 8e, reads over N GPUs: bin where tokenised, route to the owner of the species ------------------------
 * The reference groups the reads by species in one process (group_reads_by_species, profile.rs:439-463) and hands each
 * species' records to its rayon task.  With one process per GPU every rank holds a 1/N slice of the reads (its byte range
 * of the GAF): it bins the slice against ALL species ranges (pantax_hip_bin_reads), packs one message per owner rank
 * (route_pack: stable partition on the device, order of the slice kept; "U" reads, reads of species nobody owns and reads
 * with a drop flag are left behind), the host moves the messages (RCCL all-to-all(v) over xGMI on the device buffers, MPI,
 * ...), and the owner builds resident reads from what it received (reads_from_routed: messages in source-rank order, so the
 * result is the one-process read order restricted to the owner's species).
 * Message layout, 32-bit words: n_steps[n] pstart[n] pend[n] qlen[n] mapq[n] node_id[n_steps_total]. */
typedef struct pantax_hip_route pantax_hip_route;
int pantax_hip_reads_route_pack(pantax_hip_ctx *ctx, const pantax_hip_db *db /* the db `reads` were binned against */,
                                const pantax_hip_reads *reads, const int32_t *owner_of_species /*[S] rank, or < 0: nobody*/,
                                int world_size /* <= 64 */, pantax_hip_route **out, uint64_t *n_reads_to /*[W] out*/,
                                uint64_t *n_steps_to /*[W] out*/);
/* the W messages, back to back in rank order: buf_out[word_off_out[d] .. word_off_out[d+1]) goes to rank d
 * (word_off_out [W+1], may be NULL: 5 * n_reads_to + n_steps_to each).  on_device = 1: device pointer (valid until
 * route_free), 0: pinned host copy. */
int pantax_hip_route_buffer(pantax_hip_ctx *ctx, pantax_hip_route *route, int on_device, const uint32_t **buf_out,
                            uint64_t *word_off_out);
void pantax_hip_route_free(pantax_hip_ctx *ctx, pantax_hip_route *route);
/* recv: the messages of ranks 0..W-1 for this rank, back to back (device pointer when on_device, else host memory);
 * n_reads_from / n_steps_from [W] as announced by the senders.  The reads come out ready for pantax_hip_bin_reads. */
int pantax_hip_reads_from_routed(pantax_hip_ctx *ctx, const uint32_t *recv, int on_device, int world_size,
                                 const uint64_t *n_reads_from, const uint64_t *n_steps_from, pantax_hip_reads **out);

/* ---- resident step: the in-memory core of profile::profile (profile.rs:3325-3364) between "GAF parsed"
 * and "tables written", over a db and reads that are already in HBM.  One call = rcls_profile ->
 * species_profiling -> trio_nodes_info (when rebuild_trio) -> get_node_abundances -> strain_profiling ->
 * the abundance_est filters; the stages above remain available one by one and give identical results.
 * The host waits once, at the end.  Outputs are the LOCAL quantities of this rank's species: the global
 * normalisers (profile.rs:341, :3198, :3243) are sums of absolute_out / species_sum_*_out over ranks. */
typedef struct {
    double unique_trio_nodes_fraction, unique_trio_nodes_mean_count_f, single_cov_ratio, single_cov_diff; /* --fr --fc --sr --sd */
    int64_t min_cov, min_depth;
    int32_t shift, filtered, sample_nodes /* as in pantax_hip_strain_config */, rebuild_trio /* 1 = like the reference, every run */;
    int32_t solver_semantics;              /* as in pantax_hip_strain_config */
} pantax_hip_step_config;

int pantax_hip_profile_step(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads,
                            const double *avg_len /*[S] species_genomes_stats.txt*/, const pantax_hip_step_config *cfg,
                            uint8_t *keep_out /*[S] species kept by species_profiling*/, double *absolute_out /*[S] predicted_coverage*/,
                            pantax_hip_hap_metrics *metrics_out /*[H]*/, pantax_hip_solve_info *info_out /*[S] or NULL*/,
                            uint8_t *pass_out /*[H]*/, double *species_sum_all_out /*[S] or NULL*/,
                            double *species_sum_pass_out /*[S] or NULL*/);

/* The same step in two halves, for a caller that streams samples: `enqueue` puts the whole step on the device and returns
 * without waiting; `collect` takes the OLDEST enqueued step of the db: its one host wait, the reporting arithmetic and the
 * a15 filters (outputs as above).  Up to two steps of a db may be in flight, so step i+1 can be enqueued before step i is
 * collected and the device never waits for the host between two steps.  On the device the main-stream work of the steps runs
 * one step after the other; only the unique-trio rebuild of step i+1 (side stream, rebuild_trio != 0) may start earlier:
 * behind the first filter of step i -- the last reader of the index -- beside step i's masks, row sort and LPs, which read
 * copies.  Every step computes what the one-call form computes; `reads` / `avg_len` of an enqueued step must stay valid until its collect (avg_len is copied at enqueue). */
int pantax_hip_profile_step_enqueue(pantax_hip_ctx *ctx, pantax_hip_db *db, pantax_hip_reads *reads, const double *avg_len,
                                    const pantax_hip_step_config *cfg);
int pantax_hip_profile_step_collect(pantax_hip_ctx *ctx, pantax_hip_db *db, uint8_t *keep_out, double *absolute_out,
                                    pantax_hip_hap_metrics *metrics_out, pantax_hip_solve_info *info_out, uint8_t *pass_out,
                                    double *species_sum_all_out, double *species_sum_pass_out);

/* A resident db that serves one sample after the other: the unique-trio index of the COMING run (trio_nodes_info, profile.rs:2936 --
 * it depends on the graphs only) is started now, e.g. right before that run's GAF is loaded, so that it is built beside the PCIe
 * transfer instead of in front of the coverage pass.  The next profile_step / _enqueue of the db with rebuild_trio != 0 uses it instead
 * of building again (one build per run, as in the reference); nothing is waited for here. */
int pantax_hip_trio_index_prefetch(pantax_hip_ctx *ctx, pantax_hip_db *db);

/* ---- the device sort of the LP row grouping as a host-buffer utility: rows (k0[i], k1[i], k2[i]) sorted
 * ascending as tuples, in place.  algo: 0 = what the strain step would pick for n rows, 1 = LSD radix sort,
 * 2 = sample sort (n <= 600000), 4 = the batched sort of the many-species step: entries arrive grouped by ascending k0
 * (one segment per k0 value, of any size), (k1, k2) is sorted inside every segment, straight from the node arrays: an entry
 * whose k1 is 0 or whose k2 is not the bit pattern of a positive double is no row -- the rows come back
 * sorted in the first entries, the rest of the three arrays is zeroed; 5 = 4 with k1 < 256 and the segment number packed into
 * the mask word on the device (the step's two-word records).  (3, round 3's segmented sort, is gone: PANTAX_HIP_E_INVALID.) */
int pantax_hip_sort_rows(pantax_hip_ctx *ctx, uint64_t n, uint64_t *k0, uint64_t *k1, uint64_t *k2, int algo);

/* ---- the device primitives under every stage as host-buffer utilities (api_primitives.cpp): each uploads, runs on the ctx's stream, downloads
 * and synchronises.  They exist so that tests can compare the primitives with a host reference at the shapes the product runs them at.
 *
 * scan: out[i] = in[0] + .. + in[i - 1] in 32-bit arithmetic over n items of item_bytes = 1 or 4 bytes; *total_out (may be NULL) = the sum of all,
 * *tile_items_out (may be NULL) = the items per workgroup the launch used (2048, 8192 or 16384: by n, or what the ctx's option "scan_tile"
 * forces).  in_place != 0 (4-byte items only): the device scan reads and writes one buffer. */
int pantax_hip_scan(pantax_hip_ctx *ctx, uint64_t n, const void *in, int item_bytes, int in_place, uint32_t *out, uint32_t *total_out,
                    uint32_t *tile_items_out);
/* radix sort: n records of nw = 1, 2 or 3 key words (k0 .. k[nw - 1]; the others NULL) and an optional 32-bit payload (NULL: none), sorted in
 * place by a stable LSD radix sort over the n_passes digits (k[pass_word[p]] >> pass_shift[p]) & 0xFF, pass 0 the least significant.  n fixes the
 * launch geometry, n_actual <= n is the record count the device is given: the first n_actual records come back sorted, the others as they went
 * in (both device sides hold the caller's records beforehand; all n records of the side that holds the result are fetched).
 * *result_in_b_out (may be NULL) = 1 when the result ended on the second side (an odd number of passes). */
int pantax_hip_radix_sort(pantax_hip_ctx *ctx, uint64_t n, uint64_t n_actual, int nw, uint64_t *k0, uint64_t *k1, uint64_t *k2, uint32_t *payload,
                          const int32_t *pass_word, const int32_t *pass_shift, int n_passes, int *result_in_b_out);
/* fill: a device buffer of buf_bytes is set to the byte `sentinel`, then [off, off + bytes) of it to `byte` by the library's fill (the runtime's
 * memset below 1 MiB, 16-byte stores from every CU from there on); out[buf_bytes] = the whole buffer afterwards. */
int pantax_hip_fill(pantax_hip_ctx *ctx, uint64_t buf_bytes, int sentinel, uint64_t off, uint64_t bytes, int byte, uint8_t *out);

/* filter_max_alignment_mt (gaf_filter.rs:44-97, called by alignment.rs:171 on long-read GAFs): per read id
 * keep the line with the largest (matches, identity) if it also has mapq > 20 and span > 1000; one line per id.
 * Parsed and grouped on the device; the kept lines are written in FILE ORDER (the reference's order and its choice
 * among equal-best lines are rayon scheduling accidents; here: the first such line).  out_path NULL =
 * "<stem>_filtered.gaf" beside the input.  Counters may be NULL. */
int pantax_hip_gaf_filter(pantax_hip_ctx *ctx, const char *gaf_path, const char *out_path, uint64_t *n_lines,
                          uint64_t *n_records, uint64_t *n_written);

/* device-ready images of the species of a resident db, one file per species (graph in the kernels' layouts +
 * its unique-trio index): written from a db (the index is built first if needed; hap_names[H] in db order) and read
 * back into a db whose trio index is already in place -- a6 becomes "map + copy", a7 a no-op. */
int pantax_hip_db_save_images(pantax_hip_ctx *ctx, pantax_hip_db *db, const char *const *paths /*[S]*/,
                              const char *const *hap_names /*[H]*/);
int pantax_hip_db_load_images(pantax_hip_ctx *ctx, uint32_t n_species, const char *const *paths, const int64_t *range_start,
                              const int64_t *range_end, pantax_hip_db **out);

/* a11 (sample_sorted, profile.rs:1287-1295): which of n_valid rows `StdRng::seed_from_u64(seed)` +
 * `choose_multiple(sample_nodes)` keeps, as a bitmap over their ranks (bits_out: (n_valid+31)/32 words).  Host only.
 * rand 0.9.2 / rand_chacha 0.9.0 (Cargo.lock) are restated, not linked: parity with the crates is unpinned. */
int pantax_hip_sample_ranks(uint64_t n_valid, uint64_t sample_nodes, uint64_t seed, uint32_t *bits_out);
/* one ChaCha block (64-bit counter, zero stream id, `rounds` = 8/12/20) of the generator above, for known-answer tests */
int pantax_hip_chacha_block(const uint32_t *key8, uint64_t counter, int rounds, uint32_t *out16);

/* ---- solver seam: one species, host buffers in, same meaning as X_opt's arguments
 * (profile.rs:2690-2698).  cand_path_idx = possible_paths_idx; fixed_zero[k]=1 pins x_k = 0
 * (second solve, profile.rs:1484-1488).  x_out [n_cand]; path_cov_ratio_out [n_cand] or NULL. */
int pantax_hip_pao_solve(pantax_hip_ctx *ctx, uint32_t n_nodes, const int64_t *node_len,
                         const double *node_abundance, const uint64_t *node_base_cov, uint32_t n_paths,
                         const uint64_t *path_off, const uint32_t *path_nodes, uint32_t n_cand,
                         const uint32_t *cand_path_idx, const uint8_t *fixed_zero, double *x_out,
                         float *path_cov_ratio_out, double *obj_out, int32_t *status_out);

/* The same seam for MANY species in one call (SURVEY.md 8b "pao_solve_batch": what the GPU wants -- one workgroup per
 * species, all LPs side by side).  A Rust caller that keeps its own first filter (profile.rs:2969-3009 inside the rayon loop
 * of :3297-3319) collects the arguments of its X_opt calls as arrays of offsets and gets every species' answer back.
 * Species s owns nodes [node_off[s], node_off[s+1]), haplotypes [hap_off[s], hap_off[s+1]) and candidates
 * [cand_off[s], cand_off[s+1]); path_off indexes path_nodes over all haplotypes of the batch; cand_path_idx is the
 * haplotype's index WITHIN its species.  Any number of candidates, as in the reference (dense nvert x npaths matrix,
 * profile.rs:1333-1342): 1..64 take the one-word path, 65..256 four mask words, more than 256 haplotypes a solver whose mask words,
 * basis inverse and column state are sized at run time.  status[s]: 0 solved (or nothing to solve: no candidates),
 * PANTAX_HIP_E_SOLVER -- per species, like the reference drops only the species whose solver failed
 * (profile.rs:2999-3003); the call itself fails only on invalid arguments or a HIP error. */
typedef struct {
    uint32_t n_species;
    const uint64_t *node_off;       /* [S+1] */
    const int64_t *node_len;        /* [V] */
    const double *node_abundance;   /* [V] */
    const uint64_t *node_base_cov;  /* [V] or NULL (only path_cov_ratio needs it) */
    const uint64_t *hap_off;        /* [S+1] */
    const uint64_t *path_off;       /* [H+1] */
    const uint32_t *path_nodes;     /* [P] species-local 0-based node ids */
    const uint64_t *cand_off;       /* [S+1] */
    const uint32_t *cand_path_idx;  /* [C] possible_paths_idx of every species, concatenated */
    const uint8_t *fixed_zero;      /* [C] or NULL: 1 pins x_k = 0 (second solve, profile.rs:1484-1488) */
} pantax_hip_species_batch;
typedef struct {
    double *x;              /* [C] out */
    float *path_cov_ratio;  /* [C] out or NULL */
    double *obj;            /* [S] out or NULL */
    int32_t *status;        /* [S] out */
    int32_t *iters;         /* [S] out or NULL: pivots of the active-set solver */
} pantax_hip_solution_batch;
int pantax_hip_pao_solve_batch(pantax_hip_ctx *ctx, const pantax_hip_species_batch *in, const pantax_hip_solution_batch *out);

/* ---- pipeline seam: files in, files out (profile.rs:3325) -------------------------------- */
typedef struct { /* ProfilingConfig (types.rs:57-91) as plain C; NULL path = reference default under db/wd */
    const char *db, *wd, *output_dir;
    const char *genomes_metadata, *range_file, *input_aln_file, *species_len_file, *out_binning_file, *reads_binning_file;
    double min_species_abundance, unique_trio_nodes_fraction, unique_trio_nodes_mean_count_f, single_cov_ratio,
        single_cov_diff;
    int64_t min_cov, min_depth;
    int32_t species, strain, shift, filtered, full, force, mode, sample_nodes;
    const char *designated_species; /* --ds or NULL */
    const char *zip;                /* "serialize" (.bin) | "lz" (.bin.lz4) | "zstd" (.bin.zst) | NULL (= GFA); "h5" is refused */
    /* one process per GPU: with world_size > 1 this process takes its share of the selected species (longest-processing-
     * time packing on reads + graph size, the same table on every rank) and rank 0 writes the tables.
     * With `alltoallv` set the INPUT is sharded too: rank r tokenises and bins only its line-aligned 1/N byte range
     * of the GAF, the species counters are summed over the ranks, the duplicate-id rule (profile.rs:361-437) is decided on
     * (id hash, species) records exchanged by hash, and the packed records of every read travel to the rank that owns its
     * species (pantax_hip_reads_route_pack / _from_routed) -- no rank ever reads the whole file.  Without it every rank
     * tokenises the whole GAF (simple, but N x the ingest).
     * Collectives per run: allreduce_sum a handful of times (run mode; {failure flag, counters}; {failure flag, the two
     * normalisers}; barriers around the part files) -- every rank-local failure is carried in such a flag, so the ranks
     * always leave together -- and, when sharded, alltoallv two to three times (id records; packed reads; the ids to drop,
     * only if some id does span species). */
    int32_t rank, world_size;
    /* device-ready graph images <db>/species_graph_info/<otu>.hipdb (graphs + unique-trio index):
     * 0 = ignore them, 1 = use them when every selected species has a fresh one, 2 = as 1, and write them after a run
     * that had to parse the graphs */
    int32_t image_cache;
    /* world_size > 1: in-place sum over all ranks of buf[0..n) (e.g. ncclAllReduce + stream sync, MPI_Allreduce); 0 = ok */
    int (*allreduce_sum)(void *user, double *buf, uint64_t n);
    void *comm_user;
    /* world_size > 1, optional (NULL = unsharded input): bytes send[send_off[j] .. send_off[j+1]) of rank i arrive as
     * recv[recv_off[i] .. recv_off[i+1]) on rank j; both offset arrays have world_size + 1 entries and every rank passes
     * recv offsets that match what the others send (the library exchanges the sizes through allreduce_sum first).
     * E.g. ncclGroupStart + ncclSend/ncclRecv per peer + ncclGroupEnd + stream sync, or MPI_Alltoallv.  0 = ok.
     * comm_device_buffers != 0: send / recv are DEVICE pointers of this ctx's GPU (RCCL moves HBM to HBM over xGMI);
     * 0: host pointers (the library stages through pinned memory). */
    int (*alltoallv)(void *user, const void *send, const uint64_t *send_off, void *recv, const uint64_t *recv_off);
    int32_t comm_device_buffers;
    int32_t sample_test;            /* --sample_test (cli.rs:230-232): sample_sorted keeps 500 rows whatever --sample says (profile.rs:1387-1393, :2738-2744) */
    int32_t solver_semantics;       /* --solver: PANTAX_HIP_SEMANTICS_HIGHS for "highs", PANTAX_HIP_SEMANTICS_GUROBI for every other backend (pantax_hip_strain_config) */
    double minimization_min_cov;    /* types.rs:72 (main.rs:150 sets 0; no CLI flag).  It only shifts the indicator rows z_i >= (x_i - this) / (2 max), and the
                                     * indicators are bound by nothing but sum z <= npaths (profile.rs:1374-1378): INERT at any value.  Mirrored for
                                     * completeness of the struct; negative or non-finite values are refused. */
    /* --read-strains: path of the per-read strain report (pantax_hip_read_strains over every group of species; NULL or "None" = off).
     * TSV without header, one row per GAF record in the order and count of the -R report (the two files join by position):
     * read_id, species_taxid (both as in the -R report), genome_ID, strain_taxid (the genomes_info.txt join of the strain table),
     * n_compatible, posterior (shortest round-trip digits).  No strain: "U U 0 0" when no candidate contains the read's nodes,
     * "U U - 0" when the read is not counted in a species or its species has no candidates.  Written only by a run that performs the
     * strain step; world_size > 1 or a sharded ingest with it is PANTAX_HIP_E_INVALID. */
    const char *read_strain_file;
    /* --strain-coverage: path of the per-strain coverage track (pantax_hip_strain_cov_track over every group of species, right behind the group's strain
     * step; NULL or "None" = off).  TSV with a header; the strains are the rows of strain_abundance.txt, in its order, every strain's windows ascending:
     * species_taxid, strain_taxid, genome_ID (as in the strain table), start = w * W, end = min((w + 1) * W, G_h), n_nodes, len, covered, bases,
     * depth = bases / len, breadth = covered / len (f64, shortest round-trip digits).  Windows with len = 0 are not written.  Written only by a run
     * that performs the strain step; world_size > 1 or a sharded ingest with it is PANTAX_HIP_E_INVALID (rows would have to be joined across ranks). */
    const char *strain_coverage_file;
    int64_t strain_coverage_window; /* --strain-coverage-window: W in bases; 0 = the default of 10000; negative: PANTAX_HIP_E_INVALID */
    /* --strain-evidence: path of the per-strain node evidence report (pantax_hip_strain_evidence over every group of species, right behind the group's
     * strain step; Sel_s = the species' rows of strain_abundance.txt; NULL or "None" = off).  TSV with a header, long format:
     * species_taxid, strain_taxid, genome_ID, class, n_nodes, len, covered, bases, depth = bases / len, breadth = covered / len (f64, shortest round-trip
     * digits; "-" when len = 0), predicted_coverage.  First the strains in the order of strain_abundance.txt, classes "all" then "private" each
     * (predicted_coverage = the unrounded second_sol); then every species that went through a strain step, in the order the run took them (the order of
     * species_abundance.txt among the selected species), classes "total", "orphan", "core" with strain_taxid = genome_ID = "-"; "core" is left
     * out for a species without rows; predicted_coverage is "-" on total and orphan, and on core the f64 sum of the species' reported strains in
     * ascending haplotype index.  Written only by a run that performs the strain step; world_size > 1 or a sharded ingest with it is PANTAX_HIP_E_INVALID. */
    const char *strain_evidence_file;
    /* --strain-read-support: path of the per-strain read support report (pantax_hip_strain_read_support over every group of species, right behind the
     * group's strain step; candidates and weights as for read_strain_file; NULL or "None" = off).  TSV with a header, long format: species_taxid,
     * strain_taxid, genome_ID, class, n_reads, n_steps, span, fraction, other_strain_taxid.  First the strains in the order of strain_abundance.txt, classes
     * "compatible", "unique", "assigned" each (fraction = n_reads / the species' counted n_reads, f64 with shortest round-trip digits, "-" when that is 0;
     * other_strain_taxid "-"); then every species that went through a strain step, in the order the run took them, classes "counted", "unexplained",
     * "ambiguous", "uninformative" with strain_taxid = genome_ID = other_strain_taxid = "-" (a species without rows: "counted" only); then one row of class
     * "shared" per pair a < b of rows of a species of at most 64 rows with a non-zero count: a's strain columns, other_strain_taxid = b's strain taxid,
     * n_steps = span = "-", fraction = the count / min(compatible_a, compatible_b).  Written only by a run that performs the strain step; world_size > 1 or a
     * sharded ingest with it is PANTAX_HIP_E_INVALID. */
    const char *strain_read_support_file;
    /* --strain-depth: path of the per-strain depth distribution report (pantax_hip_strain_depth over every group of species, right behind the group's
     * strain step; Sel_s = the species' rows of strain_abundance.txt; NULL or "None" = off).  TSV with a header, long format: species_taxid, strain_taxid,
     * genome_ID, class, n_nodes, len, len_zero, q05, q25, q50, q75, q95, q50_hi, predicted_coverage.  First the strains in the order of
     * strain_abundance.txt, classes "all" then "private" each (predicted_coverage = the unrounded second_sol); then every species that went through a
     * strain step, in the order the run took them, classes "total" and "orphan" with strain_taxid = genome_ID = "-" and predicted_coverage "-".
     * n_nodes and len are the histogram summed over its bins, len_zero the len of bin 0; qXX = lo(bin) of the length-weighted quantile
     * (pantax_hip_depth_quantile at 50, 250, 500, 750, 950 per mille), q50_hi = hi(bin) of the median's bin: the resolution of the median.  Every quantile
     * column is "-" when len = 0.  Written only by a run that performs the strain step; world_size > 1 or a sharded ingest with it is PANTAX_HIP_E_INVALID. */
    const char *strain_depth_file;
    /* --strain-near-miss: path of the unreported-strain near-miss report (pantax_hip_strain_near_miss over every group of species, right behind the
     * group's strain step; NULL or "None" = off).  Sel_s = the species' rows of strain_abundance.txt.  Cand_s of a species of <= 64 haplotypes = every other
     * haplotype of the species; of a wider species = the unreported haplotypes that carry PANTAX_HIP_HAS_FRACTION, by unique_trio_nodes_fraction descending
     * then index ascending, the first 256 (the cap bounds the node-mask arena).  TSV with a header, long format: species_taxid, strain_taxid, genome_ID, rank,
     * class, n_nodes, len, covered, bases, depth, breadth, share, stage, unique_trio_nodes_fraction, frequencies_mean, first_sol, second_sol.  Candidate rows
     * first: per species in the order the run took them, the candidates pantax_hip_near_miss_rank keeps with strain_near_miss_top, rank from 1, classes
     * "novel", "exclusive", "all" each (all = the evidence call's all of the haplotype); depth = bases / len, breadth = covered / len ("-" when len = 0);
     * share = bases / the species' orphan bases ("-" on class all and when that is 0); stage = where the haplotype left the path: first_filter (no
     * PANTAX_HIP_HAS_FIRST), second_filter (HAS_FIRST, no HAS_SECOND), table_filter (HAS_SECOND, not a row of the table); the four metric columns are "-"
     * where their has bit is clear; strain_taxid / genome_ID = the first genomes_info.txt row of the haplotype (empty without one).  Then every species
     * that went through a strain step: classes "orphan", "claimed", "contested" with strain, rank, stage and metric columns "-", share = bases / orphan
     * bases.  Written only by a run that performs the strain step; world_size > 1 or a sharded ingest with it is PANTAX_HIP_E_INVALID. */
    const char *strain_near_miss_file;
    int32_t strain_near_miss_top;   /* --strain-near-miss-top: candidates printed per species; 0 = the default of 5; negative: PANTAX_HIP_E_INVALID */
    /* --strain-pair-evidence: path of the pairwise strain evidence report (pantax_hip_strain_pair_evidence over every group of species, right behind the
     * group's evidence sums, on the same coverage result; NULL, "" or "None" = off).  Sel_s = the species' rows of strain_abundance.txt, in ascending
     * haplotype index.  TSV with a header: species_taxid, strain_taxid, genome_ID, other_strain_taxid, other_genome_ID, class, n_nodes, len, covered, bases,
     * depth, breadth, predicted_coverage, pair_class.  Species in the order they went through the device; for every two entries a < b of a species three
     * rows: class "shared", head a, other b, pair[a][b], predicted_coverage = second_sol(a) + second_sol(b) (a lower bound of what is expected there: other
     * strains may walk these nodes too); class "only", head a, other b, pair[a][a] - pair[a][b], predicted_coverage = second_sol(a); class "only", head b,
     * other a, pair[b][b] - pair[a][b], predicted_coverage = second_sol(b).  An entry stands in the table with its first row of strain_abundance.txt.
     * depth = bases / len, breadth = covered / len ("-" when len = 0).  pair_class, the same on the three rows: identical, nested or distinct, from the len
     * column as the --db-pairs table derives it.  A species with fewer than two rows writes nothing; one with more than 256 rows writes one row of class
     * "skipped" with "-" in every other column but the species', and the call is not made for it.  Written only by a run that performs the strain step;
     * world_size > 1 or a sharded ingest with it is PANTAX_HIP_E_INVALID. */
    const char *strain_pair_evidence_file;
} pantax_hip_profiling_config;

/* A selection whose graphs hold more path steps than one resident db addresses (2^32: BASELINE configs[4] on one GPU) goes through the device in
 * groups of species, one after the other, inside the call -- no limit on the size of the DB other than the device memory a single group needs. */
int pantax_hip_profile(pantax_hip_ctx *ctx, const pantax_hip_profiling_config *cfg);

/* The sized extension of the pipeline seam.  pantax_hip_profiling_config keeps its size for the callers compiled against it: outputs added after
 * strain_pair_evidence_file are appended HERE, one field each, and reach the seam through pantax_hip_profile_with_ext.  struct_size is
 * sizeof(pantax_hip_profile_ext) as the caller's header has it: a field that does not lie wholly inside struct_size reads as off, so a caller built
 * against an older header keeps working against a newer library; struct_size below 8 or not a multiple of 8 is PANTAX_HIP_E_INVALID.  ext == NULL:
 * everything here is off, and pantax_hip_profile(ctx, cfg) is pantax_hip_profile_with_ext(ctx, cfg, NULL).  This struct is closed at strain_fit_file: later outputs are
 * fields of pantax_hip_profile_ext2 below. */
typedef struct {
    uint64_t struct_size;         /* sizeof(pantax_hip_profile_ext) as the caller's header has it */
    /* --strain-fit: path of the model fit report (pantax_hip_strain_fit over every group of species, right behind the group's evidence sums, on the same
     * coverage result; NULL, "" or "None" = off).  Sel_s = the species' rows of strain_abundance.txt, sel_w = their unrounded second_sol (the number the
     * evidence report prints as predicted_coverage).  TSV with a header, long format: species_taxid, strain_taxid, genome_ID, class, n_nodes, len, bases,
     * expected, excess, deficit, blind_nodes, blind_expected, fit, predicted_coverage.  First the strains in the order of strain_abundance.txt, classes
     * "all" then "private" each (predicted_coverage = the weight); then every species that went through a strain step, in the order the run took them,
     * classes "total", "explained", "orphan" with strain_taxid = genome_ID = "-"; "explained" is left out for a species without rows, its
     * predicted_coverage is the f64 sum of the species' weights in ascending haplotype index; predicted_coverage is "-" on total and orphan.
     * fit = 1 - (double)(excess + deficit) / (double)(bases + expected) (f64, shortest round-trip digits; "-" when bases + expected = 0): 1 where the
     * table reproduces the sample on these nodes, 0 where nothing coincides.  Written only by a run that performs the strain step; world_size > 1 or a
     * sharded ingest with it is PANTAX_HIP_E_INVALID. */
    const char *strain_fit_file;
} pantax_hip_profile_ext;
int pantax_hip_profile_with_ext(pantax_hip_ctx *ctx, const pantax_hip_profiling_config *cfg, const pantax_hip_profile_ext *ext);
/* The extension as it grows.  pantax_hip_profile_ext above is its first version and keeps ITS size too (compiled callers and a committed host check hold
 * its 16 bytes); the outputs behind strain_fit_file are the fields of the longer struct below, which BEGINS with the first version.  A caller fills
 * v1.struct_size = sizeof(pantax_hip_profile_ext2) and passes &ext2.v1 to pantax_hip_profile_with_ext: by the rule above the library reads every field
 * that lies wholly inside struct_size, so a caller with the 16-byte struct runs with the fields below off.  A later output is a field appended here. */
typedef struct {
    pantax_hip_profile_ext v1;    /* v1.struct_size = sizeof(pantax_hip_profile_ext2) */
    /* --strain-bootstrap: path of the bootstrap report (pantax_hip_strain_bootstrap over every group of species, right behind the group's model fit, on the
     * same coverage result; NULL, "" or "None" = off).  Sel_s = the species' rows of strain_abundance.txt, sp_key = the species taxid as a number (a taxid that
     * is no number: FNV-1a of its text).  TSV with a header: species_taxid, strain_taxid, genome_ID, class, predicted_coverage, refit, n_solved, mean, sd, q025,
     * q25, q50, q75, q975, min, zero_fraction, share, share_q025, share_q975, n_rows, objective; f64 in shortest round-trip digits, "-" where a column does not
     * apply or nothing was solved.  First the strains in the order of strain_abundance.txt, class "strain": predicted_coverage = the unrounded second_sol,
     * refit = x of replicate 0, n_solved .. zero_fraction = pantax_hip_bootstrap_summary over the replicates' x, share = refit / sum of the species' refits,
     * share_q025 / share_q975 from the same summary over x_k / sum_k x_k per solved replicate (a sum of 0 counts as 0).  Then every species that went
     * through a strain step and has rows in the table, in the order the run took them, class "species" ("skipped" for more than 64 rows): n_rows and
     * objective of replicate 0, n_solved, mean, sd, the quantiles and min over the replicates' objectives.  Same rules as strain_fit_file. */
    const char *strain_bootstrap_file;
    uint64_t strain_bootstrap_replicates;   /* 0 reads as 100; beyond 2^32 - 2: PANTAX_HIP_E_INVALID */
    uint64_t strain_bootstrap_seed;         /* a struct that does not hold the field reads as 42, the seed of the row sampler; the front ends default to 42 */
} pantax_hip_profile_ext2;
/* ... and once more: pantax_hip_profile_ext2 is closed at strain_bootstrap_seed (a committed host check holds its 40 bytes); the outputs behind it are the
 * fields of the struct below, which begins with the second version.  A caller fills v2.v1.struct_size = sizeof(pantax_hip_profile_ext3) and passes
 * &ext3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16- or 40-byte struct runs with the fields below off.  A later output is a field appended here. */
typedef struct {
    pantax_hip_profile_ext2 v2;   /* v2.v1.struct_size = sizeof(pantax_hip_profile_ext3) */
    /* --strain-dropout: path of the leave-one-out report (pantax_hip_strain_dropout over every group of species, right behind the group's bootstrap, on the
     * same coverage result; NULL, "" or "None" = off).  Sel_s = the species' rows of strain_abundance.txt in ascending haplotype index.  TSV with a header:
     * species_taxid, strain_taxid, genome_ID, class, predicted_coverage, refit, n_rows, objective, objective_without, delta, delta_fraction, n_member,
     * n_only, n_worse, n_better, substitute_strain_taxid, substitute_genome_ID, substitute_gain, shift; f64 in shortest round-trip digits, "-" where a
     * column does not apply.  First the strains in the order of strain_abundance.txt, class "strain": predicted_coverage = the unrounded second_sol,
     * refit = x of entry 0, n_rows and objective of entry 0, objective_without = the objective of the strain's entry k + 1, delta = objective_without -
     * objective, delta_fraction = delta / objective_without ("-" when that is 0), the four counts of entry k + 1, the substitute columns and shift from
     * pantax_hip_dropout_substitute ("-" when there is none; refit .. shift are "-" where entry 0 or entry k + 1 is not solved).  Then every species that went
     * through a strain step and has rows in the table, in the order the run took them, class "species" ("skipped" for more than 64 rows): n_rows and
     * objective, the rest "-".  Same rules as strain_fit_file. */
    const char *strain_dropout_file;
} pantax_hip_profile_ext3;
/* ... and once more: pantax_hip_profile_ext3 is closed at strain_dropout_file (a committed host check holds its 48 bytes); the outputs behind it are the
 * fields of the struct below, which begins with the third version.  A caller fills v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext4) and passes
 * &ext4.v3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16-, 40- or 48-byte struct runs with the fields below off.  A later output is a field
 * appended here. */
typedef struct {
    pantax_hip_profile_ext3 v3;   /* v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext4) */
    /* --strain-addin: path of the add-one report (pantax_hip_strain_addin over every group of species, right behind the group's leave-one-out test, on the
     * same coverage result; NULL, "" or "None" = off).  Sel_s = the species' rows of strain_abundance.txt in ascending haplotype index; Cand_s = the
     * candidates of the near-miss report (every haplotype of the species without a row), ranked by pantax_hip_near_miss_rank with top = strain_addin_top and
     * cut in rank order to 64 - K_s: a candidate without novel bases is not tested.  TSV with a header: species_taxid, strain_taxid, genome_ID, rank, class,
     * n_rows, objective, objective_with, gain, gain_fraction, coverage, n_member, n_novel, n_better, n_worse, donor_strain_taxid, donor_genome_ID,
     * donor_loss, shift, stage, unique_trio_nodes_fraction; f64 in shortest round-trip digits, "-" where a column does not apply.  Per species in the
     * order it went through the device its tested candidates in rank order, class "candidate": n_rows and objective of entry 0, objective_with = the
     * objective of the candidate's entry c + 1, gain = objective - objective_with, gain_fraction = gain / objective ("-" when that is 0), coverage = the
     * candidate's x under its own entry, the four counts of entry c + 1, the donor columns and shift from pantax_hip_addin_donor (strain_taxid and genome_ID of a
     * candidate and of a donor are those of the haplotype's first row of genomes_info.txt, as in the near-miss report; "-" when there is no donor;
     * n_rows .. shift are "-" where entry 0 or entry c + 1 is not solved), stage and unique_trio_nodes_fraction as the near-miss report prints them.
     * Then one row per species that has rows in the strain table or a tested candidate, in the same order, class "species" ("skipped" for more than 64
     * rows in the table): n_rows, objective and, in n_novel, the rows no reported strain walks (entry 0's second count); the rest "-".  Same rules as
     * strain_fit_file. */
    const char *strain_addin_file;
    uint64_t strain_addin_top;   /* candidates tested per species: 0 reads as 5, and so does a struct that does not hold the field */
} pantax_hip_profile_ext4;
/* ... and once more: pantax_hip_profile_ext4 is closed at strain_addin_top (a committed host check holds its 64 bytes); the outputs behind it are the fields
 * of the struct below, which begins with the fourth version.  A caller fills v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext5) and passes
 * &ext5.v4.v3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16-, 40-, 48- or 64-byte struct runs with the fields below off.  A later output is a
 * field appended here. */
typedef struct {
    pantax_hip_profile_ext4 v4;   /* v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext5) */
    /* --strain-em: path of the read class report (pantax_hip_strain_read_em over every group of species, right behind the group's read support call; NULL,
     * "" or "None" = off).  Candidates = the species' rows of strain_abundance.txt; G = the len of the strain's `all` class of pantax_hip_strain_evidence
     * (the distinct nodes it walks; the seam makes that call for this report too when strain_evidence_file is off); max_iter = strain_em_iterations,
     * tol = 1e-6.  TSV with a header: species_taxid, strain_taxid, genome_ID, class, rank, n_members, members, n_reads, n_steps, span, share, len,
     * em_coverage, em_bases, em_share, predicted_coverage, n_classes, n_iter, converged, delta; f64 in shortest round-trip digits, "-" where a column does
     * not apply.  First the strains in the order of strain_abundance.txt, class "strain": n_reads, n_steps, span summed over the classes that hold the
     * strain (= compatible of read support), len = G, em_coverage = x, em_bases = x * G, em_share = em_bases / the sum of em_bases over the species'
     * strains in ascending haplotype index ("-" when that is 0), predicted_coverage unrounded.  Then per species in the order it went through the device:
     * class "read_class", the first strain_em_classes classes by span descending, ties by mask ascending: rank from 1, n_members = the popcount, members =
     * the genome_IDs joined by "," in ascending haplotype index, share = span / the counted span ("-" when that is 0);  class "other", one row when the
     * species has more classes than printed, holding their sums (n_members = how many);  class "unexplained";  class "species" ("skipped" for more than 64
     * rows in the table): counted, n_classes, n_iter, converged, delta.  Same rules as strain_fit_file. */
    const char *strain_em_file;
    uint64_t strain_em_classes;      /* classes printed per species: 0 reads as 10, and so does a struct that does not hold the field */
    uint64_t strain_em_iterations;   /* max_iter: 0 reads as 1000, and so does a struct that does not hold the field; cut to 2^32 - 1 */
} pantax_hip_profile_ext5;
/* ... and once more: pantax_hip_profile_ext5 is closed at strain_em_iterations (a committed host check holds its 88 bytes); the outputs behind it are the
 * fields of the struct below, which begins with the fifth version.  A caller fills v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext6) and passes
 * &ext6.v5.v4.v3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16-, 40-, 48-, 64- or 88-byte struct runs with the fields below off.  A later output
 * is a field appended here. */
#define PANTAX_HIP_SEGMENTS_PEAK_OFF 0xFFFFFFFFFFFFFFFFull
typedef struct {
    pantax_hip_profile_ext5 v5;   /* v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext6) */
    /* --strain-segments: path of the segment report (pantax_hip_strain_segments over every group of species, right behind the group's strain step, beside
     * the coverage track and on the same selected haplotypes; NULL, "" or "None" = off).  Per row of strain_abundance.txt peak_depth = max(2, ceil(F x the
     * unrounded predicted_coverage)), clamped at 2^31 (F = strain_segments_peak; 0 when peaks are off).  The device is asked for the segments of at least
     * min(strain_segments_min, bridge + 1) bases and pantax_hip_segment_chain joins them per strain with `bridge` and min_span = strain_segments_min.  TSV
     * with a header: species_taxid, strain_taxid, genome_ID, class, rank, start, end, span, in_class, n_segments, n_nodes, bases, depth, fraction, threshold,
     * predicted_coverage; f64 in shortest round-trip digits, "-" where a column does not apply.  Per strain in the order of strain_abundance.txt: class
     * "strain" (span = G_h); "gap_total" and "peak_total" over ALL runs of the class (n_segments = n_runs, in_class = run_len, span = run_max, fraction =
     * run_len / G_h, "-" when G_h = 0; threshold = peak_depth on peak_total); then the kept chains in ascending start, class "gap" or "peak" with rank from 1
     * per class: start, end, span, in_class, n_segments, n_nodes = the steps, bases, depth = bases / in_class, fraction = in_class / span, threshold =
     * peak_depth on peak rows.  Same rules as strain_fit_file. */
    const char *strain_segments_file;
    uint64_t strain_segments_min;     /* min_span in bases: 0 reads as 1000, and so does a struct that does not hold the field */
    uint64_t strain_segments_bridge;  /* bridge + 1: 0 reads as a bridge of 100 bases, and so does a struct that does not hold the field; 1 = a bridge of 0 */
    uint64_t strain_segments_peak;    /* F: 0 reads as 10, and so does a struct that does not hold the field; PANTAX_HIP_SEGMENTS_PEAK_OFF = no peak class */
} pantax_hip_profile_ext6;
/* ... and once more: pantax_hip_profile_ext6 is closed at strain_segments_peak (a committed host check holds its 120 bytes); the outputs behind it are the
 * fields of the struct below, which begins with the sixth version.  A caller fills v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext7) and
 * passes &ext7.v6.v5.v4.v3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16-, 40-, 48-, 64-, 88- or 120-byte struct runs with the fields below off.
 * A later output is a field appended here. */
#define PANTAX_HIP_MOSAIC_TOP_OFF 0xFFFFFFFFFFFFFFFFull
typedef struct {
    pantax_hip_profile_ext6 v6;   /* v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext7) */
    /* --strain-mosaic: path of the mosaic read report (pantax_hip_strain_mosaic over every group of species, right behind the group's strain step, with
     * exactly the candidates and weights of read_strain_file; NULL, "" or "None" = off).  TSV with a header: species_taxid, strain_taxid, genome_ID, class,
     * n_reads, n_steps, span, n_segments, fraction, other_strain_taxid, other_genome_ID, node_a, node_b; f64 in shortest round-trip digits, "-" where a
     * column does not apply or a fraction has no denominator.  (1) per row of strain_abundance.txt, in its order, class "donor": n_segments and n_steps =
     * the segments of mosaic reads assigned to the strain and their steps, fraction = those steps / the steps of the species' mosaic reads.  (2) per
     * species in shard order: "counted", "compatible", "mosaic1", "mosaic2", "mosaic3plus", "foreign" with Q and fraction = n_reads / counted.n_reads
     * (foreign carries foreign_steps in n_segments), then "mosaic_total" = Q over the three mosaic classes with n_segments; a species without rows:
     * counted only; one of more than 64 rows: counted and "skipped".  (3) per pair of rows a < b (haplotype index) of a species with a break between
     * them, class "switch": a's strain columns, b in other_*, n_segments = pair[a][b] + pair[b][a], fraction = that / the species' n_breaks.  (4) per
     * species its strain_mosaic_top junctions by count (then node_a, node_b ascending), class "junction": node_a and node_b as the node ids of the GAF,
     * n_segments = the count, fraction = count / n_breaks.  Same rules as strain_fit_file. */
    const char *strain_mosaic_file;
    uint64_t strain_mosaic_top;   /* junctions printed per species: 0 reads as 10, and so does a struct that does not hold the field; PANTAX_HIP_MOSAIC_TOP_OFF = no junction rows, none collected */
} pantax_hip_profile_ext7;
/* ... and once more: pantax_hip_profile_ext7 is closed at strain_mosaic_top (a committed host check holds its 136 bytes); the outputs behind it are the
 * fields of the struct below, which begins with the seventh version.  A caller fills v7.v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext8) and
 * passes &ext8.v7.v6.v5.v4.v3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16-, 40-, 48-, 64-, 88-, 120- or 136-byte struct runs with the fields
 * below off.  A later output is a field appended here. */
typedef struct {
    pantax_hip_profile_ext7 v7;   /* v7.v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext8) */
    /* --strain-rescue: path of the read rescue report (pantax_hip_strain_read_rescue over every group of species, right behind the group's strain step;
     * NULL, "" or "None" = off).  Sel_s = the species' rows of strain_abundance.txt; Cand_s = the candidates of the near-miss report, first in the order
     * of pantax_hip_near_miss_rank with top = 0, then the remaining ones in ascending haplotype index (a candidate without novel bases can still rescue a
     * mosaic read), cut to 64 - K_s; a species of more than 64 rows is skipped.  TSV with a header: species_taxid, strain_taxid, genome_ID, rank, class,
     * n_reads, n_steps, span, fraction, alone_reads, foreign_reads, foreign_steps, claimed_steps, stage, unique_trio_nodes_fraction; f64 in shortest
     * round-trip digits, "-" where a column does not apply or a fraction has no denominator.  (1) per species in shard order its candidates in the order
     * of pantax_hip_rescue_rank with top = strain_rescue_top, rank from 1, class "candidate": Q of rescued, fraction = rescued.n_reads / (foreign +
     * mosaic).n_reads, alone.n_reads, from_foreign.n_reads, claimed_steps = cand_steps; strain_taxid, genome_ID, stage and unique_trio_nodes_fraction as
     * the near-miss report prints them.  (2) per species in shard order: "counted", "compatible", "foreign", "foreign_rescued", "foreign_patchwork",
     * "foreign_novel", "mosaic", "mosaic_rescued", "contested" with Q and fraction = n_reads / counted.n_reads; the foreign row carries foreign_steps and
     * claimed_steps, the foreign_novel row novel_steps in foreign_steps; a skipped species: "counted" and "skipped".  Same rules as strain_fit_file. */
    const char *strain_rescue_file;
    uint64_t strain_rescue_top;   /* candidates printed per species: 0 reads as 5, and so does a struct that does not hold the field */
} pantax_hip_profile_ext8;
/* ... and once more: pantax_hip_profile_ext8 is closed at strain_rescue_top (a committed host check holds its 152 bytes); the outputs behind it are the
 * fields of the struct below, which begins with the eighth version.  A caller fills v8.v7.v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext9)
 * and passes &ext9.v8.v7.v6.v5.v4.v3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16-, 40-, 48-, 64-, 88-, 120-, 136- or 152-byte struct runs
 * with the fields below off.  A later output is a field appended here. */
typedef struct {
    pantax_hip_profile_ext8 v8;   /* v8.v7.v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext9) */
    /* --strain-links: path of the link support report (pantax_hip_strain_links over every group of species, right behind the group's strain step, beside
     * the read rescue call; NULL, "" or "None" = off).  Sel_s = the species' rows of strain_abundance.txt; a species of more than 64 rows is skipped.  TSV
     * with a header: species_taxid, strain_taxid, genome_ID, class, rank, n_links, crossed, open, broken, private, private_crossed, private_broken,
     * support, crossed_fraction, start, node_a, node_b, flank_depth, shared_with, predicted_coverage; f64 in shortest round-trip digits, "-" where a
     * column does not apply or a fraction has no denominator.  (1) per row of strain_abundance.txt, in its order, a "strain" row with the eight numbers of
     * hap_out and crossed_fraction = crossed / links, then that strain's first strain_links_top breaks in the order of pantax_hip_link_top: class "break",
     * rank from 1, start, node_a and node_b (node ids as in the GAF), flank_depth, shared_with = popcount(brk_mask).  (2) per species in shard order:
     * "links" and "core" with n_links and crossed from link_out; then "crossings", "known", "skip", "switch", "foreign" with the count in support and its
     * share of crossings in crossed_fraction; a skipped species: "crossings" and "skipped".  Same rules as strain_fit_file. */
    const char *strain_links_file;
    uint64_t strain_links_top;   /* breaks printed per strain: 0 reads as 10, and so does a struct that does not hold the field */
} pantax_hip_profile_ext9;
/* ... and once more: pantax_hip_profile_ext9 is closed at strain_links_top (a committed host check holds its 168 bytes); the outputs behind it are the
 * fields of the struct below, which begins with the ninth version.  A caller fills v9.v8.v7.v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext10)
 * and passes &ext10.v9.v8.v7.v6.v5.v4.v3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16-, 40-, 48-, 64-, 88-, 120-, 136-, 152- or 168-byte struct
 * runs with the fields below off.  A later output is a field appended here. */
typedef struct {
    pantax_hip_profile_ext9 v9;   /* v9.v8.v7.v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext10) */
    /* --strain-rarefy: path of the rarefaction report (pantax_hip_strain_rarefy over every group of species, right behind the group's strain step, beside
     * the link support call; NULL, "" or "None" = off).  Sel_s = the species' rows of strain_abundance.txt in ascending haplotype index; a species of more
     * than 64 rows is skipped.  TSV with a header: species_taxid, strain_taxid, genome_ID, class, level, fraction, n_solved, predicted_coverage, refit, mean,
     * sd, min, max, scaled_mean, zero_fraction, n_member, n_only, n_reads, bases, n_rows, objective; f64 in shortest round-trip digits, "-" where a column
     * does not apply.  (1) per row of strain_abundance.txt, in its order, a "strain" row per level 0 .. strain_rarefy_levels: fraction = 2^-level; refit = x
     * of entry 0; n_solved, mean, sd, min and zero_fraction = pantax_hip_bootstrap_summary over the level's x of the replicates (level 0: the one value of
     * entry 0, n_solved = 1, sd = 0), max over the same solved LPs; scaled_mean = mean x 2^level, the number to read beside refit; n_member and n_only =
     * the means over the replicates, as f64.  (2) per species in shard order a "species" row per level: n_solved, n_reads and bases (means over the
     * replicates, as f64), n_rows (the mean over the replicates) and the mean objective of the solved LPs; a species of more than 64 rows: one "skipped" row
     * and no strain rows.  Same rules as
     * strain_fit_file. */
    const char *strain_rarefy_file;
    uint64_t strain_rarefy_levels;       /* thinned levels 1 .. N (fractions 1/2 .. 2^-N), at most 16: 0 reads as 5, and so does a struct that does not hold the field */
    uint64_t strain_rarefy_replicates;   /* replicates per level: 0 reads as 5, and so does a struct that does not hold the field */
    uint64_t strain_rarefy_seed;         /* a struct that does not hold the field reads as 42; 0 passed explicitly is 0 */
} pantax_hip_profile_ext10;
/* ... and once more: pantax_hip_profile_ext10 is closed at strain_rarefy_seed (a committed host check holds its 200 bytes); the outputs behind it are the
 * fields of the struct below, which begins with the tenth version.  A caller fills v10.v9.v8.v7.v6.v5.v4.v3.v2.v1.struct_size =
 * sizeof(pantax_hip_profile_ext11) and passes &ext11.v10.v9.v8.v7.v6.v5.v4.v3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16-, 40-, 48-, 64-,
 * 88-, 120-, 136-, 152-, 168- or 200-byte struct runs with the field below off.  A later output is a field appended here. */
typedef struct {
    pantax_hip_profile_ext10 v10;   /* v10.v9.v8.v7.v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext11) */
    /* --strain-fragments: path of the fragment support report (NULL, "" or "None" = off).  Key and tag of every GAF record by the rule of
     * pantax_hip_fragment_key, pantax_hip_fragment_mates once per run, and pantax_hip_strain_fragments over every group of species, right behind the
     * group's strain step and beside the rarefaction call, with the candidates and weights of read_strain_file (the rows of strain_abundance.txt, their
     * unrounded predicted_coverage).  TSV with a header: species_taxid, strain_taxid, genome_ID, class, n_fragments, n_reads, n_steps, span, fraction,
     * other_strain_taxid, other_genome_ID; f64 in shortest round-trip digits, "-" where a column does not apply.  (1) per row of strain_abundance.txt, in
     * its order: "compatible", "unique", "unique_by_pair", "assigned" with fraction over the species' paired fragments (n_reads = 2 n_fragments);
     * (2) per species in shard order the nine classes, fraction = n_reads over the counted reads (the read classes have "-" in n_fragments, the fragment
     * classes n_reads = 2 n_fragments; a species of more than 64 rows prints counted, paired, single, multi, mate_elsewhere and one "skipped" row);
     * (3) per species one "discordant_pair" row per pair a < b of its rows (ascending haplotype index) with a non-zero count: strain a in the strain
     * columns, strain b in other_*, fraction over the species' discordant fragments.  Same rules as strain_fit_file. */
    const char *strain_fragments_file;
} pantax_hip_profile_ext11;
/* ... and once more: pantax_hip_profile_ext11 is closed at strain_fragments_file (a committed host check holds its 208 bytes); the outputs behind it are the
 * fields of the struct below, which begins with the eleventh version.  A caller fills v11.v10.v9.v8.v7.v6.v5.v4.v3.v2.v1.struct_size =
 * sizeof(pantax_hip_profile_ext12) and passes &ext12.v11.v10.v9.v8.v7.v6.v5.v4.v3.v2.v1 to pantax_hip_profile_with_ext; a caller with a 16-, 40-, 48-, 64-,
 * 88-, 120-, 136-, 152-, 168-, 200- or 208-byte struct runs with the fields below off.  A later output is a field appended here. */
typedef struct {
    pantax_hip_profile_ext11 v11;   /* v11.v10.v9.v8.v7.v6.v5.v4.v3.v2.v1.struct_size = sizeof(pantax_hip_profile_ext12) */
    /* --strain-growth: path of the replication index report (pantax_hip_strain_growth over every group of species, right behind the group's strain step
     * and beside the coverage track, then pantax_hip_growth_fit per row with min_own = max(1, W x strain_growth_min_own_permille / 1000), min_windows =
     * PANTAX_HIP_GROWTH_MIN_WINDOWS and min_depth = PANTAX_HIP_GROWTH_MIN_DEPTH; NULL, "" or "None" = off).  The selection of a species is its rows of
     * strain_abundance.txt.  TSV with a header, one row per row of strain_abundance.txt, in its order: species_taxid, strain_taxid, genome_ID, window,
     * n_windows, n_kept, n_zero, n_fit, own_len, own_fraction (own_len / G_h), median_depth, slope, intercept, r2, index, status, predicted_coverage; f64 in
     * shortest round-trip digits.  Same rules as strain_coverage_file: world_size > 1 or a sharded ingest with it is PANTAX_HIP_E_INVALID; a run without
     * a strain step writes nothing and says so on stderr. */
    const char *strain_growth_file;
    uint64_t strain_growth_window;             /* W in bases: 0 reads as 5000, and so does a struct that does not hold the field */
    uint64_t strain_growth_min_own_permille;   /* own bases a window needs, in thousandths of W (1 .. 1000): 0 reads as 500 */
    uint64_t strain_growth_trim_permille;      /* windows trimmed from each end of the sorted range, in thousandths (below 500): 0 reads as 100 */
} pantax_hip_profile_ext12;

/* ---- the --db-pairs mode: pairwise strain distinguishability of a db as one table (pantax_hip_db_hap_pairs over every haplotype of the chosen species).
 * Files in, one file out: no GAF, no work directory, no strain step; one rank.  The species are those named in `species`, or by default every species of
 * the range file with more than one haplotype, in range-file order; an unknown taxid is PANTAX_HIP_E_INVALID.  Their graphs are read with the host
 * loaders by the file seam's choice of container (<db>/species_graph_info/<otu>.bin, .bin.lz4, .bin.zst per `zip`, else <db>/species_gfa/<otu>.gfa; images
 * are not used) and go through the device in groups: a group ends before the species that would carry it past the path steps of one resident db (3e9, or
 * the option db_path_steps_max) or past its node indices.  A species of more than 256 haplotypes is not computed (a `skipped` row, one line on stderr).
 * TSV with a header: species_taxid, genome_ID_a, genome_ID_b, class, n_nodes_a, len_a, n_nodes_b, len_b, shared_nodes, shared_len, only_a_len, only_b_len,
 * distance, jaccard.  Pair rows first, per species in that order, a < b in haplotype-index order, only those of distance <= max_distance when that is >= 0:
 * genome_ID = the genome_ID of the haplotype's first row of <db>/genomes_info.txt (the strain table's join), the haplotype's own name without one;
 * { n_nodes, len } of a and b = the diagonal; shared = pair[a][b]; only_a_len, only_b_len and distance as defined at pantax_hip_db_hap_pairs;
 * class = "identical" (distance 0: the LP cannot separate them), "nested" (exactly one of only_a_len, only_b_len is 0: one strain has nothing of its own
 * against the other) or "distinct"; jaccard = shared_len / (len_a + len_b - shared_len) as f64 with shortest round-trip digits, "-" when that is 0.
 * Then one row per species, in the same order: class "species", genome_ID_a = the number of haplotypes, genome_ID_b = "-", n_nodes_a / len_a = total,
 * shared_nodes / shared_len = core, distance = the smallest distance over ALL the species' pairs ("-" for a single haplotype), every other column "-"; or
 * class "skipped" for a species over the limit, with the number of haplotypes and "-" elsewhere. */
typedef struct {
    const char *db;              /* -db: the database directory */
    const char *out_file;        /* --db-pairs: the table */
    const char *range_file;      /* --range-file, or NULL: <db>/species_range.txt */
    const char *species;         /* --db-pairs-species: taxids separated by commas; NULL or "" = every species with more than one haplotype */
    const char *zip;             /* --zip serialize | lz | zstd; NULL (--gfa) = GFA text */
    int64_t max_distance;        /* --db-pairs-max-distance in bases; negative = every pair */
} pantax_hip_db_pairs_config;
int pantax_hip_db_pairs(pantax_hip_ctx *ctx, const pantax_hip_db_pairs_config *cfg);

/* ---- a1 / a6 host readers (no GPU needed): the file contracts of the pipeline seam, exposed so a
 * caller that keeps its own orchestration can still reuse the tokenizer and graph loaders ---------- */
typedef struct pantax_hip_gaf pantax_hip_gaf;     /* owns the packed arrays of one tokenised GAF */
/* load_gaf_file_lazy (rcls.rs:119-146): columns 1,2,6,7,8,9,12; '@' comment lines and empty lines skipped; "*" AND the
 * empty field = null (the reader's null_values / missing_is_null; => PANTAX_HIP_READ_NULLFIELD for cols 6-9, mapq 255,
 * qlen 0); a non-integer in an integer column reads as null; integers above 2^32 - 1 are clamped to it (32-bit packed
 * columns).  The rules are restated, independently of this library, in oracle/gaf_reader.py, which the tests compare
 * every tokenizer with.  err_out (may be NULL) receives a static/thread-local message on failure. */
int pantax_hip_gaf_load(const char *path, int n_threads, pantax_hip_gaf **out, const char **err_out);
/* the same tokenisation on the device (text uploaded once, five launches): identical arrays.  LIMIT of the
 * device readers (this entry, pantax_hip_reads_load_gaf, pantax_hip_gaf_filter): the text travels in pieces cut at line
 * ends -- a sixth of the text, 64 MiB .. 1 GiB, less only through PANTAX_GAF_PIECE_BYTES -- and a piece holds whole lines:
 * ONE LINE longer than 3.5 GiB (or than a lowered piece size) is refused with PANTAX_HIP_E_LIMIT.  A HiFi / ONT line with
 * a long cs tag is kilobytes to megabytes: far inside the default. */
int pantax_hip_gaf_load_device(pantax_hip_ctx *ctx, const char *path, pantax_hip_gaf **out);
int pantax_hip_gaf_view(const pantax_hip_gaf *gaf, pantax_hip_packed_reads *view_out);
/* What a tokenizer knows about the read ids, and which route the device tokenizer took (read-only; the arrays live as long as the handle).
 * id_hash = FNV-1a-64 of the id bytes with the final avalanche h ^= h >> 32; h *= 0xd6e8feb86659fd93; h ^= h >> 32 (the key of the
 * duplicate-id rule, profile.rs:361-437).  The route fields are there for tests: they tell which path a given text was tokenised on and
 * change nothing.  The first call on a handle that kept id spans copies them into id_off / id_len: not to be raced from two threads. */
typedef struct {
    uint64_t n_reads;
    const uint64_t *id_hash;  /* [R] */
    const uint64_t *id_off;   /* [R] where the id starts in the file; NULL when the spans were not kept (pantax_hip_reads_load_gaf) */
    const uint32_t *id_len;   /* [R] its length in bytes; NULL when the spans were not kept */
    int32_t ids_distinct;     /* 1 = no two reads share an id hash, 0 = some do, -1 = not checked (host tokenizer, empty text) */
    int32_t id_check;         /* who decided ids_distinct: 0 = nobody (host tokenizer, fewer than two reads), 1 = the hash set filled piece by
                               * piece, 2 = the sort of all hashes behind the last piece (the set was sized too small for the text) */
    uint32_t n_pieces;        /* pieces the device tokenizer cut the text into (host tokenizer: 0) */
    uint32_t n_grow_r;        /* times the joined per-read columns were enlarged with reads already in them */
    uint32_t n_grow_t;        /* the same for the joined step column with steps already in it */
} pantax_hip_gaf_ids_view;
int pantax_hip_gaf_ids(const pantax_hip_gaf *gaf, pantax_hip_gaf_ids_view *view_out);
/* file -> packed reads RESIDENT in HBM, tokenised on the device, ready for pantax_hip_bin_reads; the walks never
 * visit the host.  The text travels in pieces on an upload stream (pread into a pinned ring on a few host threads) while the
 * piece before is tokenised.  gaf_out (optional) receives the host-side columns (read_len, mapq, flags; its view has
 * node_id / step_off / pstart / pend = NULL); with gaf_out == NULL those columns are not brought back at all. */
int pantax_hip_reads_load_gaf(pantax_hip_ctx *ctx, const char *path, pantax_hip_reads **reads_out, pantax_hip_gaf **gaf_out);
/* replace the per-read drop flags of resident reads (a5: null fields, duplicate ids); NULL clears them.  The reads
 * must be binned again afterwards. */
int pantax_hip_reads_set_flags(pantax_hip_ctx *ctx, pantax_hip_reads *reads, const uint8_t *flags);
void pantax_hip_gaf_free(pantax_hip_gaf *gaf);

typedef struct pantax_hip_graph pantax_hip_graph; /* one species graph in `Graph` shape (types.rs:51-55) */
/* format 0 = GFA S/W/P lines (read_gfa, profile.rs:466-545), 1 = bincode-1 .bin (zip.rs:236-247),
 * 2 = .bin.lz4 (LZ4 frame), 3 = .bin.zst (zip.rs:250-265; liblz4.so.1 / libzstd.so.1 are bound at run time) */
int pantax_hip_graph_load(const char *path, int format, pantax_hip_graph **out, const char **err_out);
/* sizes: n_nodes, n_haps, n_steps; arrays are valid until graph_free; hap_names_out[i] NUL-terminated */
int pantax_hip_graph_view(const pantax_hip_graph *g, uint64_t *n_nodes, uint64_t *n_haps, const int64_t **node_len,
                          const uint64_t **path_off, const uint32_t **path_nodes, const char *const **hap_names);
void pantax_hip_graph_free(pantax_hip_graph *g);

/* the float text of the two tables (polars CsvWriter behind rcls.rs:409-420: shortest round-trip digits, "16.0" for integral
 * values; exemplar rows README.md:343, :354).  Host only.  Returns the length, or < 0. */
int pantax_hip_format_f64(double v, char *buf, size_t cap);

/* The per-species node statistics of the strain step collected last on this db (pantax_hip_strain_profile, pantax_hip_profile_step,
 * pantax_hip_profile_step_collect), as the device left them: max node abundance, nodes with abundance > 0, and the unrounded sum / count of the
 * abundances above min_depth (frequencies_mean of a single-path species is their rounded quotient).  Host copies only; any output may be NULL.
 * PANTAX_HIP_E_STATE before the first collected step, and while enqueued steps of the db are not yet collected. */
int pantax_hip_strain_node_stats(pantax_hip_ctx *ctx, pantax_hip_db *db, double *amax_out, uint32_t *nvalid_out, double *nzsum_out,
                                 uint32_t *nzcnt_out);

/* The per-haplotype unique-trio statistics (a9) of the same step, under the same contract: the number of unique-trio windows with an abundance > 0
 * and the unrounded mean of those that pass the z-score filter (0.0 where the standard deviation is 0), for every haplotype of the db -- those
 * the first filter dropped included; zeros for the haplotypes of a species the step skipped.  [H] each; either output may be NULL. */
int pantax_hip_strain_hap_stats(pantax_hip_ctx *ctx, pantax_hip_db *db, uint32_t *nnz_out, double *mean_filtered_out);

/* The per-node results of the same step when it went through the split node pass (option node_pass=split, or a step that is not eligible for the
 * fused pass): the covered bases of every node (node_base_cov) and the node abundances bases / length, [V] each, as the device holds them.  When the
 * step sampled rows (sample_nodes), a11 has edited `ab`: the nodes it did not choose read 0.  The call synchronises and copies; it launches nothing.
 * PANTAX_HIP_E_STATE before the first collected step, while enqueued steps are not yet collected, when the step collected last took the fused node
 * pass (which stores neither array), and once a later pantax_hip_node_coverage has counted the covered bases itself.  Either output may be NULL. */
int pantax_hip_strain_node_cov(pantax_hip_ctx *ctx, pantax_hip_db *db, uint32_t *cov_out, double *ab_out);

/* ---- measurement: HIP-event timings of kernels launched on the ctx stream ---------------- */
int pantax_hip_timing_enable(pantax_hip_ctx *ctx, int on);
int pantax_hip_timing_reset(pantax_hip_ctx *ctx);
/* name != NULL/"": bracket only launches of that kernel, or of several ("a|b") (the event pairs of ~100 launches per step cost
 * ~0.15 ms; a throughput measurement that also wants one kernel's duration times just that one) */
int pantax_hip_timing_filter(pantax_hip_ctx *ctx, const char *name);
/* fills up to cap entries; returns the number of distinct kernel names (or <0) */
int pantax_hip_timing_get(pantax_hip_ctx *ctx, int cap, const char **names_out, uint64_t *launches_out,
                          double *total_ms_out);
int pantax_hip_sync(pantax_hip_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
