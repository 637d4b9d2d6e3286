"""Which route the LP rows of a resident step take (row_route / lad_prepare, node_pass_fused_eligible), pinned by the library's timer labels: every case
runs one resident step, compares its tables with the oracle's and then asserts WHICH of the six launches that tell the routes apart ran and which did not.
A label names a bracket, not a kernel symbol: the mask pass is bracketed once, as mask_nodes_kernel wherever the node -> haplotype words exist (the path
walk for a species of more than 64 haplotypes then runs inside that bracket) and as mask_kernel only where they do not (option mask=walk)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LABELS = {"node_rows_kernel", "node_cov_stats_kernel", "mask_nodes_kernel", "mask_kernel", "ratio_kernel", "row_emit_kernel"}

# (haplotypes, genome length[, fraction of the strains present]) per species: the set of tests/test_gpu_node_pass.py (every species at most 64 haplotypes,
# short nodes: the fused node pass is open to it), and a small one with one species of 65 haplotypes among ordinary ones (the wide route)
SETS = {"narrow": (20261016, [(5, 120000), (4, 100000), (1, 40000), (3, 60000), (20, 150000, 0.7), (6, 66000), (2, 50000)], 120000, 1),
        "wide": (20261018, [(5, 60000), (65, 40000), (3, 50000)], 40000, None)}

# id, set, library options, sample_nodes (a11), the labels of LABELS that appear -- all others of LABELS must not
CASES = [
    # below the sample-sort limit the rows are compacted and sorted whole; the masks come from the by-node pass, which sums path_cov_ratio on its way
    ("defaults", "narrow", {}, 0, {"node_cov_stats_kernel", "mask_nodes_kernel", "row_emit_kernel"}),
    # the node sort: masks formed inside it, and the fused node pass in place of the statistics kernel
    ("nodes", "narrow", {"row_sort": "nodes"}, 0, {"node_rows_kernel"}),
    ("nodes_split", "narrow", {"row_sort": "nodes", "node_pass": "split"}, 0, {"node_cov_stats_kernel"}),
    ("nodes_mask_pass", "narrow", {"row_sort": "nodes", "mask_pass": "1"}, 0, {"node_cov_stats_kernel", "mask_nodes_kernel"}),
    ("nodes_ratio_kernel", "narrow", {"row_sort": "nodes", "ratio_kernel": "1"}, 0, {"node_cov_stats_kernel", "mask_nodes_kernel", "ratio_kernel"}),
    # a11 edits the abundances in front of the sort: no fused pass, the masks still formed in the sort
    ("nodes_sampled", "narrow", {"row_sort": "nodes"}, 1000, {"node_cov_stats_kernel"}),
    # a species of 65 haplotypes: its masks come from the path walk (inside the mask pass's bracket) and its ratio sums from ratio_kernel; no fused pass for the db
    ("nodes_wide", "wide", {"row_sort": "nodes"}, 0, {"node_cov_stats_kernel", "mask_nodes_kernel", "ratio_kernel"}),
    # "radix" keeps the rows off the node sort; a db this small still takes the sample sort behind the compaction
    ("radix", "narrow", {"row_sort": "radix"}, 0, {"node_cov_stats_kernel", "mask_nodes_kernel", "row_emit_kernel"}),
    # without the node -> haplotype words every mask comes from the path walk and every ratio sum from ratio_kernel
    ("mask_walk", "narrow", {"mask": "walk"}, 0, {"node_cov_stats_kernel", "mask_kernel", "ratio_kernel", "row_emit_kernel"}),
]
# the two fused scans of the step -- the pattern tables behind a whole-row sort (Pat), the a11 sampling (Sample, bracketed as row_sample_kernel) -- again under
# the 8192- and the 16384-item tile, which the size rule takes only from 2^22 / 2^26 items on (option scan_tile, scan_chained.hpp): same routes, same tables
SCAN_LABEL = {"defaults": "scan_chained_kernel<Pat>", "nodes_sampled": "row_sample_kernel"}
CASES += [("%s_scan_%s" % (name, tile), key, dict(options, scan_tile=tile), sample_nodes, expected)
          for tile in ("big", "huge") for name, key, options, sample_nodes, expected in CASES if name in SCAN_LABEL]


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world():
    """set key -> (set, avg_len); (set key, sample_nodes) -> the oracle's species rows and passing strain rows: made once, shared by the cases, never changed"""
    import synthdata as synth
    from oracle import oracle as orc
    from tests.helpers import oracle_strain_level, oracle_passing_rows
    sets, refs = {}, {}

    def get_set(key):
        if key not in sets:
            seed, spec, n_reads, dropped = SETS[key]
            rng = np.random.default_rng(seed)
            species, start = [], 1
            for s, (h, gl, *pf) in enumerate(spec):
                g = synth.make_species(rng, str(1000 + s), h, gl, start, "GCF_%06d" % (s + 1), present_frac=pf[0] if pf else 0.4)
                species.append(g)
                start = g.range_end + 1
            sset = synth.SyntheticSet(species, synth.make_reads(rng, species, n_reads))
            avg = np.array(sset.avg_len(), dtype=np.float64)
            if dropped is not None:
                avg[dropped] = 0.0               # a species without a genome length is dropped by the species level (profile.rs:329)
            sets[key] = (sset, avg)
        return sets[key]

    def get_ref(key, sample_nodes):
        if (key, sample_nodes) not in refs:
            sset, avg = get_set(key)
            rd, S = sset.reads, len(sset.species)
            sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in sset.species], [g.range_end for g in sset.species])
            keep, absolute, abundance = orc.species_profile(sp, rd.qlen, orc.species_counts(sp, rd.qlen, rd.mapq, S), avg)
            level = oracle_strain_level(sset, sp, keep, absolute, [s for s in range(S) if abundance[s] > 1e-4], threads=8, sample_nodes=sample_nodes)
            refs[(key, sample_nodes)] = ({sset.species[s].name for s in range(S) if keep[s]}, oracle_passing_rows(sset, level))
        return refs[(key, sample_nodes)]
    return get_set, get_ref


def test_the_sets_are_what_the_cases_need(world):
    get_set, _ = world
    narrow, _ = get_set("narrow")
    assert max(g.n_paths for g in narrow.species) <= 64
    assert sum(int(g.node_len.sum()) for g in narrow.species) // sum(g.n_nodes for g in narrow.species) < 48   # (not the long-node variant of the statistics pass)
    assert max(g.n_nodes for g in narrow.species) > 1000                                                       # a11 at 1000 rows samples
    wide, _ = get_set("wide")
    assert sorted(g.n_paths for g in wide.species) == [3, 5, 65]
    for sset in (narrow, wide):
        assert sum(g.n_nodes for g in sset.species) <= 600000                                                  # below the sample-sort limit


@pytest.mark.parametrize("name,key,options,sample_nodes,expected", CASES, ids=[c[0] for c in CASES])
def test_route_and_tables(eng, world, set_opt, name, key, options, sample_nodes, expected):
    from pantax_amd.pipeline import StepConfig, profile_step
    from tests.helpers import check_step_rows_against_oracle
    get_set, get_ref = world
    sset, avg = get_set(key)
    kept, passing = get_ref(key, sample_nodes)
    for opt, value in options.items():
        set_opt(eng, opt, value)
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    names = [g.name for g in sset.species]
    haps = [h for g in sset.species for h in g.hap_names]
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        sp_rows, st_rows, stats = profile_step(eng, names, haps, avg, StepConfig(sample_nodes=sample_nodes))
        ran = set(eng.timing_get())
    finally:
        eng.timing_enable(False)
    print("%s: %s" % (name, sorted(ran & LABELS)))
    assert {r[0] for r in sp_rows} == kept
    assert len(passing) >= 2 and any(len(rows) > 1 for rows in passing.values())
    check_step_rows_against_oracle(st_rows, passing)
    if sample_nodes:
        assert max(stats["n_rows"]) == sample_nodes          # (a11 really sampled)
    assert ran & LABELS == expected, sorted(ran & LABELS)
    if "scan_tile" in options:
        assert SCAN_LABEL[name.split("_scan_")[0]] in ran, sorted(ran)
