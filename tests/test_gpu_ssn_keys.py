"""The node-order row sort stores a row's key words (species / mask) only where something reads them (option ssn_keys, sample_sort_nodes.hip): in a
resident step the sorted rows' one reader of the keys is ssn_heads_kernel, which looks at the mixed bucket pairs alone, and the step keeps the abundances.
Every case runs one resident step four ways -- ssn_keys=all, =needed, =needed with the key buffers filled with 0xA5 bytes first (ssn_poison_keys: a read of
a word the sort did not store shows), =needed with the tie fill on the side stream (ssn_ties_async=1) -- and asserts the same tables and statistics from
all four, element for element, and the oracle's passing rows the way tests/test_gpu_row_route.py compares them.  The poisoned variant also runs as the FIRST
step of a fresh Engine: the sort buffers outlive a step, and an earlier ssn_keys=all step would have left correct masks behind.

The shapes (SETS) are the smallest that reach each path; test_the_sets_are_what_the_cases_need asserts that they do:
  "main": a species of more than 4096 nodes (SN_SAMPLE) and many candidate columns of different membership (20 haplotypes, present_frac 0.7: several
          splitter pairs change the mask); one of more than 4096 nodes with exactly ONE candidate column (every splitter has one mask: pair 0 and the last
          pair alone are scanned); multi-haplotype species of at most 4096 nodes and a one-haplotype species of a few dozen nodes (the small path: all
          words kept); a species the species level drops (avg_len = 0) and one without reads (no rows).
  "w64":  a db that holds a species of 64 haplotypes: row_pack_shift goes negative and the rows are three words (ksp), with a species of more than 4096
          nodes beside it.
Not here: a species of >= 2e5 rows with few distinct abundances, to reach ssn_local_wave2_kernel and the big-bucket paths of ssn_local_kernel.  Evenly spaced
samples of such a segment are representative (the largest even bucket stays near 2 n / 1024 < 512 rows below 2.6e5 rows), so it would take about 1e6 nodes,
and the oracle's LPs for them take minutes, not seconds.  Those paths store through the same Sn::put_if(mixed, ...) as the wave kernel; tests/test_gpu_parity.py
forces them through pantax_hip_sort_rows (every key word stored), and bench.py's output comparison against the previous commit runs them at full size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# seed, (haplotypes, genome length[, fraction of the strains present]) per species, reads, the species dropped by avg_len = 0, the species without reads
SETS = {"main": (20261101, [(5, 120000), (4, 100000), (1, 40000), (3, 160000, 0.2), (20, 150000, 0.7), (6, 50000), (2, 50000)], 120000, 1, 6),
        "w64": (20261102, [(5, 150000), (64, 40000), (3, 50000)], 40000, None, None)}

# the four ways; "all" is the reference of the other three
VARIANTS = [("all", {"ssn_keys": "all"}),
            ("needed", {"ssn_keys": "needed"}),
            ("needed_poisoned", {"ssn_keys": "needed", "ssn_poison_keys": "1"}),
            ("needed_ties_async", {"ssn_keys": "needed", "ssn_ties_async": "1"})]
STATS = ("obj", "iters", "n_rows", "n_cand", "n_patterns")


@pytest.fixture(scope="module")
def world():
    """set key -> (set, avg_len, the oracle's kept species, its passing strain rows): made once, shared by the tests, never changed"""
    import synthdata as synth
    from oracle import oracle as orc
    from tests.helpers import oracle_strain_level, oracle_passing_rows
    made = {}

    def get(key):
        if key not in made:
            seed, spec, n_reads, dropped, readless = SETS[key]
            rng = np.random.default_rng(seed)
            species, start = [], 1
            for s, (h, gl, *pf) in enumerate(spec):
                g = synth.make_species(rng, str(1000 + s), h, gl, start, "GCF_%06d" % (s + 1), present_frac=pf[0] if pf else 0.4)
                species.append(g)
                start = g.range_end + 1
            sset = synth.SyntheticSet(species, synth.make_reads(rng, [g for s, g in enumerate(species) if s != readless], n_reads))
            avg = np.array(sset.avg_len(), dtype=np.float64)
            if dropped is not None:
                avg[dropped] = 0.0               # a species without a genome length is dropped by the species level (profile.rs:329)
            rd, S = sset.reads, len(species)
            sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in species], [g.range_end for g in species])
            keep, absolute, abundance = orc.species_profile(sp, rd.qlen, orc.species_counts(sp, rd.qlen, rd.mapq, S), avg)
            level = oracle_strain_level(sset, sp, keep, absolute, [s for s in range(S) if abundance[s] > 1e-4], threads=8)
            made[key] = (sset, avg, {species[s].name for s in range(S) if keep[s]}, oracle_passing_rows(sset, level))
        return made[key]
    return get


def one_step(eng, sset, avg, options):
    from pantax_amd.pipeline import StepConfig, profile_step
    eng.set_option("row_sort", "nodes")
    for name in ("ssn_keys", "ssn_poison_keys", "ssn_ties_async"):
        eng.set_option(name, options.get(name))   # None: the default
    try:
        eng.upload_db(sset.species)
        eng.upload_packed(sset.reads)
        return profile_step(eng, [g.name for g in sset.species], [h for g in sset.species for h in g.hap_names], avg, StepConfig())
    finally:
        for name in ("row_sort", "ssn_keys", "ssn_poison_keys", "ssn_ties_async"):
            eng.set_option(name, None)


def assert_same_step(got, ref, what):
    assert got[0] == ref[0], what + ": species rows"
    assert got[1] == ref[1], what + ": strain rows"
    for k in STATS:
        a, b = np.asarray(got[2][k], dtype=np.float64), np.asarray(ref[2][k], dtype=np.float64)
        assert np.array_equal(a, b, equal_nan=True), (what, k)


@pytest.fixture(scope="module")
def steps(world):
    """set key -> {variant: (species rows, strain rows, stats)}: the four steps of a set, on one Engine in the order of VARIANTS, run once"""
    from pantax_amd.engine import Engine
    done = {}

    def get(key):
        if key not in done:
            sset, avg, _, _ = world(key)
            with Engine(0) as eng:
                done[key] = {name: one_step(eng, sset, avg, options) for name, options in VARIANTS}
        return done[key]
    return get


def test_the_sets_are_what_the_cases_need(world, steps):
    sset, _, kept, _ = world("main")
    st = steps("main")["all"][2]
    nodes = [g.n_nodes for g in sset.species]
    print("main: nodes", nodes, "n_cand", st["n_cand"], "n_rows", st["n_rows"], "n_patterns", st["n_patterns"])
    assert sum(nodes) <= 600000                                                        # (the option, not the size, puts the rows on the node sort)
    big = [s for s in range(len(nodes)) if nodes[s] > 4096 and st["n_rows"][s] > 4096]
    assert any(st["n_cand"][s] >= 3 and st["n_patterns"][s] >= 4 for s in big)        # masks change between splitters
    assert any(st["n_cand"][s] == 1 and st["n_patterns"][s] == 1 for s in big)        # one mask: only pair 0 and the last pair are scanned
    assert any(nodes[s] <= 4096 and st["n_cand"][s] >= 2 and st["n_rows"][s] > 0 for s in range(len(nodes)))   # the small path, several masks
    assert sset.species[1].name not in kept and st["n_rows"][1] == 0                  # dropped by the species level
    assert sset.species[6].name not in kept and st["n_rows"][6] == 0                  # no reads
    w64, _, _, _ = world("w64")
    sw = steps("w64")["all"][2]
    print("w64: nodes", [g.n_nodes for g in w64.species], "n_cand", sw["n_cand"], "n_rows", sw["n_rows"], "n_patterns", sw["n_patterns"])
    assert sorted(g.n_paths for g in w64.species) == [3, 5, 64]                       # 64 mask bits: no room for the species in the mask word
    assert w64.species[0].n_nodes > 4096 and sw["n_rows"][0] > 4096 and sw["n_patterns"][0] >= 2
    assert sw["n_rows"][1] > 0 and sw["n_patterns"][1] >= 2


@pytest.mark.parametrize("key", sorted(SETS))
@pytest.mark.parametrize("variant", [v[0] for v in VARIANTS])
def test_step_tables(world, steps, key, variant):
    from tests.helpers import check_step_rows_against_oracle
    _, _, kept, passing = world(key)
    got = steps(key)[variant]
    assert {r[0] for r in got[0]} == kept
    assert len(passing) >= 2 and any(len(rows) > 1 for rows in passing.values())
    check_step_rows_against_oracle(got[1], passing)
    assert_same_step(got, steps(key)["all"], "%s/%s against ssn_keys=all" % (key, variant))


@pytest.mark.parametrize("key", sorted(SETS))
def test_poisoned_first_step_of_a_fresh_engine(world, steps, key):
    """no earlier step has written the sort buffers: every key word the heads kernel reads is this sort's own, or 0xA5 bytes"""
    from pantax_amd.engine import Engine
    from tests.helpers import check_step_rows_against_oracle
    sset, avg, kept, passing = world(key)
    with Engine(0) as eng:
        got = one_step(eng, sset, avg, dict(VARIANTS)["needed_poisoned"])
    assert {r[0] for r in got[0]} == kept
    check_step_rows_against_oracle(got[1], passing)
    assert_same_step(got, steps(key)["all"], "%s/needed_poisoned, fresh engine, against ssn_keys=all" % key)


def test_needed_without_pattern_tables_is_refused(set_opt):
    """pantax_hip_sort_rows returns the keys: ssn_keys=needed is an error there, and the default stores them all (tests/test_gpu_parity.py)"""
    from pantax_amd.engine import Engine
    rng = np.random.default_rng(7)
    n = 20000
    k0 = np.zeros(n, dtype=np.uint64)
    k1 = rng.integers(1, 8, size=n).astype(np.uint64)
    k2 = rng.integers(1, 50, size=n).astype(np.float64).view(np.uint64)
    with Engine(0) as eng:
        set_opt(eng, "ssn_keys", "needed")
        with pytest.raises(Exception):
            eng.sort_rows(k0, k1, k2, algo=4)
        set_opt(eng, "ssn_keys", "sometimes")
        with pytest.raises(Exception):
            eng.sort_rows(k0, k1, k2, algo=4)
