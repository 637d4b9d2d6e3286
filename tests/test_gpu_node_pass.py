"""The resident step's fused node pass (node_rows_kernel: node statistics + LP rows in ONE pass over the nodes) against the two kernels it
replaces (option node_pass=split: node_cov_stats_kernel + ssn_hist_kernel<true>), in one process on the same inputs, and against the oracle.

What must hold (the rows and patterns the solver sees are the same bytes on both paths):
  * every integer and every LP quantity of the step's outputs is EXACTLY equal: species decisions, metrics, solve info, amax / nvalid / nzcnt;
  * nzsum -- an f64 sum whose order follows the launch geometry -- within 1e-12 relative: a few thousand to a few hundred thousand positive
    terms of similar size, so a pairwise / blocked sum is good to ~1e-15 and a miss means a wrong sum, not rounding; frequencies_mean and the
    divergence derived from it are equal after their round2 (they are part of the byte-compared metrics);
  * the fused path gives the same bytes (nzsum included) from run to run: fixed-shape sums, no float atomics.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (haplotypes, genome length[, fraction of the strains present in the sample]) per species: a large segment, one the species level drops (no genome length), a single-path species, a segment of
# at most 4096 nodes (sorted whole by the sampler), 17..64 haplotypes (several column-table bytes, columns beyond 8), one just above 4096 nodes,
# a small two-strain one
SPEC = [(5, 120000), (4, 100000), (1, 40000), (3, 60000), (20, 150000, 0.7), (6, 66000), (2, 50000)]
DROPPED = 1


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _make_set(seed, spec, n_reads):
    import synthdata as synth
    rng = np.random.default_rng(seed)
    species, start = [], 1
    for s, (h, gl, *pf) in enumerate(spec):
        g = synth.make_species(rng, str(1000 + s), h, gl, start, "GCF_%06d" % (s + 1), present_frac=pf[0] if pf else 0.4)
        species.append(g)
        start = g.range_end + 1
    return synth.SyntheticSet(species, synth.make_reads(rng, species, n_reads))


@pytest.fixture(scope="module")
def corner_set():
    sset = _make_set(20261016, SPEC, 120000)
    n = [g.n_nodes for g in sset.species]
    assert n[3] <= 4096 and 4096 < n[5] <= 4096 + 512 and n[0] > 4096 and n[2] <= 4096, n      # the sampler's limit from both sides
    ln = np.concatenate([g.node_len for g in sset.species if g.n_paths > 1])
    assert (ln > 33).sum() > 100 and (ln > 64).sum() > 100 and np.median(ln) < 33              # interior bit-vector words in a short-node graph
    assert sum(int(g.node_len.sum()) for g in sset.species) // sum(n) < 48                       # (not the long-node variant of the statistics pass)
    return sset


def _avg(sset, dropped=DROPPED):
    avg = np.array(sset.avg_len(), dtype=np.float64)
    if dropped is not None:
        avg[dropped] = 0.0                       # a species without a genome length is dropped by the species level (profile.rs:329)
    return avg


def _raw_step(eng, avg, **kw):
    """one resident step with every launch timed -> everything it returns, as bytes / copies, + the names of the kernels that ran"""
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        keep, absolute, met, info, passed, s_all, s_pass = eng.profile_step(avg, **kw)
        names = set(eng.timing_get())
    finally:
        eng.timing_enable(False)
    amax, nvalid, nzsum, nzcnt = eng.strain_node_stats()
    import ctypes as C
    return dict(keep=keep.copy(), absolute=absolute.copy(), met=C.string_at(met, C.sizeof(met[0]) * eng.H), info=C.string_at(info, C.sizeof(info[0]) * eng.S),
                passed=np.array(passed).copy(), s_all=s_all.copy(), s_pass=s_pass.copy(), amax=amax, nvalid=nvalid, nzsum=nzsum, nzcnt=nzcnt, kernels=names,
                n_cand=[info[s].n_candidates for s in range(eng.S)], n_rows=[info[s].n_rows for s in range(eng.S)])


def _both(eng, avg, **kw):
    eng.set_option("node_pass", "split")
    try:
        a = _raw_step(eng, avg, **kw)
    finally:
        eng.set_option("node_pass", None)
    return a, _raw_step(eng, avg, **kw)


def _assert_same(a, b):
    for k in ("keep", "absolute", "passed", "s_all", "s_pass", "nvalid", "nzcnt"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["amax"], b["amax"]), (a["amax"], b["amax"])                       # a max: no order
    assert a["info"] == b["info"]                                                               # n_rows, n_cand, n_patterns, iterations, both objectives, status
    assert a["met"] == b["met"]                                                                 # every metric, frequencies_mean / divergence after their round2
    rel = np.abs(a["nzsum"] - b["nzsum"]) / np.maximum(np.abs(a["nzsum"]), 1e-300)
    print("nzsum relative difference split / fused: max %.3g" % rel.max())
    assert np.all(rel <= 1e-12), rel.max()


def _assert_paths(split, fused):
    assert {"node_cov_stats_kernel", "ssn_hist_kernel"} <= split["kernels"] and "node_rows_kernel" not in split["kernels"], sorted(split["kernels"])
    assert "node_rows_kernel" in fused["kernels"] and not ({"node_cov_stats_kernel", "ssn_hist_kernel", "node_stats_kernel"} & fused["kernels"]), sorted(fused["kernels"])


@pytest.mark.parametrize("fr", [0.3, 1.01])
def test_fused_pass_equals_the_two_kernels_and_the_oracle(eng, corner_set, set_opt, fr):
    """fr = 1.01: no haplotype of a multi-strain species passes the first filter -- ACTIVE species without LP columns, whose statistics the fused
    pass still has to report (large and small segments), beside the single-path species that keeps its one column."""
    from oracle import oracle as orc
    from pantax_amd.pipeline import StepConfig, profile_step
    from tests.helpers import oracle_strain_level, oracle_passing_rows, check_step_rows_against_oracle
    sset = corner_set
    set_opt(eng, "row_sort", "nodes")            # the node sort below its size threshold: the step path of the full-size configurations
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    avg = _avg(sset)
    split, fused = _both(eng, avg, fr=fr)
    _assert_paths(split, fused)
    _assert_same(split, fused)
    assert not fused["keep"][DROPPED] and fused["keep"].sum() >= 5
    assert fused["amax"][DROPPED] == 0.0 and fused["nvalid"][DROPPED] == 0 and fused["nzsum"][DROPPED] == 0.0
    multi = [s for s, g in enumerate(sset.species) if g.n_paths > 1 and fused["keep"][s]]
    if fr > 1.0:
        assert all(fused["n_cand"][s] == 0 for s in multi) and fused["n_cand"][2] == 1
        assert all(fused["nvalid"][s] > 0 and fused["nzsum"][s] > 0.0 for s in multi)          # statistics of the species without columns
    else:
        assert sum(fused["n_cand"][s] > 0 for s in multi) >= 4 and max(fused["n_cand"]) > 8 and fused["n_rows"][3] > 0 and fused["n_rows"][5] > 0
    # the statistics against numpy on the oracle's coverage, the tables against the oracle's strain level
    rd = sset.reads
    sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in sset.species], [g.range_end for g in sset.species])
    from tests.helpers import select_reads
    for s, g in enumerate(sset.species):
        if not fused["keep"][s]:
            continue
        G = orc.Graph(g.node_len, g.path_off, g.path_nodes)
        so, nid, ps, pe = select_reads(rd, np.nonzero(sp == s)[0])
        b = orc.node_coverage(G, orc.TrioTable(G), g.range_start, so, nid, ps, pe)[0]
        ab = b.astype(np.int64).astype(np.float64) / g.node_len.astype(np.float64)
        assert fused["amax"][s] == ab.max() and fused["nvalid"][s] == (ab > 0).sum() and fused["nzcnt"][s] == (ab > 0).sum()
        assert fused["nzsum"][s] == pytest.approx(ab[ab > 0].sum(), rel=1e-12)
    names = [g.name for g in sset.species]
    haps = [h for g in sset.species for h in g.hap_names]
    sp_rows, st_rows, stats = profile_step(eng, names, haps, avg, StepConfig(fr=fr))
    level = oracle_strain_level(sset, sp, fused["keep"], fused["absolute"], range(len(sset.species)), threads=8, fr=fr)
    active = {r[0] for r in sp_rows if r[1] > 1e-4}
    check_step_rows_against_oracle(st_rows, {k: v for k, v in oracle_passing_rows(sset, level).items() if k in active})
    # the fused path twice on one input: the same bytes, the f64 sums included
    again = _raw_step(eng, avg, fr=fr)
    assert again["met"] == fused["met"] and again["info"] == fused["info"] and again["nzsum"].tobytes() == fused["nzsum"].tobytes()
    assert again["amax"].tobytes() == fused["amax"].tobytes()


def test_min_depth_reaches_the_fused_statistics(eng, corner_set, set_opt):
    sset = corner_set
    set_opt(eng, "row_sort", "nodes")
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    split, fused = _both(eng, _avg(sset), min_depth=3)
    _assert_paths(split, fused)
    _assert_same(split, fused)
    assert np.any(fused["nzcnt"] < fused["nvalid"])


def test_a_species_over_64_haplotypes_keeps_the_db_on_the_two_kernels(eng, set_opt):
    sset = _make_set(20261017, [(5, 60000), (70, 40000), (3, 50000)], 40000)
    set_opt(eng, "row_sort", "nodes")
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    split, dflt = _both(eng, _avg(sset, None))
    for r in (split, dflt):
        assert "node_rows_kernel" not in r["kernels"] and "node_cov_stats_kernel" in r["kernels"], sorted(r["kernels"])
    _assert_same(split, dflt)


def test_row_sampling_keeps_the_two_kernels(eng, corner_set, set_opt):
    sset = corner_set
    set_opt(eng, "row_sort", "nodes")
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    split, dflt = _both(eng, _avg(sset), sample_nodes=1000)
    for r in (split, dflt):
        assert "node_rows_kernel" not in r["kernels"] and "node_cov_stats_kernel" in r["kernels"], sorted(r["kernels"])
    _assert_same(split, dflt)
    assert max(dflt["n_rows"]) == 1000          # (a11 really sampled)


def test_pipelined_steps_with_the_side_stream_arena_fill(eng, corner_set, set_opt):
    """Three resident steps in flight behind each other, the coverage arena zero-filled on the SIDE stream (cov_clean_async=1) and verified to be zero
    before every coverage pass that skips its own fill (cov_arena_verify): the fused kernel is the arena's last reader, the fill has to wait for it."""
    from pantax_amd.pipeline import StepConfig, profile_step, profile_steps_pipelined
    sset = corner_set
    set_opt(eng, "row_sort", "nodes")
    set_opt(eng, "cov_clean_async", "1")
    set_opt(eng, "cov_arena_verify", "1")
    eng.upload_db(sset.species)
    rd = sset.reads
    names = [g.name for g in sset.species]
    haps = [h for g in sset.species for h in g.hap_names]
    avg = _avg(sset)
    rng = np.random.default_rng(5)
    flag_sets = [None] + [(rng.random(rd.n_reads) < f).astype(np.uint8) for f in (0.4, 0.7)]   # three different samples of the same reads
    single = []
    eng.set_option("node_pass", "split")
    try:
        for fl in flag_sets:
            eng.upload_packed(rd, fl)
            single.append(profile_step(eng, names, haps, avg, StepConfig()))
    finally:
        eng.set_option("node_pass", None)
    got = profile_steps_pipelined(eng, names, haps, avg, len(flag_sets), StepConfig(), next_input=lambda i: eng.upload_packed(rd, flag_sets[i]))
    assert len(got) == len(single)
    for a, b in zip(got, single):
        assert a[0] == b[0] and a[1] == b[1] and a[2]["n_active"] == b[2]["n_active"] and a[2]["n_rows"] == b[2]["n_rows"] and a[2]["iters"] == b[2]["iters"]
        assert a[2]["n_cand"] == b[2]["n_cand"] and a[2]["n_patterns"] == b[2]["n_patterns"]
        assert np.array_equal(np.array(a[2]["obj"], dtype=float), np.array(b[2]["obj"], dtype=float), equal_nan=True)
    assert single[1][1] != single[0][1]
    eng.timing_enable(True)                      # (the path the pipelined steps took: the same options, one more step, its launches named)
    eng.timing_reset()
    try:
        profile_step(eng, names, haps, avg, StepConfig())
        assert "node_rows_kernel" in eng.timing_get()
    finally:
        eng.timing_enable(False)


def test_pipelined_steps_with_the_last_readers_cleaning_the_arena(eng, corner_set, set_opt):
    """Three resident steps in flight behind each other with option cov_self_clean=1: the last readers of the coverage arena (the haplotype statistics
    and the node statistics pass) zero what they read, every coverage pass after the first skips its zero fill, and cov_arena_verify counts the arena's
    non-zero words before each such pass.  The results are those of the same three steps under the default options, array by array."""
    from pantax_amd.pipeline import StepConfig, profile_step, profile_steps_pipelined
    sset = corner_set
    set_opt(eng, "row_sort", "nodes")
    eng.upload_db(sset.species)
    rd = sset.reads
    names = [g.name for g in sset.species]
    haps = [h for g in sset.species for h in g.hap_names]
    avg = _avg(sset)
    rng = np.random.default_rng(5)
    flag_sets = [None] + [(rng.random(rd.n_reads) < f).astype(np.uint8) for f in (0.4, 0.7)]   # three different samples of the same reads
    single = []
    for fl in flag_sets:                         # (the default options: a zero fill in front of every coverage pass or beside the LPs, nothing verified)
        eng.upload_packed(rd, fl)
        single.append(profile_step(eng, names, haps, avg, StepConfig()))
    set_opt(eng, "cov_self_clean", "1")
    set_opt(eng, "cov_arena_verify", "1")
    got = profile_steps_pipelined(eng, names, haps, avg, len(flag_sets), StepConfig(), next_input=lambda i: eng.upload_packed(rd, flag_sets[i]))
    assert len(got) == len(single)
    for a, b in zip(got, single):
        assert a[0] == b[0] and a[1] == b[1] and a[2]["n_active"] == b[2]["n_active"] and a[2]["n_rows"] == b[2]["n_rows"] and a[2]["iters"] == b[2]["iters"]
        assert a[2]["n_cand"] == b[2]["n_cand"] and a[2]["n_patterns"] == b[2]["n_patterns"]
        assert np.array_equal(np.array(a[2]["obj"], dtype=float), np.array(b[2]["obj"], dtype=float), equal_nan=True)
    assert single[1][1] != single[0][1]
    eng.timing_enable(True)                      # (the path the pipelined steps took: one more step, which finds the arena clean; its launches named)
    eng.timing_reset()
    try:
        profile_step(eng, names, haps, avg, StepConfig())
        ran = set(eng.timing_get())
        assert "node_cov_stats_kernel" in ran and "node_rows_kernel" not in ran and "zero_fill_kernel" not in ran, sorted(ran)
    finally:
        eng.timing_enable(False)
