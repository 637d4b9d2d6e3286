"""The fused node pass (node_rows_kernel) where its instruction-issue rework can go wrong: the level-major, branch-free tree descent of a half's four
items (sn_bucket_ids: every lane descends, a lane without a row discards its id), the peeled tail (tiles wholly inside the segment take a body without
guards and a wave-uniform base per half; only a segment's last tile takes the guarded body, whose dead lanes load node n - 1 and select zeros), and
the per-half addressing of the four streams and the flag word.  One resident step on the fused path against node_pass=split (whose ssn_hist_kernel
keeps the serial descent: the comparison pins the bucket ids), against the oracle, and against itself.

What must hold: what tests/test_gpu_node_pass.py asserts (fused == split exactly, nzsum to 1e-12 relative; the timer labels name the kernels), the
strain rows against the oracle, the statistics against numpy on the oracle's coverage, and two fused runs return equal bytes.

The set, every property asserted on the host when it is made (_check_shapes) or, where it depends on the step's own filter, right after the step:
  segments of 6 144 (the db's FIRST species, node_base 0: exactly three tiles, no guarded tile at all), 4 097 (two whole tiles and a guarded tile of
  one node), 6 145, 8 191 and 4 352 = 17 x 256 nodes (the db's LAST species: its last end is bit_off[V]); node_base values that are odd, = 2 mod 32 and
  = 32 mod 64 (the flag word's shift, the wave's first bit);
  a species of 64 haplotypes, all present and deep enough that ALL 64 pass the first filter (asserted after the step, and against the oracle's candidate
  count): column 63 is kept, thousands of covered nodes are visited by haplotype 63, and their masks have bit 63 set -- under a signed 64-bit compare
  such rows sort in front of every splitter, so the mask compare of the descent must be unsigned;
  a species whose rows all carry ONE key (a single path, every node covered whole exactly once: a = 1, mask = 1), so every splitter is equal and every
  row lands in a tie bucket;
  a segment of 8 191 nodes in which only the ~300 nodes of one short haplotype are covered: far fewer than 1 023 valid samples, so splitters repeat;
  its third haplotype is covered thinly and fails the filter: covered nodes with an EMPTY mask (c0, no row);
  thinly covered ordinary species: nodes of zero abundance interleaved lane by lane with rows (hundreds of changes along every large segment).
  Rows below the smallest and above the largest splitter are NOT asserted: neither the splitters nor the count matrix leave the device through any call
  of the library, so the host cannot check it.  It is expected only -- the sampler puts three to four valid samples between two splitters, so in a segment
  with thousands of rows the few smallest and largest samples are themselves such rows.
ssn_plan gives every workgroup ONE tile at this size (per = ceil(tiles x S / 8192) = 1): the workgroup of a segment's last tile owns only the guarded
tile (4 097: one node of it), and no workgroup walks more than one tile -- that needs tiles x S > 8 192, which no quick set has.  The walk over several
whole tiles and on into the guarded one is the suite's at full size: tests/test_gpu_configs.py runs the resident step at 100 species (per = 2), every
species' strain rows against the oracle, and at 1 000 species (per = 20) against an oracle sample.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

READ_LEN = 75
N_READS = 283000                                                # (nearly all of them the 64-haplotype species': its 64 strains at depth 10)
SIZES = (6144, 4097, 6145, 8191, 4127, 4352)
ONE_KEY, FEW, WIDE = 4, 3, 2
ONE_KEY_LEN = 40


def _crafted_few(rng, name, start, prefix):
    """8 191 nodes; haplotype A walks all of them (absent), B every 27th (present, deep), C every 27th from 13 on (present, thin)"""
    import synthdata as synth
    n = SIZES[FEW]
    ln = rng.integers(1, 60, size=n).astype(np.int64)
    paths = [np.arange(n, dtype=np.uint32), np.arange(0, n, 27, dtype=np.uint32), np.arange(13, n, 27, dtype=np.uint32)]
    off = np.zeros(4, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in paths])
    glen = np.array([ln[p].sum() for p in paths], dtype=np.int64)
    return synth.SpeciesGraph(name, ln, off, np.concatenate(paths).astype(np.uint32), sorted("%s%03d.1" % (prefix, h) for h in range(3)), start, start + n - 1,
                              glen, np.array([0.0, 30.0, 0.4]))


def _crafted_one_key(name, start, prefix):
    import synthdata as synth
    n = SIZES[ONE_KEY]
    ln = np.full(n, ONE_KEY_LEN, dtype=np.int64)
    return synth.SpeciesGraph(name, ln, np.array([0, n], dtype=np.uint64), np.arange(n, dtype=np.uint32), ["%s000.1" % prefix], start, start + n - 1,
                              np.array([ln.sum()], dtype=np.int64), np.array([1.0]))


def _make_set():
    import synthdata as synth
    from tests.test_gpu_node_bits import _refit
    rng = np.random.default_rng(20261020)
    # (haplotypes, genome length, fraction of the strains present, depth of a present strain)
    spec = {0: (5, 125000, 0.4, 1.5), 1: (4, 85000, 0.5, 1.5), WIDE: (64, 125000, 1.0, 10.0), 5: (6, 90000, 0.34, 1.5)}
    species, start = [], 1
    for s, n in enumerate(SIZES):
        if s == FEW:
            g = _crafted_few(rng, str(1000 + s), start, "GCF_%06d" % (s + 1))
        elif s == ONE_KEY:
            g = _crafted_one_key(str(1000 + s), start, "GCF_%06d" % (s + 1))
        else:
            h, gl, pf, depth = spec[s]
            g = synth.make_species(rng, str(1000 + s), h, gl, start, "GCF_%06d" % (s + 1), present_frac=pf)
            assert g.n_nodes >= n, (s, g.n_nodes)
            g = _refit(g, g.node_len, n)
            g.truth_depth[g.truth_depth > 0] = depth              # thin cover: zero abundance between the rows
        species.append(g)
        start = g.range_end + 1
    reads = synth.make_reads(rng, species[:ONE_KEY] + species[ONE_KEY + 1:], N_READS, read_len=READ_LEN)
    # the one-key species: one read per node, the node whole
    g = species[ONE_KEY]
    n = g.n_nodes
    full = np.full(n, ONE_KEY_LEN, dtype=np.int64)
    one = synth.PackedReads(np.arange(n + 1, dtype=np.uint64), (g.range_start + np.arange(n)).astype(np.uint32), np.zeros(n, dtype=np.uint8),
                            np.zeros(n, dtype=np.int64), full, full.copy(), np.full(n, 60, dtype=np.int64), full.copy())
    cat = lambda f: np.concatenate([getattr(reads, f), getattr(one, f)])
    step_off = np.concatenate([reads.step_off, one.step_off[1:] + reads.step_off[-1]])
    return synth.SyntheticSet(species, synth.PackedReads(step_off, cat("node_id"), cat("strand"), cat("pstart"), cat("pend"), cat("qlen"), cat("mapq"), cat("plen")))


def _check_shapes(sset):
    sp = sset.species
    assert tuple(g.n_nodes for g in sp) == SIZES and all(n > 4096 for n in SIZES)                   # every segment takes the node pass
    assert {4097, 4352, 6144, 6145, 8191} <= set(SIZES) and SIZES[0] == 6144 and SIZES[0] % 2048 == 0 and SIZES[-1] == 4352
    base = np.concatenate([[0], np.cumsum(SIZES)])[:-1]
    assert base[0] == 0 and base[2] % 2 == 1 and base[3] % 32 == 2 and base[5] % 64 == 32, base      # the flag word's shift and the wave's first bit
    assert sum(b % 32 != 0 for b in base) >= 3 and sum(b % 64 != 0 for b in base) >= 4
    assert sp[WIDE].n_paths == 64 and (sp[WIDE].truth_depth > 0).all()
    few = sp[FEW]
    assert len(few.path_nodes[int(few.path_off[1]):int(few.path_off[2])]) < 320 and few.truth_depth[0] == 0.0   # far fewer rows than the 1 023 splitters


@pytest.fixture(scope="module")
def world():
    """the set, the oracle's species per read and its covered bases per node -- made once, read-only"""
    from oracle import oracle as orc
    from tests.helpers import select_reads
    sset = _make_set()
    _check_shapes(sset)
    rd = sset.reads
    sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in sset.species], [g.range_end for g in sset.species])
    cov = []
    for s, g in enumerate(sset.species):
        G = orc.Graph(g.node_len, g.path_off, g.path_nodes)
        so, nid, ps, pe = select_reads(rd, np.nonzero(sp == s)[0])
        b, c = orc.node_coverage(G, orc.TrioTable(G), g.range_start, so, nid, ps, pe)[:2]
        cov.append((b.astype(np.int64), np.asarray(c).astype(np.int64)))
    # zero abundance interleaved with covered nodes, lane by lane, in the ordinary species; the one key; the few covered nodes
    for s in (0, 1, 5):
        on = cov[s][0] > 0
        assert np.count_nonzero(on[1:] != on[:-1]) > 300 and 0.2 < on.mean() < 0.98, (s, on.mean())
    assert np.all(cov[ONE_KEY][0] == ONE_KEY_LEN)
    assert 100 < (cov[FEW][0] > 0).sum() < 700
    return dict(sset=sset, sp=sp, cov=cov)


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _visited(g, haps):
    v = np.zeros(g.n_nodes, dtype=bool)
    for h in haps:
        v[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])]] = True
    return v


def test_fused_equals_split_the_oracle_and_itself(eng, world, set_opt):
    from pantax_amd.pipeline import StepConfig, profile_step
    from tests.helpers import oracle_strain_level, oracle_passing_rows, check_step_rows_against_oracle
    from tests.test_gpu_node_pass import _raw_step, _assert_same, _assert_paths
    from tests.test_gpu_node_bits import _bytes_equal
    sset = world["sset"]
    set_opt(eng, "row_sort", "nodes")            # the node sort below its size threshold: the step path of the full-size configurations
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    avg = np.array(sset.avg_len(), dtype=np.float64)
    fused = _raw_step(eng, avg)
    set_opt(eng, "node_pass", "split")
    split = _raw_step(eng, avg)
    set_opt(eng, "node_pass", None)
    again = _raw_step(eng, avg)
    _assert_paths(split, fused)
    _assert_same(split, fused)
    _bytes_equal(fused, again)                   # two runs of the fused step: equal bytes, the f64 sums included
    print("candidates per species:", fused["n_cand"], "rows:", fused["n_rows"])
    assert fused["keep"].all() and all(c > 0 for c in fused["n_cand"])
    # what the step's own filter decides, checked where it is known
    assert fused["n_cand"][WIDE] == 64                                                           # every haplotype kept: haplotype 63 is column 63 of the mask
    wide_hi = _visited(sset.species[WIDE], [63]) & (world["cov"][WIDE][0] > 0)
    print("64-haplotype species: %d covered nodes visited by haplotype 63 (mask bit 63)" % wide_hi.sum())
    assert wide_hi.sum() > 1000 and (~wide_hi & (world["cov"][WIDE][0] > 0)).sum() > 100         # rows with and without bit 63: a signed compare reorders them
    assert fused["n_cand"][ONE_KEY] == 1 and fused["n_rows"][ONE_KEY] == SIZES[ONE_KEY] and fused["amax"][ONE_KEY] == 1.0   # every node a row, one key
    assert 0 < fused["n_rows"][FEW] < 700                                                        # (n_rows: the covered nodes, with or without a column) far fewer rows than splitters
    # the statistics against numpy on the oracle's coverage
    for s, g in enumerate(sset.species):
        ab = world["cov"][s][0].astype(np.float64) / g.node_len.astype(np.float64)
        assert fused["amax"][s] == ab.max() and fused["nvalid"][s] == (ab > 0).sum() and fused["nzcnt"][s] == (ab > 0).sum()
        assert fused["nzsum"][s] == pytest.approx(ab[ab > 0].sum(), rel=1e-12)
    # the strain rows against the oracle
    names = [g.name for g in sset.species]
    haps = [h for g in sset.species for h in g.hap_names]
    sp_rows, st_rows, stats = profile_step(eng, names, haps, avg, StepConfig())
    level = oracle_strain_level(sset, world["sp"], fused["keep"], fused["absolute"], range(len(sset.species)), threads=8)
    active = {r[0] for r in sp_rows if r[1] > 1e-4}
    assert len(active) == len(sset.species)
    check_step_rows_against_oracle(st_rows, {k: v for k, v in oracle_passing_rows(sset, level).items() if k in active})
    # rows and nodes that are no rows, lane by lane: a row = a covered node that a kept haplotype visits
    for s, g in enumerate(sset.species):
        cand = [h for h, m in enumerate(level[s][0]) if m["path_base_cov"] is not None]
        assert len(cand) == level[s][1] == fused["n_cand"][s]
        b = world["cov"][s][0]
        row = _visited(g, cand) & (b > 0)
        assert 0 < row.sum() <= fused["n_rows"][s] == (b > 0).sum(), (s, row.sum(), fused["n_rows"][s])
        flips, nomask = np.count_nonzero(row[1:] != row[:-1]), int(((b > 0) & ~_visited(g, cand)).sum())
        print("species %d: %d nodes, %d rows, %d row / no-row changes, %d covered nodes with an empty mask" % (s, g.n_nodes, row.sum(), flips, nomask))
        if s in (0, 1, 5):
            assert flips > 300, (s, flips)
        if s == FEW:
            assert nomask >= 20 and flips > 100, (nomask, flips)                                 # c0: covered, no column
