"""Where the fused node pass (node_rows_kernel) takes a node's bit-vector words from: option node_bits=range (an item's stretch of the bit vector
loaded whole beside the streams, every node served from the wave's registers by shuffles; a stretch over the capacity gathers) against
node_bits=gather (every node loads its own words: the loads of the kernel before this option), against node_pass=split and against the oracle --
one resident step three ways, in one process on the same inputs.

What must hold:
  * range against gather: every returned byte is equal, nzsum included (the same sums in the same order: only the source of the words differs);
  * against split and against the oracle: what tests/test_gpu_node_pass.py asserts -- exact, except nzsum to 1e-12 relative (see there);
  * the timer labels show node_rows_kernel on both fused runs.
The set is built so that the new code is exercised at every place it can go wrong; each property is asserted on the host from node_len (and the
oracle's coverage) when the set is made, so no case runs without it:
  segments of 4 097 and 4 160 nodes and one of n % 64 == 1 (an item of one node, a partial and a full last item, the end clamp); the LAST species of the
  db (its last end is bit_off[V]); segments whose first bit is no multiple of 32, items that start and end inside a word; nodes of exactly 31, 32, 33, 64
  and 65 bases and hundreds over 64 (interior words) at a segment average below 48; a segment of very short nodes (median <= 4, many nodes per word);
  with node_bits_words=1 every large segment has items over and under the 2 048-bit capacity; with the default one item sums to more than 4 096 bits;
  and every species that takes the node pass (all multi-strain) has hundreds of nodes that have a column and are covered in part, so that the bits, not the
  flags, decide the counts.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_READS = 100000
READ_LEN = 75
N_SHORT, SHORT_LEN = 1600, 24                                   # short reads: many read ends, each one a node covered in part
EXACT = (31, 32, 33, 64, 65)
# relative depth of a present strain, per species: the small segment (the sampler's, no node pass) takes most of the reads, the strains of the large segments
# are covered one to two times -- a read's end falls inside a node whose rest nothing covers
DEPTH = (1.0, 1.0, 1.0, 60.0, 1.0, 1.0)


def _refit(g, node_len, n=None):
    """the species with other node lengths and, with n, cut to its first n nodes (walks keep the nodes that are left)"""
    import synthdata as synth
    n = len(node_len) if n is None else n
    node_len = np.asarray(node_len[:n], dtype=np.int64)
    paths = [g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])] for h in range(g.n_paths)]
    paths = [p[p < n] for p in paths]
    assert all(len(p) > 2 for p in paths)
    off = np.zeros(g.n_paths + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in paths])
    glen = np.array([node_len[p].sum() for p in paths], dtype=np.int64)
    return synth.SpeciesGraph(g.name, node_len, off, np.concatenate(paths).astype(np.uint32), g.hap_names, g.range_start, g.range_start + n - 1, glen, g.truth_depth)


def _make_set():
    import synthdata as synth
    rng = np.random.default_rng(20261019)
    # (haplotypes, genome length, mean node length, nodes to keep, fraction of the strains present)
    spec = [(5, 125000, 32, 6401, 0.4),      # n % 64 == 1; holds the run over the default capacity
            (4, 20000, 3, None, 0.5),        # very short nodes
            (20, 150000, 32, None, 0.15),    # several column-table bytes               
            (3, 60000, 32, None, 0.67),      # at most 4096 nodes: the sampler's (no node pass)
            (6, 85000, 32, 4160, 0.34),      # 65 full items
            (5, 85000, 32, 4097, 0.4)]       # 64 items and one node; the last species: its last end is bit_off[V]
    species, start, bits = [], 1, 0
    for s, (h, gl, ml, keep, pf) in enumerate(spec):
        g = synth.make_species(rng, str(1000 + s), h, gl, start, "GCF_%06d" % (s + 1), mean_len=ml, present_frac=pf)
        ln = g.node_len.copy()
        n = keep or len(ln)
        assert len(ln) >= n, (s, len(ln))
        if n > 4096:
            ln[640:640 + 40] = 60                                    # an item over 2 048 bits in every large segment
            for k, e in enumerate(EXACT * 8):
                ln[1300 + 37 * k] = e                                # the lengths at the edges of the word loop, at many alignments
        if s == 0:
            ln[2048 + 128:2048 + 192] = 70                           # one item (64 nodes of a wave) over 4 096 bits
        if s + 1 < len(spec) and (bits + int(ln[:n].sum())) % 32 == 0:
            ln[n - 1] += 1                                           # the next segment starts inside a word
        g = _refit(g, ln, n)
        pres = np.nonzero(g.truth_depth > 0)[0]
        g.truth_depth[:] = 0.0
        g.truth_depth[pres] = DEPTH[s]                               # thin cover of the large segments: nodes covered in part
        species.append(g)
        start = g.range_end + 1
        bits += int(ln[:n].sum())
    # the species of very short nodes gets reads of its own length: a read's end makes a node covered in part, and it has few bases to spend on reads
    short = synth.make_reads(rng, species[1:2], N_SHORT, read_len=SHORT_LEN)
    rest = synth.make_reads(rng, species[:1] + species[2:], N_READS - N_SHORT, read_len=READ_LEN)
    cat = lambda f: np.concatenate([getattr(short, f), getattr(rest, f)])
    step_off = np.concatenate([short.step_off, rest.step_off[1:] + short.step_off[-1]])
    return synth.SyntheticSet(species, synth.PackedReads(step_off, cat("node_id"), cat("strand"), cat("pstart"), cat("pend"), cat("qlen"), cat("mapq"), cat("plen")))


def _items(sset):
    """per large segment: first bit and bits of every item (64 consecutive nodes of the segment)"""
    out, bit = {}, 0
    for s, g in enumerate(sset.species):
        ln = g.node_len
        if g.n_nodes > 4096:
            e = np.concatenate([[0], np.cumsum(ln)])
            a = np.arange(0, g.n_nodes, 64)
            b = np.minimum(a + 64, g.n_nodes)
            out[s] = (bit + e[a], e[b] - e[a], b - a)
        bit += int(ln.sum())
    return out


def _check_shapes(sset):
    sp = sset.species
    n = [g.n_nodes for g in sp]
    large = [s for s in range(len(sp)) if n[s] > 4096]
    assert len(large) == 5 and n[3] <= 4096 and all(g.n_paths > 1 for g in sp)
    assert n[5] == 4097 and n[4] == 4160 and n[0] % 64 == 1 and large[-1] == len(sp) - 1           # segment sizes; the last species takes the node pass
    it = _items(sset)
    assert it[5][2][-1] == 1 and it[4][2][-1] == 64 and it[0][2][-1] == 1                           # an item of one node, a full last item
    assert any(0 < k < 64 and k != 1 for s in large for k in it[s][2][-1:])                          # a partial last item
    unaligned = [s for s in large if it[s][0][0] % 32 != 0]
    assert len(unaligned) >= 3 and it[5][0][0] % 32 != 0, unaligned                                  # segments that start inside a word
    for s in unaligned:
        assert np.sum((it[s][0] % 32 != 0) & ((it[s][0] + it[s][1]) % 32 != 0)) > 10                 # items that start and end inside a word
    for s in large:
        ln = sp[s].node_len
        assert ln.sum() / len(ln) < 48                                                               # (not the long-node shape of the statistics pass)
        assert (it[s][1] > 2048).any() and (it[s][1] <= 2048).sum() > 10, s                          # node_bits_words=1: both ways in every large segment
        if s != 1:
            assert all((ln == e).sum() >= 8 for e in EXACT) and (ln > 64).sum() >= 100, s
    assert np.median(sp[1].node_len) <= 4 and n[1] >= 4097                                           # many nodes per word
    assert (it[0][1] > 4096).any() and sum((it[s][1] <= 4096).sum() for s in large) > 300            # the default capacity: over and under


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
    return dict(sset=sset, sp=sp, cov=cov, level=None)


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


def _bytes_equal(a, b):
    for k in ("keep", "absolute", "passed", "s_all", "s_pass", "amax", "nvalid", "nzsum", "nzcnt"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert a["info"] == b["info"] and a["met"] == b["met"]


@pytest.mark.parametrize("words", [1, 0])
def test_range_equals_gather_split_and_the_oracle(eng, world, set_opt, words):
    """words = 1: a lane holds one word of an item's stretch -- a large share of the items of an ordinary graph is over the 2 048 bits and gathers;
    words = 0: the default (two words, 4 096 bits)."""
    from pantax_amd.pipeline import StepConfig, profile_step
    from tests.helpers import oracle_strain_level, oracle_passing_rows, check_step_rows_against_oracle
    from tests.test_gpu_node_pass import _raw_step, _assert_same, _assert_paths
    sset = world["sset"]
    set_opt(eng, "row_sort", "nodes")            # the node sort below its size threshold: the step path of the full-size configurations
    set_opt(eng, "node_bits_words", str(words))
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    avg = np.array(sset.avg_len(), dtype=np.float64)
    set_opt(eng, "node_bits", "range")
    rng_ = _raw_step(eng, avg)
    set_opt(eng, "node_bits", "gather")
    gat = _raw_step(eng, avg)
    set_opt(eng, "node_pass", "split")
    split = _raw_step(eng, avg)
    set_opt(eng, "node_pass", None)
    set_opt(eng, "node_bits", "range")
    _assert_paths(split, rng_)
    _assert_paths(split, gat)
    _bytes_equal(rng_, gat)
    _assert_same(split, rng_)
    _assert_same(split, gat)
    assert rng_["keep"].all() and all(c > 0 for c in rng_["n_cand"])
    # the statistics against numpy on the oracle's coverage
    for s, g in enumerate(sset.species):
        ab = world["cov"][s][0].astype(np.float64) / g.node_len.astype(np.float64)
        assert rng_["amax"][s] == ab.max() and rng_["nvalid"][s] == (ab > 0).sum() and rng_["nzcnt"][s] == (ab > 0).sum()
        assert rng_["nzsum"][s] == pytest.approx(ab[ab > 0].sum(), rel=1e-12)
    # the tables against the oracle's strain level (path_base_cov is the column sum the bit-vector words feed)
    names = [g.name for g in sset.species]
    haps = [h for g in sset.species for h in g.hap_names]
    sp_rows, st_rows, stats = profile_step(eng, names, haps, avg, StepConfig())
    if world["level"] is None:
        world["level"] = oracle_strain_level(sset, world["sp"], rng_["keep"], rng_["absolute"], range(len(sset.species)), threads=8)
    level = world["level"]
    active = {r[0] for r in sp_rows if r[1] > 1e-4}
    assert len(active) == len(sset.species)
    check_step_rows_against_oracle(st_rows, {k: v for k, v in oracle_passing_rows(sset, level).items() if k in active})
    # partial coverage: nodes with a column (visited by a haplotype the first filter kept) that are covered in part and by no whole-node step alone
    for s, g in enumerate(sset.species):
        cand = [h for h, m in enumerate(level[s][0]) if m["path_base_cov"] is not None]
        assert len(cand) == level[s][1] > 0
        c = world["cov"][s][1]
        part = _visited(g, cand) & (c > 0) & (c < g.node_len)
        print("species %d: %d nodes, %d with a column and covered in part" % (s, g.n_nodes, part.sum()))
        assert g.n_nodes <= 4096 or part.sum() >= 300, (s, part.sum())   # (the small segment is the sampler's, and takes the bulk of the reads)


def test_unknown_values_are_rejected(eng, world, set_opt):
    from pantax_amd._ffi import PantaxHipError
    sset = world["sset"]
    set_opt(eng, "row_sort", "nodes")
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    avg = np.array(sset.avg_len(), dtype=np.float64)
    for name, value in (("node_bits", "scatter"), ("node_bits_words", "3")):
        set_opt(eng, name, value)
        with pytest.raises(PantaxHipError) as ei:
            eng.profile_step(avg)
        assert ei.value.code == -1 and "node_bits" in str(ei.value)      # PANTAX_HIP_E_INVALID, before anything is enqueued
        set_opt(eng, name, None)
    eng.profile_step(avg)                       # (and the ctx is usable afterwards)
