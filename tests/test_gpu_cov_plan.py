"""Which kernels a coverage pass launches (cov_plan / coverage_launch, coverage_prepare), pinned by the library's timer labels: every case runs the stage
calls (rcls_profile, then get_node_abundances), compares `bases`, `cov` and `trio_bases` with the oracle bit for bit and then asserts WHICH of the five
brackets of the pass ran and which did not.  One more case runs a db of SOME of the species over reads made for all of them: the short-read kernel then
launches a list of work items (cov_item_select), and what it computes for the db's species must not change."""
import numpy as np
import pytest

from tests.helpers import select_reads

pytestmark = pytest.mark.gpu

LABELS = {"coverage_fast_kernel", "coverage_long_kernel", "coverage_step_kernel", "walk_sum_kernel", "popcount_kernel"}
FAST, LONG, STEP, WALK, COUNT = "coverage_fast_kernel", "coverage_long_kernel", "coverage_step_kernel", "walk_sum_kernel", "popcount_kernel"

# id, reads of the world, library options, the labels of LABELS that appear -- all others of LABELS must not
CASES = [
    ("short", "short", {}, {FAST, COUNT}),
    ("long", "long", {}, {LONG, WALK, COUNT}),                                    # every walk over 64 steps: the short-read kernel has nothing to do
    ("mixed", "mixed", {}, {FAST, LONG, WALK, COUNT}),
    ("general_short", "short", {"cov_general": "1"}, {LONG, COUNT}),              # every group through the long-walk kernel; no walk is long: no walk sums
    ("mixed_by_step", "mixed", {"cov_long": "step"}, {FAST, STEP, WALK, COUNT}),
    ("zero_reads", "none", {}, {COUNT}),
]


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _subset(rd, idx):
    """the reads idx of rd, in that order, as PackedReads"""
    import synthdata as synth
    so = rd.step_off.astype(np.int64)
    k = so[idx + 1] - so[idx]
    offs = np.concatenate([[0], np.cumsum(k)]).astype(np.uint64)
    at = np.repeat(so[idx] - offs[:-1].astype(np.int64), k) + np.arange(int(offs[-1]))
    return synth.PackedReads(offs, rd.node_id[at], rd.strand[at], rd.pstart[idx], rd.pend[idx], rd.qlen[idx], rd.mapq[idx], rd.plen[idx])


def _concat(ra, rb, order):
    """the reads of ra and rb in one sample, in the given order"""
    import synthdata as synth
    lens = np.concatenate([np.diff(ra.step_off.astype(np.int64)), np.diff(rb.step_off.astype(np.int64))])
    starts = np.concatenate([ra.step_off[:-1].astype(np.int64), rb.step_off[:-1].astype(np.int64) + int(ra.step_off[-1])])
    ids_all, strand_all = np.concatenate([ra.node_id, rb.node_id]), np.concatenate([ra.strand, rb.strand])
    offs = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.uint64)
    idx = np.repeat(starts[order] - offs[:-1].astype(np.int64), lens[order]) + np.arange(int(offs[-1]))
    cat = lambda f: np.concatenate([getattr(ra, f), getattr(rb, f)])[order]
    return synth.PackedReads(offs, ids_all[idx].astype(np.uint32), strand_all[idx], cat("pstart"), cat("pend"), cat("qlen"), cat("mapq"), cat("plen"))


def _oracle(species, rd, sp):
    """per species of the db: (trio table, bases, cov, trio_bases, aborts) of the reads binned to it"""
    from oracle import oracle as orc
    out = []
    for si, g in enumerate(species):
        G = orc.Graph(g.node_len, g.path_off, g.path_nodes)
        T = orc.TrioTable(G)
        so, nid, ps, pe = select_reads(rd, np.nonzero(sp == si)[0])
        out.append((T,) + orc.node_coverage(G, T, g.range_start, so, nid, ps, pe))
    return out


@pytest.fixture(scope="module")
def world():
    """the graphs (three species) and, per key, the reads with the oracle's binning and coverage: made once, shared by the cases, never changed.  Sizes as
    in test_long_reads_and_empty_inputs / test_short_and_long_reads_in_one_sample of tests/test_gpu_parity.py."""
    import synthdata as synth
    from oracle import oracle as orc
    a = synth.make_set(23, 3, 5, 300, 120000, long_reads=True, adversarial_frac=0.02)
    b = synth.make_set(23, 3, 5, 20000, 120000, adversarial_frac=0.02)
    assert all(np.array_equal(x.path_nodes, y.path_nodes) and x.range_start == y.range_start for x, y in zip(a.species, b.species))      # the same graphs
    species = a.species
    k_long = np.diff(a.reads.step_off.astype(np.int64))
    longs = _subset(a.reads, np.nonzero(k_long > 64)[0])
    n_long, n_short = longs.n_reads, b.reads.n_reads
    reads = {"short": b.reads, "long": longs, "mixed": _concat(longs, b.reads, np.random.default_rng(5).permutation(n_long + n_short))}
    refs = {}

    def get(key):
        if key not in refs:
            rd = reads[key]
            sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in species], [g.range_end for g in species])
            refs[key] = (rd, sp, _oracle(species, rd, sp))
        return refs[key]
    return species, get


def test_the_reads_are_what_the_cases_need(world):
    species, get = world
    steps = {key: np.diff(get(key)[0].step_off.astype(np.int64)) for key in ("short", "long", "mixed")}
    assert steps["short"].max() <= 64 and len(steps["short"]) == 20000
    assert steps["long"].min() > 64 and len(steps["long"]) >= 200
    assert (steps["mixed"] > 64).sum() == len(steps["long"]) and (steps["mixed"] <= 64).sum() == len(steps["short"])
    assert sum(int(g.node_len.sum()) for g in species) // sum(g.n_nodes for g in species) < 48       # popcount_kernel, not its long-node variant


def _timed_coverage(eng, with_trio=True):
    """the stage calls under the library's timers -> (species of every read, bases, cov, trio_bases, aborts, the labels that ran)"""
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        sp, *_ = eng.rcls_profile()
        if with_trio:
            eng.trio_nodes_info(fetch=False)
        bases, cov, tb, nab = eng.get_node_abundances(with_trio=with_trio)
        ran = set(eng.timing_get())
    finally:
        eng.timing_enable(False)
    return sp, bases, cov, tb, nab, ran


def _check_against_oracle(eng, ref, bases, cov, tb, nab):
    u0 = 0
    for si, (T, b, c, t, na) in enumerate(ref):
        lo, hi = int(eng.node_off[si]), int(eng.node_off[si + 1])
        assert np.array_equal(bases[lo:hi], b) and np.array_equal(cov[lo:hi], c)
        assert np.array_equal(tb[u0:u0 + T.n_unique], t)
        u0 += T.n_unique
    assert u0 == eng.U and nab == sum(r[4] for r in ref)


@pytest.mark.parametrize("name,key,options,expected", CASES, ids=[c[0] for c in CASES])
def test_kernels_and_coverage(eng, world, set_opt, name, key, options, expected):
    species, get = world
    for opt, value in options.items():
        set_opt(eng, opt, value)
    eng.upload_db(species)
    if key == "none":
        eng.upload_reads(np.zeros(1), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
        sp, bases, cov, tb, nab, ran = _timed_coverage(eng)
        print("%s: %s" % (name, sorted(ran & LABELS)))
        assert len(sp) == 0 and not bases.any() and not cov.any() and not tb.any() and nab == 0
    else:
        rd, ref_sp, ref = get(key)
        eng.upload_packed(rd)
        sp, bases, cov, tb, nab, ran = _timed_coverage(eng)
        print("%s: %s" % (name, sorted(ran & LABELS)))
        assert np.array_equal(sp, ref_sp)
        assert sum(int(r[1].sum()) for r in ref) > 0 and sum(int(r[3].sum()) for r in ref) > 0
        _check_against_oracle(eng, ref, bases, cov, tb, nab)
    assert ran & LABELS == expected, sorted(ran & LABELS)


def test_db_of_some_species_over_reads_of_all(eng):
    """Six species of about 6 000 nodes (some 18 blocks of 2 048 ids), reads for all of them, a db of species 1 and 4: the work items of the short-read
    kernel are cut by the block of a read's first node, and only those that can hold a read of the two species are launched."""
    import synthdata as synth
    from oracle import oracle as orc
    sset = synth.make_set(20261019, 6, 5, 30000, 96000, adversarial_frac=0.01)
    rd = sset.reads
    assert all(5000 <= g.n_nodes <= 7000 for g in sset.species), [g.n_nodes for g in sset.species]
    assert np.diff(rd.step_off.astype(np.int64)).max() <= 64
    db = [sset.species[1], sset.species[4]]
    # cov_item_select's rule over the blocks that hold reads (an item never spans two blocks; a block of many groups is cut into several items): per
    # species the blocks from the one in front of lower_bound(first block of the range) to upper_bound(its last block), merged without duplicates; the
    # list is taken when it is shorter than 8/9 of them
    so = rd.step_off.astype(np.int64)
    first = rd.node_id[so[:-1][np.diff(so) > 0]].astype(np.int64)
    blocks = np.unique(first >> 11)
    assert len(blocks) > 12
    listed = np.zeros(len(blocks), dtype=bool)
    for g in db:
        lo = max(int(np.searchsorted(blocks, g.range_start >> 11, side="left")) - 1, 0)
        hi = int(np.searchsorted(blocks, g.range_end >> 11, side="right"))
        listed[lo:hi] = True
    n_listed = int(listed.sum())
    print("blocks with reads: %d, listed for the db: %d" % (len(blocks), n_listed))
    assert 0 < n_listed and n_listed + n_listed // 8 < len(blocks)
    eng.upload_db(db)
    eng.upload_packed(rd)
    sp, bases, cov, tb, nab, ran = _timed_coverage(eng)
    ref_sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in db], [g.range_end for g in db])
    assert np.array_equal(sp, ref_sp) and (sp == 0).sum() > 1000 and (sp == 1).sum() > 1000 and (sp < 0).sum() > len(sp) // 2
    ref = _oracle(db, rd, ref_sp)
    assert all(int(r[1].sum()) > 0 and int(r[3].sum()) > 0 for r in ref)
    _check_against_oracle(eng, ref, bases, cov, tb, nab)
    assert ran & LABELS == {FAST, COUNT}, sorted(ran & LABELS)
