"""The short-read coverage kernel at crafted walks, windows and shapes: the corpus of tests/cov_walk_cases.py (tests/test_cov_walk_cases.py shows on the
CPU that it holds what is said here, and that the C oracle and the literal restatement agree on it) through the stage calls -- upload_db, upload_packed,
rcls_profile, trio_nodes_info, get_node_abundances -- under every option that changes how the pass is cut or launched.  Every case compares the species of
every read, `bases`, `cov`, `trio_bases` and the abort count with the oracle BIT FOR BIT (all outputs are integers) and pins the kernels that ran by the
library's timer labels.

What each class of the corpus is there for (stage_cov.hip unless another file is named):
  len_edges   walks of 1, 2, 3, 31 .. 33, 63, 64 steps, up and down, from the first / last id of a block and from inside one: `single`, `len0` by shuffle
              from the lane of step 0, `i + 1 == k`, the segmented `seen` scan; group_layout_kernel's "never straddle a group" and group_fill_kernel's
              flat rounds of 64 (a walk that begins in one round and ends in the next takes its earlier ids from `prev_id`, stage_read_layout.hip);
              a descending 64-step walk from a block's first id ends 63 nodes below it -- the window begins `in_blk + 64` nodes in front of the read
  revisit     `dupd = code & STEP_DIST` up to 63, `at_step0 = dupd == i` and `rl = earlier ? (at_step0 ? len0 - ps : nl) : aln` (read_nodes_len of
              the three nodes of a trio window), with pstart > 0 so that len0 - ps is not the node's length
  offsets     `dead_read` (the assert, one abort per read, counted by the lane of step 0), `live` of a one-node read with pend < pstart, the last
              step's `max(target - seen, 0)`, `markable` of a one-node read with pend > len (bases but no bits)
  two18       `aln < (1u << 18)` of the LDS `bases` window against the global atomicAdd; the 300 000-base node whole (a flag), partly (mark_range:
              lds_or with words inside and outside the bit window), as an interior and as a first step
  giant       a node longer than the whole LDS bit window (COV_BWIN words): `mark_n == 0` for every item whose window holds it
  words       popcount_kernel / popcount_long_kernel at word edges: `m0`, `m1`, `w0 == w1`, `~m0` of the cooperative branch; one-base nodes on bit 31
              and on bit 32 with an uncovered neighbour; a node whole by a flag AND by bits; whole only as the union of two partial marks; stretches
              just below and above PCL_WORDS and stretches without a node over 64 bases (the per-lane loop inside popcount_long_kernel)
  far         `off = v - wlo` with `inw` false: nodes beyond the window and, through the unsigned wrap, below it -- `bases`, whole-node flags
              (atomicOr on `full`) and partial marks (mark_range) on the global path
  border      groups and items that hold reads of two species (slot_rec.y differs per lane; the window spans the border), deselected lanes beside
              active ones in the species_active case
  heads       `nh > 2`: the `j >= 2` loop behind `any1(!(m0 | m1) & (nh[u] > 2u))`, from both orientations, with tlo == thi (a == c)
  heads64     the same from lanes 2, 3, 62 and 63 of a group (a 64-step walk IS a group: step i sits in lane i, whatever the order of the slots; lanes
              0 and 1 never search a head here -- the searching step is a walk's third or later, and a walk of <= 64 steps begins in its group)
  crowd       a block of more than COV_ITEM_GROUPS groups: build_step_read's equal cuts, `gw0 >= n_groups` of both prefetch levels (an item of fewer
              groups than the workgroup has waves -- the cov_item_groups cases), and, dropped, the window probe loop that skips an item's first groups
  fill        everything at once, in every block; empty walks own no slot
  controls    three walks of 65 steps (coverage_long_kernel and walk_sum_kernel run beside the short-read kernel: `none1(... STEP_LONG)` leaves their
              groups alone), two walks that leave their species (no species: slot_rec.x < 0)
"""
import numpy as np
import pytest

from tests import cov_walk_cases as cw
from tests.helpers import oracle_coverage

pytestmark = pytest.mark.gpu

LABELS = {"coverage_fast_kernel", "coverage_long_kernel", "coverage_step_kernel", "walk_sum_kernel", "popcount_kernel"}
FAST, LONG, STEP, WALK, COUNT = "coverage_fast_kernel", "coverage_long_kernel", "coverage_step_kernel", "walk_sum_kernel", "popcount_kernel"
DEFAULT = {FAST, LONG, WALK, COUNT}          # (the three controls of 65 steps are the long-walk kernel's)
COVF_SHAPES = (182, 242, 282, 283, 284, 243, 2823, 2825, 2423, 2425, 1823, 4423, 442, 443)     # every code of cov_fast_shape (cov_plan.cpp)

# id, library options, the labels of LABELS that run
CASES = [("default", {}, DEFAULT)]
CASES += [("covf_shape_%d" % c, {"covf_shape": c}, DEFAULT) for c in COVF_SHAPES]
CASES += [("cov_item_groups_%d" % n, {"cov_item_groups": n}, DEFAULT) for n in (1, 3, 7)]      # read at upload: every case uploads its reads
CASES += [
    ("group_bucket_bits_10", {"group_bucket_bits": 10}, DEFAULT),                              # on the corpus 32 768 ids higher: there the cap widens the buckets
    ("general", {"cov_general": 1}, {LONG, WALK, COUNT}),                                       # the same groups through the other bodies
    ("general_covl_1120", {"cov_general": 1, "covl_shape": 1120}, {LONG, WALK, COUNT}),
    ("general_by_step", {"cov_general": 1, "cov_long": "step"}, {STEP, WALK, COUNT}),
    ("plain_popcount", {"ncs_no_prefix": 1}, DEFAULT),
]


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world():
    """the corpus, the oracle's binning and the oracle's coverage of it: made once, shared by the cases, never changed"""
    from oracle import oracle as orc
    species, rd, classes = cw.build()
    sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in species], [g.range_end for g in species])
    ref = oracle_coverage(species, rd, sp)
    assert sum(r[4] for r in ref) == len(classes["offsets_abort"]) > 0
    assert all(int(r[1].sum()) > 0 and int(r[2].sum()) > 0 and int(r[3].sum()) > 0 for r in ref)
    return species, rd, classes, sp, ref


def _timed_coverage(eng, species_active=None, with_trio=True):
    """the stage calls under the library's timers -> (species of every read, bases, cov, trio_bases, aborts, the labels that ran)"""
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        sp, *_ = eng.rcls_profile()
        eng.trio_nodes_info(fetch=False)
        bases, cov, tb, nab = eng.get_node_abundances(species_active=species_active, with_trio=with_trio)
        ran = set(eng.timing_get())
    finally:
        eng.timing_enable(False)
    return sp, bases, cov, tb, nab, ran


def _check(eng, ref, bases, cov, tb, nab, with_trio=True):
    u0 = 0
    for si, (T, b, c, t, na) in enumerate(ref):
        lo, hi = int(eng.node_off[si]), int(eng.node_off[si + 1])
        for name, got, exp in (("bases", bases[lo:hi], b), ("cov", cov[lo:hi], c)):
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, "%s of species %d differs at %d local nodes, first %s: got %s, oracle %s" % (
                name, si, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
        if with_trio:
            bad = np.nonzero(tb[u0:u0 + T.n_unique] != t)[0]
            assert len(bad) == 0, "trio_bases of species %d differs at %d rows, first keys %s: got %s, oracle %s" % (
                si, len(bad), T.abc[bad[:6]].tolist(), tb[u0:u0 + T.n_unique][bad[:6]].tolist(), t[bad[:6]].tolist())
        u0 += T.n_unique
    assert u0 == eng.U and nab == sum(r[4] for r in ref)


@pytest.mark.parametrize("name,options,expected", CASES, ids=[c[0] for c in CASES])
def test_crafted_walks(eng, world, set_opt, name, options, expected):
    species, rd, classes, ref_sp, ref = world
    if name == "plain_popcount":      # ... so that the default case counted through popcount_long_kernel (long_node_shape)
        assert sum(int(g.node_len.sum()) for g in species) // sum(g.n_nodes for g in species) >= 48
    for opt, value in options.items():
        set_opt(eng, opt, value)
    if "group_bucket_bits" in options:
        # at the corpus's own ids (391 buckets of 32) no cap the option can set is reached; 16 blocks higher there are 1 415, so the least cap makes
        # build_step_read widen the buckets to 64 ids -- the reference's results do not change (tests/test_cov_walk_cases.py)
        species, rd = cw.shifted(species, rd)
        assert (int(rd.node_id.max()) >> 5) + 1 > 1 << options["group_bucket_bits"]
    eng.upload_db(species)
    eng.upload_packed(rd)
    sp, bases, cov, tb, nab, ran = _timed_coverage(eng)
    print("%s: %s" % (name, sorted(ran & LABELS)))
    assert np.array_equal(sp, ref_sp)
    _check(eng, ref, bases, cov, tb, nab)
    assert ran & LABELS == expected, sorted(ran & LABELS)


def test_without_trio(eng, world):
    species, rd, classes, ref_sp, ref = world
    eng.upload_db(species)
    eng.upload_packed(rd)
    sp, bases, cov, tb, nab, ran = _timed_coverage(eng, with_trio=False)
    assert np.array_equal(sp, ref_sp) and tb is None
    _check(eng, ref, bases, cov, tb, nab, with_trio=False)
    assert ran & LABELS == DEFAULT, sorted(ran & LABELS)


def test_deselected_species_and_dropped_reads(eng, world):
    """species B deselected, and drop flags on the reads of the crowd's first 40 groups (in the order of the stream: by first id) and on every third other
    read: the first groups of the crowd's first item hold no live read and the probe for the window's base runs on to a later group; the items of the
    border blocks begin with deselected reads.  The oracle runs on the surviving reads; nothing of B is touched."""
    species, rd, classes, ref_sp, ref_all = world
    so = rd.step_off.astype(np.int64)
    k = np.diff(so)
    crowd = classes["crowd"]
    crowd = crowd[np.argsort(rd.node_id[so[crowd]], kind="stable")]
    n_drop = int(np.searchsorted(np.cumsum(k[crowd]), 40 * 64, side="right"))
    flags = np.zeros(rd.n_reads, dtype=np.uint8)
    others = np.setdiff1d(np.arange(rd.n_reads), classes["crowd"])
    flags[others[::3]] = 1
    flags[crowd[:n_drop]] = 1
    # every read that starts among the dropped stretch of ids is dropped: whole groups at the front of the crowd's block are dead
    first = np.full(rd.n_reads, -1, dtype=np.int64)
    first[k > 0] = rd.node_id[so[:-1][k > 0]]
    edge = int(first[crowd[n_drop - 1]])
    assert n_drop >= 150 and flags[(first >= cw.CROWD_BLOCK * cw.BLOCK) & (first < edge)].all()
    active = np.array([1, 0, 1], dtype=np.uint8)
    ref = oracle_coverage(species, rd, np.where(active[np.maximum(ref_sp, 0)] == 1, ref_sp, -1), keep=flags == 0)
    assert not ref[1][1].any() and not ref[1][2].any() and not ref[1][3].any() and ref[1][4] == 0
    assert 0 < sum(r[4] for r in ref) < sum(r[4] for r in ref_all) and int(ref[0][3].sum()) > 0 and int(ref[2][3].sum()) > 0
    eng.upload_db(species)
    eng.upload_packed(rd, flags=flags)
    sp, bases, cov, tb, nab, ran = _timed_coverage(eng, species_active=active)
    assert np.array_equal(sp, ref_sp)
    lo, hi = int(eng.node_off[1]), int(eng.node_off[2])
    assert not bases[lo:hi].any() and not cov[lo:hi].any()          # the nodes of B: all zero
    _check(eng, ref, bases, cov, tb, nab)
    assert ran & LABELS == DEFAULT, sorted(ran & LABELS)
