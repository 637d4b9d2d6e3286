"""The covered-base counts of the resident step, node by node: the corpus of tests/node_count_cases.py (tests/test_node_count_cases.py shows on the
CPU that it holds what is said here) through profile_step under every option that picks another instantiation of node_cov_stats_kernel
(stage_node_stats.hip), read back through pantax_hip_strain_node_cov.  Every comparison is exact: `cov` per node with the C oracle, `ab` bit for bit
with numpy's float64 bases / len (the IEEE division the kernel forms), amax / nvalid / nzcnt, path_cov_ratio of every haplotype that has one against
float32(sum cov) / float32(sum len) of its path (exact: every haplotype is shorter than 2^24 bases) -- but nzsum, an f64 sum whose order follows the
launch geometry, which is held to 1e-12 relative as in tests/test_gpu_node_pass.py.  The steps run at fr = FR, at which every haplotype of a species
that is present is an LP column of the oracle's strain level: the haplotypes that carry a ratio are pinned to the oracle's, so the ratios cover sums
over whole species and over paths that leave nodes out.

What each class is there for (lines of node_cov_stats_kernel):
  word        `m0`, `m1`, `w0 == w1`, the interior-word loop, and in the long-node variant `below0` and `pw[w1 - wa] - pw[w0 - wa]`; `fw` for the nodes
              whole by the flag and by bits
  neighbours  a lane that counts (or, cleaning, clears) a bit of the node next door: over a wave border, a workgroup border and a species border
  flags       `atomicAnd(&full[v >> 5], ~m)`: a flag word whose nodes belong to several waves
  prefix      `has_long` false inside the long-node kernel; `nw` under 256, 257 .. 512 and over 512 (`carry` over one and two passes of the k loop);
              nw == NCS_PWORDS, which fits, and NCS_PWORDS + 1, which does not, at each residue of (b0 >> 5) & 3; a node longer than the prefix on its
              own; marked bits of the previous wave's node in the stretch's first word; the stretch that ends on bit_off[V]
  dropped     `active[s] == 0`: zeros written without reading, beside neighbours that share a word with the dropped species
  rounds      a wave's second round: the carried `run`, `in0` / `in1` against round_b0, the two atomics over a round's ends (`s_part`, `e_part`,
              `ws == we`), `full[v >> 5] = 0` for a flag word wholly inside one run of lanes

The three instantiations share one timer label; which of them a case ran follows from the options, mirrored on the host (long_node_shape, the cleaning
readers: no zero_fill_kernel in front of the next coverage pass, which cov_arena_verify then checks word by word).
"""
import ctypes as C

import numpy as np
import pytest

from tests import node_count_cases as nc
from tests.helpers import oracle_coverage

pytestmark = pytest.mark.gpu

NCS, FUSED, POP, PLAIN_STATS, FILL = "node_cov_stats_kernel", "node_rows_kernel", "popcount_kernel", "node_stats_kernel", "zero_fill_kernel"
NODE_LABELS = {NCS, FUSED, POP, PLAIN_STATS}
E_STATE = -7
HAS_RATIO = 4
MET_DT = np.dtype([("has", "<u4"), ("is_rescue", "<i4"), ("f", "<f8", (7,))])       # pantax_hip_hap_metrics; f[2] = path_cov_ratio
SPLIT = {"node_pass": "split"}
FR = 0.005                        # the first filter's fraction of unique-trio windows hit: low enough that the multi-path species keep LP columns on these reads


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


class World:
    """a corpus, the oracle's binning, and the oracle's coverage per (dropped species, subset of the reads): made once, shared, never changed"""

    def __init__(self, corpus):
        from oracle import oracle as orc
        self.c = corpus
        rd = corpus.reads
        self.sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in corpus.species], [g.range_end for g in corpus.species])
        self.names = [g.name for g in corpus.species]
        self.haps = [h for g in corpus.species for h in g.hap_names]
        self.default_dropped = () if corpus.dropped is None else (corpus.dropped,)
        self._exp = {}

    def expect(self, dropped, flags=None, key=None):
        k = (tuple(dropped), key)
        if k not in self._exp:
            ref = oracle_coverage(self.c.species, self.c.reads, nc.step_species(self.c, self.sp, dropped), None if flags is None else flags == 0)
            assert all(r[4] == 0 for r in ref)
            bases, cov = np.concatenate([r[1] for r in ref]), np.concatenate([r[2] for r in ref]).astype(np.int64)
            bases.flags.writeable = cov.flags.writeable = False
            self._exp[k] = (bases, cov, self._ratio_haps(ref, dropped))
        return self._exp[k]

    def _ratio_haps(self, ref, dropped):
        """the haplotypes the oracle's strain level gives a path_cov_ratio (its LP columns of the species that are present), as a mask over the db's"""
        from oracle import oracle as orc
        out = []
        for si, (g, (T, b, cv, tb, na)) in enumerate(zip(self.c.species, ref)):
            if si in dropped:
                out += [False] * g.n_paths
                continue
            rc, met, n_cand, o1, o2 = orc.optimize_species(orc.Graph(g.node_len, g.path_off, g.path_nodes), T, b, cv, tb, fr=FR)
            assert rc == 0
            out += [bool(met[k].has & HAS_RATIO) for k in range(g.n_paths)]
        return np.array(out)


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name):
        if name not in made:
            made[name] = World({"edges": lambda: nc.build_edges(False), "edges_long": lambda: nc.build_edges(True), "rounds": nc.build_rounds}[name]())
        return made[name]
    return get


def _timed(eng, fn):
    eng.timing_enable(True)
    eng.timing_reset()
    try:
        out = fn()
        ran = set(eng.timing_get())
    finally:
        eng.timing_enable(False)
    return out, ran


def _raw_step(eng, avg):
    """one resident step with every launch timed -> its results as copies, the names of the kernels that ran"""
    (keep, absolute, met, info, passed, s_all, s_pass), ran = _timed(eng, lambda: eng.profile_step(avg, fr=FR))
    return dict(keep=keep.copy(), absolute=absolute.copy(), met=C.string_at(met, C.sizeof(met[0]) * eng.H), info=C.string_at(info, C.sizeof(info[0]) * eng.S),
                passed=np.array(passed).copy(), ran=ran, stats=eng.strain_node_stats())


def _long_shape(c, options):
    """long_node_shape (cov_plan.hpp) on the host"""
    return int(c.bit_off[-1]) // len(c.node_len) >= int(options.get("ncs_prefix_min", 48)) and not options.get("ncs_no_prefix")


def _check_nodes(w, got_cov, got_ab, bases, cov, what):
    c = w.c
    got_cov = np.asarray(got_cov).astype(np.int64)
    for si in range(len(c.species)):
        lo, hi = int(c.node_base[si]), int(c.node_base[si + 1])
        bad = np.nonzero(got_cov[lo:hi] != cov[lo:hi])[0]
        assert len(bad) == 0, "%s: cov of species %d differs at %d local nodes, first %s: got %s, oracle %s, lengths %s, bit offsets %s" % (
            what, si, len(bad), bad[:8].tolist(), got_cov[lo:hi][bad[:8]].tolist(), cov[lo:hi][bad[:8]].tolist(), c.node_len[lo:hi][bad[:8]].tolist(),
            c.bit_off[lo:hi][bad[:8]].tolist())
    if got_ab is not None:
        ab = bases.astype(np.float64) / c.node_len.astype(np.float64)
        bad = np.nonzero(np.asarray(got_ab).view(np.uint64) != ab.view(np.uint64))[0]
        assert len(bad) == 0, "%s: ab differs at %d nodes, first %s: got %s, numpy %s" % (what, len(bad), bad[:8].tolist(), got_ab[bad[:8]].tolist(), ab[bad[:8]].tolist())


def _check_stats(w, stats, bases, dropped, what):
    c = w.c
    amax, nvalid, nzsum, nzcnt = stats
    for si in range(len(c.species)):
        lo, hi = int(c.node_base[si]), int(c.node_base[si + 1])
        ab = bases[lo:hi].astype(np.float64) / c.node_len[lo:hi].astype(np.float64)
        if si in dropped:
            assert not ab.any()
        assert amax[si] == ab.max() and nvalid[si] == (ab > 0).sum() and nzcnt[si] == (ab > 0).sum(), (what, si)     # min_depth 0: every valid node counts
        ref = float(np.sum(ab[ab > 0]))
        print("%s: species %d nzsum %.17g, numpy %.17g" % (what, si, nzsum[si], ref))
        assert abs(nzsum[si] - ref) <= 1e-12 * abs(ref), (what, si, nzsum[si], ref)


def _check_ratios(w, met_bytes, cov, want_has, dropped, what):
    c = w.c
    met = np.frombuffer(met_bytes, dtype=MET_DT)
    assert np.array_equal((met["has"] & HAS_RATIO) != 0, want_has), (what, (met["has"] & HAS_RATIO) != 0, want_has)     # the oracle's LP columns
    h, n = 0, 0
    for si, g in enumerate(c.species):
        lo = int(c.node_base[si])
        for k in range(g.n_paths):
            if met["has"][h] & HAS_RATIO:
                assert si not in dropped
                path = g.path_nodes[int(g.path_off[k]):int(g.path_off[k + 1])].astype(np.int64)
                s_cov, s_len = int(cov[lo + path].sum()), int(g.node_len[path].sum())
                assert s_cov < 1 << 24 and s_len < 1 << 24                       # both sums are exact in f32: so is the quotient's rounding
                want = float(np.float32(s_cov) / np.float32(s_len))
                assert met["f"][h][2] == want, "%s: path_cov_ratio of haplotype %d (species %d): %r, from the oracle's counts %r" % (what, h, si, met["f"][h][2], want)
                n += 1
            h += 1
    print("%s: %d haplotypes with a path_cov_ratio" % (what, n))
    assert n >= sum(1 for si, g in enumerate(c.species) if g.n_paths == 1 and si not in dropped)    # a single-path species that is present keeps its column
    return n


def _check_step(eng, w, got, dropped, what, flags=None, key=None, ratios=True):
    c = w.c
    bases, cov, ratio_haps = w.expect(dropped, flags, key)
    want_keep = np.ones(len(c.species), dtype=np.uint8)
    want_keep[list(dropped)] = 0
    assert np.array_equal(got["keep"], want_keep), (what, got["keep"])
    got_cov, got_ab = eng.strain_node_cov()
    _check_nodes(w, got_cov, got_ab, bases, cov, what)
    _check_stats(w, eng.strain_node_stats(), bases, dropped, what)
    if ratios:
        _check_ratios(w, got["met"], cov, ratio_haps, dropped, what)


# set, case, options, the long-node variant is expected
STEP_CASES = [
    ("edges", "plain", SPLIT, False),
    ("rounds", "plain", SPLIT, False),
    ("edges", "prefix", dict(SPLIT, ncs_prefix_min=1), True),
    ("edges_long", "prefix", dict(SPLIT, ncs_prefix_min=1), True),
    ("rounds", "prefix", dict(SPLIT, ncs_prefix_min=1), True),
    ("edges_long", "prefix_by_default", {}, True),                   # long nodes on average: the default route is the long-node variant of the split pass
    ("edges_long", "prefix_off", dict(SPLIT, ncs_no_prefix=1), False),
    ("edges", "no_absent_skip", dict(SPLIT, no_absent_skip=1), False),
    ("edges_long", "no_absent_skip", dict(SPLIT, no_absent_skip=1, ncs_prefix_min=1), True),
    ("rounds", "no_absent_skip", dict(SPLIT, no_absent_skip=1), False),
]


@pytest.mark.parametrize("which,case,options,longn", STEP_CASES, ids=["%s-%s" % (c[0], c[1]) for c in STEP_CASES])
def test_counts_per_node(eng, worlds, set_opt, which, case, options, longn):
    w = worlds(which)
    c = w.c
    dropped = (1,) if case == "no_absent_skip" else w.default_dropped          # (`rounds` drops its small species there: the large one's last word is shared with it)
    for opt, value in options.items():
        set_opt(eng, opt, value)
    assert _long_shape(c, options) == longn
    eng.upload_db(c.species)
    eng.upload_packed(c.reads)
    got = _raw_step(eng, nc.avg_len(c, dropped))
    print("%s %s: %s" % (which, case, sorted(got["ran"] & NODE_LABELS)))
    assert got["ran"] & NODE_LABELS == {NCS}, sorted(got["ran"] & NODE_LABELS)
    _check_step(eng, w, got, dropped, "%s %s" % (which, case))
    if case == "no_absent_skip":                                                 # the dropped species was read, and read as zeros
        lo, hi = int(c.node_base[1]), int(c.node_base[2])
        cov, ab = eng.strain_node_cov()
        assert not cov[lo:hi].any() and not ab[lo:hi].any()


@pytest.mark.parametrize("which", ["edges", "rounds"])
def test_fused_pass_keeps_no_counts_and_agrees_with_the_split_pass(eng, worlds, set_opt, which):
    """node_rows_kernel forms the counts inside the row sort and stores neither array: the seam answers E_STATE; what the counts feed -- every metric,
    path_cov_ratio among them, the solve info and the node statistics -- is that of the split pass under the same row sort, byte for byte (nzsum, whose
    order of summation differs between the two launch geometries, to 1e-12), and the ratios equal the oracle's counts."""
    from pantax_amd._ffi import PantaxHipError
    w = worlds(which)
    c = w.c
    dropped = w.default_dropped
    avg = nc.avg_len(c, dropped)
    set_opt(eng, "row_sort", "nodes")
    eng.upload_db(c.species)
    eng.upload_packed(c.reads)
    with pytest.raises(PantaxHipError) as e0:                                    # no step collected yet
        eng.strain_node_cov()
    assert e0.value.code == E_STATE
    eng.set_option("node_pass", "split")
    try:
        split = _raw_step(eng, avg)
        _check_step(eng, w, split, dropped, "%s split under row_sort=nodes" % which)
    finally:
        eng.set_option("node_pass", None)
    fused = _raw_step(eng, avg)
    assert split["ran"] & NODE_LABELS == {NCS} and fused["ran"] & NODE_LABELS == {FUSED}, (sorted(split["ran"] & NODE_LABELS), sorted(fused["ran"] & NODE_LABELS))
    with pytest.raises(PantaxHipError) as e1:
        eng.strain_node_cov()
    assert e1.value.code == E_STATE and "fused" in str(e1.value)
    for k in ("keep", "absolute", "passed"):
        assert np.array_equal(split[k], fused[k]), k
    assert split["met"] == fused["met"] and split["info"] == fused["info"]
    for a, b, name in zip(split["stats"], fused["stats"], ("amax", "nvalid", "nzsum", "nzcnt")):
        if name == "nzsum":
            print("%s: nzsum split %s fused %s" % (which, a.tolist(), b.tolist()))
            assert np.all(np.abs(a - b) <= 1e-12 * np.abs(a))
        else:
            assert a.tobytes() == b.tobytes(), name
    bases, cov, ratio_haps = w.expect(dropped)
    _check_stats(w, fused["stats"], bases, dropped, "%s fused" % which)
    n = _check_ratios(w, fused["met"], cov, ratio_haps, dropped, "%s fused" % which)
    assert n >= 3                                                                # multi-path species among them: sums over paths that leave nodes out


@pytest.mark.parametrize("which", ["edges", "edges_long", "rounds"])
def test_stage_call_on_the_same_marks(eng, worlds, which):
    """popcount_kernel (`edges`, `rounds`) / popcount_long_kernel (`edges_long`: long nodes on average) count the same marks for the stage call; its
    stretches are 64 ALIGNED nodes, of which the corpus reaches all three kinds (tests/test_node_count_cases.py).  A stage count replaces the counts of
    an earlier resident step: the seam says so."""
    from pantax_amd._ffi import PantaxHipError
    w = worlds(which)
    c = w.c
    dropped = w.default_dropped
    eng.upload_db(c.species)
    eng.upload_packed(c.reads)
    eng.set_option("node_pass", "split")
    try:
        got = _raw_step(eng, nc.avg_len(c, dropped))
    finally:
        eng.set_option("node_pass", None)
    cov0, _ = eng.strain_node_cov()                                              # a collected step on the split pass: the seam answers
    active = np.ones(len(c.species), dtype=np.uint8)
    active[list(dropped)] = 0

    def stage():
        sp, *_ = eng.rcls_profile()
        eng.trio_nodes_info(fetch=False)
        return sp, eng.get_node_abundances(species_active=active, with_trio=False)
    (sp, (bases, cov, tb, nab)), ran = _timed(eng, stage)
    assert np.array_equal(sp, w.sp) and nab == 0
    assert ran & NODE_LABELS == {POP}, sorted(ran & NODE_LABELS)
    assert _long_shape(c, {}) == (which == "edges_long")                         # which of the two kernels the label stands for
    e_bases, e_cov, _ = w.expect(dropped)
    assert np.array_equal(bases, e_bases)
    _check_nodes(w, cov, None, e_bases, e_cov, "%s stage" % which)
    assert np.array_equal(cov0.astype(np.int64), e_cov)
    with pytest.raises(PantaxHipError) as e:
        eng.strain_node_cov()
    assert e.value.code == E_STATE and "stage" in str(e.value)


def _clean_plan(w):
    """three samples of one db: all reads; about 40 % of them flagged away and another species dropped; a different subset, the first species dropped again"""
    c = w.c
    rng = np.random.default_rng(11)
    n = c.reads.n_reads
    flags = [None, (rng.random(n) < 0.4).astype(np.uint8), (rng.random(n) < 0.55).astype(np.uint8)]
    drops = [(1,), (2,), (1,)] if len(c.species) > 2 else [(), (1,), ()]
    return flags, drops


@pytest.mark.parametrize("which", ["edges", "rounds"])
def test_cleaning_readers_leave_nothing_and_take_nothing(eng, worlds, set_opt, which):
    """cov_self_clean: node_cov_stats_kernel<true> is the last reader of `bases`, the bit vector and the flags and zeroes what it read.  Three steps on
    one db, each compared with the oracle on that step's reads: a bit an earlier step left behind is extra coverage at its node, a bit cleared from a
    neighbour's share of a word is missing coverage.  cov_arena_verify counts the arena's non-zero words before every coverage pass that skips its
    fill (the step fails with E_STATE if there are any)."""
    from pantax_amd.pipeline import StepConfig, profile_step
    w = worlds(which)
    c = w.c
    flags, drops = _clean_plan(w)
    set_opt(eng, "cov_self_clean", "1")
    set_opt(eng, "cov_arena_verify", "1")
    eng.upload_db(c.species)
    for i, (fl, dr) in enumerate(zip(flags, drops)):
        eng.upload_packed(c.reads, fl)
        got = _raw_step(eng, nc.avg_len(c, dr))
        print("%s clean step %d: %s" % (which, i, sorted(got["ran"] & (NODE_LABELS | {FILL}))))
        assert got["ran"] & NODE_LABELS == {NCS}
        if i:
            assert FILL not in got["ran"]                             # the readers of the step before cleaned: this pass skipped its fill (and verified)
        _check_step(eng, w, got, dr, "%s clean step %d" % (which, i), fl, i)
    # ... and a step under the default options behind them: it fills, and finds what the oracle finds
    eng.set_option("cov_self_clean", None)
    eng.upload_packed(c.reads)
    got = _raw_step(eng, nc.avg_len(c, w.default_dropped))
    assert got["ran"] & NODE_LABELS in ({NCS}, {FUSED})
    if NCS in got["ran"]:
        _check_step(eng, w, got, w.default_dropped, "%s after the cleaning steps" % which)


@pytest.mark.parametrize("which", ["edges", "rounds"])
def test_cleaning_readers_with_steps_in_flight(eng, worlds, set_opt, which):
    """the same three samples through profile_steps_pipelined: step i + 1 is enqueued before step i is collected, so only the last step's arrays can be
    fetched -- they hold what every earlier step left behind -- and every step's tables are those of the same steps one at a time."""
    from pantax_amd.pipeline import StepConfig, profile_step, profile_steps_pipelined
    w = worlds(which)
    c = w.c
    flags, drops = _clean_plan(w)
    set_opt(eng, "cov_self_clean", "1")
    set_opt(eng, "cov_arena_verify", "1")
    eng.upload_db(c.species)
    single = []
    for fl, dr in zip(flags, drops):
        eng.upload_packed(c.reads, fl)
        single.append(profile_step(eng, w.names, w.haps, nc.avg_len(c, dr), StepConfig()))
    avg = nc.avg_len(c, drops[0])

    def swap(i):                                                      # the enqueue reads the species lengths when it is called
        avg[:] = nc.avg_len(c, drops[i])
        eng.upload_packed(c.reads, flags[i])
    got = profile_steps_pipelined(eng, w.names, w.haps, avg, len(flags), StepConfig(), next_input=swap)
    assert len(got) == len(single)
    for a, b in zip(got, single):
        assert a[0] == b[0] and a[1] == b[1]
        for k in ("n_rows", "iters", "n_cand", "n_patterns", "n_active"):
            assert a[2][k] == b[2][k], k
        assert np.array_equal(np.array(a[2]["obj"], dtype=float), np.array(b[2]["obj"], dtype=float), equal_nan=True)
    assert single[0][0] != single[1][0] and len(single[0][0]) == len(c.species) - len(drops[0])       # (the samples differ: another species is missing)
    last = len(flags) - 1
    bases, cov, _ = w.expect(drops[last], flags[last], last)
    got_cov, got_ab = eng.strain_node_cov()
    _check_nodes(w, got_cov, got_ab, bases, cov, "%s pipelined, last step" % which)
    _check_stats(w, eng.strain_node_stats(), bases, drops[last], "%s pipelined, last step" % which)
    (rows, ran) = _timed(eng, lambda: profile_step(eng, w.names, w.haps, avg, StepConfig()))     # one more step: it finds the arena clean
    assert NCS in ran and FILL not in ran and FUSED not in ran, sorted(ran & (NODE_LABELS | {FILL}))
    assert rows[0] == single[last][0] and rows[1] == single[last][1]
