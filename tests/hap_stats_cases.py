"""Crafted unique-trio abundances for the a9 statistics (profile.rs:1028-1051, :1114-1182): one species whose unique-trio windows the test steers
one by one.

The graph.  Backbone nodes b_0, b_1, ... shared by every haplotype, and for every haplotype h and site k a private node p_{h,k}; walk h is
b_0, p_{h,0}, b_1, p_{h,1}, ... over nt + 2 nodes.  Every window of three consecutive nodes of walk h holds a private node of h, so it occurs in no other
walk: nt unique trios per haplotype, window w = nodes w, w+1, w+2 of the walk.  Every node is NODE_LEN long, every window 3 * NODE_LEN.

The reads.  A read is a walk over the three nodes of one window with chosen pstart / pend; it adds pend - pstart to that window's trio_bases
(profile.rs:890-907) and to nothing else that is unique.  A plan gives, per haplotype and window, (n reads, bases per read): the window's abundance is
n * bases / (3 * NODE_LEN).  The generator never assumes the table or the sums: the oracle builds both (orc.TrioTable, orc.node_coverage), and
`Case.reference()` reads every expectation from them.

Two references per case:
  * orc.hap_trio_stats / orc.optimize_species: the project's sequential f64 reading of the reference -- the parity target of the device;
  * `exact_stats`: the same statistics in fractions.Fraction (mean, variance, every z^2 against 9).  It judges the INPUTS: a case is admitted only when
    no |z| lies within 1e-6 (relative) of 3, the variance is exactly 0 or clearly positive (sd >= 1e-3 of the mean: abundances are quotients of small
    integers, f64 carries 1e-16), and the first filter's fraction is either exactly its threshold -- one correctly rounded f64 division on both sides --
    or 1e-6 away from it.  tests/test_hap_stats_cases.py asserts that for every case, without a GPU.

The degenerate haplotypes (`Case.degenerate`): all non-zero abundances EQUAL but not representable in f64.  In exact arithmetic the variance is 0 and the
filtered mean 0.0.  The reference sums sequentially (data.iter().sum()), and c sequential additions of x divided by c need not give x back: then sd is
a rounding residue, every |z| is about 1, and the filtered mean is x (to an ulp).  Every order of equal values gives that same sum, so the reference's
answer is deterministic, and it depends on the SHAPE of the sum: a pairwise tree over the same values can land on the other side.  `degenerate_pairs`
searches (count, reads, bases) where the two shapes disagree about mean == x, in both directions; the oracle's answer is the expected one.
"""
import functools
from fractions import Fraction

import numpy as np

NODE_LEN = 100
WIN_LEN = 3 * NODE_LEN
Z_MARGIN = 1e-6          # relative distance of every |z| from 3 (exact arithmetic)
SD_FLOOR = 1e-3          # "clearly positive": sd >= SD_FLOOR * mean
FRAC_MARGIN = 1e-6       # relative distance of a fraction from its threshold unless it is exactly there


# --------------------------------------------------------------------------------------------------------------------------- the graph and the reads
def crafted_species(name, H, nt, range_start, prefix="GCF_8"):
    """-> synthdata.SpeciesGraph of H walks over nt + 2 alternating backbone / private nodes (nt unique-trio windows per haplotype)."""
    import synthdata as synth
    assert H >= 2 and nt >= 1
    L = nt + 2
    nb, npv = (L + 1) // 2, L // 2
    V = nb + H * npv
    node_len = np.full(V, NODE_LEN, dtype=np.int64)
    i = np.arange(L)
    walks = np.where(i % 2 == 0, i // 2, 0)[None, :].repeat(H, axis=0)
    priv = nb + np.arange(H)[:, None] * npv + (i[None, :] // 2)
    walks = np.where((i % 2 == 1)[None, :], priv, walks).astype(np.uint32)
    path_off = (np.arange(H + 1) * L).astype(np.uint64)
    names = sorted("%s%s%05d.1" % (prefix, name, h) for h in range(H))
    return synth.SpeciesGraph(name, node_len, path_off, walks.reshape(-1), names, range_start, range_start + V - 1,
                              np.full(H, L * NODE_LEN, dtype=np.int64), np.zeros(H))


def window_reads(g, plan):
    """plan {h: {w: (n, bases)}} -> list of (three global node ids, pstart, pend) -- n reads of `bases` bases over window w of walk h."""
    L = int(g.path_off[1] - g.path_off[0])
    out = []
    for h in sorted(plan):
        walk = g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].astype(np.int64) + g.range_start
        for w in sorted(plan[h]):
            n, bases = plan[h][w]
            assert 0 <= w < L - 2 and NODE_LEN + 2 <= bases <= WIN_LEN, (h, w, n, bases)
            first = min(NODE_LEN, bases - NODE_LEN - 1)              # bases on the first node; the middle node whole; the rest on the last
            ps = NODE_LEN - first
            out += [(tuple(walk[w:w + 3]), ps, ps + bases)] * n
    return out


def pack_reads(read_lists, seed):
    """lists of (nodes, pstart, pend) -> synthdata.PackedReads, shuffled (species interleave like a real GAF); qlen = bases, MAPQ 60."""
    import synthdata as synth
    reads = [r for lst in read_lists for r in lst]
    order = np.random.default_rng(seed).permutation(len(reads))
    reads = [reads[i] for i in order]
    ns = np.array([len(r[0]) for r in reads], dtype=np.int64)
    step_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    step_off[1:] = np.cumsum(ns)
    node_id = np.array([v for r in reads for v in r[0]], dtype=np.uint32)
    ps = np.array([r[1] for r in reads], dtype=np.int64)
    pe = np.array([r[2] for r in reads], dtype=np.int64)
    ql = pe - ps
    return synth.PackedReads(step_off, node_id, np.zeros(len(node_id), dtype=np.uint8), ps, pe, ql, np.full(len(reads), 60, dtype=np.int64), ql.copy(), [])


def single_strain_species(name, range_start, n_reads=40):
    """A one-walk species (a chain of 1024-bp chunks) and a few two-node reads on it: no unique trio, one LP column."""
    import synthdata as synth
    g = synth.make_species(np.random.default_rng(5), name, 1, 5000, range_start, "GCF_7%s" % name)
    reads = [((g.range_start + k % 3, g.range_start + k % 3 + 1), 1000, 1150) for k in range(n_reads)]
    return g, reads


# --------------------------------------------------------------------------------------------------------------------------- exact restatement
def exact_stats(tb, ln):
    """trio_bases and window lengths of ONE haplotype's unique trios (integers) -> dict in exact arithmetic:
    nnz, mean, var, z2 (every value's z^2, None where var == 0), kept (|z| < 3), mean_filtered (0 where var == 0 or nothing is kept)."""
    x = [Fraction(int(t), int(l)) for t, l in zip(tb, ln) if int(t) > 0]
    n = len(x)
    if n == 0:
        return dict(nnz=0, mean=Fraction(0), var=Fraction(0), z2=[], kept=[], mean_filtered=Fraction(0), values=x)
    mean = sum(x, Fraction(0)) / n
    var = sum(((v - mean) ** 2 for v in x), Fraction(0)) / n
    if var == 0:
        return dict(nnz=n, mean=mean, var=var, z2=None, kept=[], mean_filtered=Fraction(0), values=x)
    z2 = [(v - mean) ** 2 / var for v in x]
    kept = [v for v, z in zip(x, z2) if z < 9]
    return dict(nnz=n, mean=mean, var=var, z2=z2, kept=kept, mean_filtered=sum(kept, Fraction(0)) / len(kept) if kept else Fraction(0), values=x)


def shift_threshold(fr, fm, shift):
    """the first filter's threshold as the reference forms it in f64 (profile.rs:1140-1168)"""
    if not shift:
        return fr
    if fm >= 1.0:
        sh = fr + (0.8 - fr) * fm / 100.0
        return 0.8 if sh > 0.8 else sh
    return fr * fm


def seq_sum(x, c):
    s = 0.0
    for _ in range(c):
        s += x
    return s


def tree_sum(x, c):
    v = [x] * c
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


@functools.lru_cache(maxsize=None)
def degenerate_pairs(max_count):
    """(count, reads, bases) with count equal abundances x = reads * bases / WIN_LEN for which a sequential sum and a pairwise tree disagree about
    sum / count == x -> (those where only the SEQUENTIAL mean misses x: the reference answers x, those where only the TREE misses x: it answers 0.0)"""
    seq_off, tree_off = [], []
    for c in range(3, max_count + 1):
        for n in (1, 2, 3):
            for bases in range(NODE_LEN + 2, WIN_LEN + 1):
                x = float(n * bases) / float(WIN_LEN)
                if x * WIN_LEN == n * bases and Fraction(x) == Fraction(n * bases, WIN_LEN):
                    continue                                         # representable: not this case
                s, t = seq_sum(x, c) / c == x, tree_sum(x, c) / c == x
                if s != t:
                    (tree_off if s else seq_off).append((c, n, bases))
    return seq_off, tree_off


# --------------------------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, species, read_lists, fr=0.3, shift=False, degenerate=(), dropped=(), seed=1):
        self.name, self.species, self.fr, self.shift = name, species, fr, shift
        self.reads = pack_reads(read_lists, seed)
        self.degenerate = set(degenerate)          # (species, haplotype): equal, non-representable abundances
        self.dropped = tuple(dropped)              # species the species level is made to drop (no genome length)
        self.hap_off = np.concatenate([[0], np.cumsum([g.n_paths for g in species])]).astype(np.int64)
        self._ref = None

    @property
    def H(self):
        return int(self.hap_off[-1])

    def avg_len(self):
        avg = np.array([float(g.genome_len.mean()) for g in self.species])
        for s in self.dropped:
            avg[s] = 0.0
        return avg

    def reference(self):
        """Computed once, shared by every test of the case, never modified: per species the oracle's graph, table, coverage and a9 statistics, and
        over the whole db nt / nnz / mean_filtered [H], the first filter's n_candidates [S] and the `has` bits [H] of orc.optimize_species."""
        if self._ref is None:
            from oracle import oracle as orc
            from tests.helpers import select_reads
            rd = self.reads
            sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in self.species], [g.range_end for g in self.species])
            counts = orc.species_counts(sp, rd.qlen, rd.mapq, len(self.species))
            keep, absolute, _ = orc.species_profile(sp, rd.qlen, counts, self.avg_len())
            nt, nnz, mf = np.zeros(self.H, dtype=np.int64), np.zeros(self.H, dtype=np.int64), np.zeros(self.H)
            has, ncand, per = np.zeros(self.H, dtype=np.uint32), np.zeros(len(self.species), dtype=np.int64), []
            stat = np.zeros(self.H, dtype=bool)                          # haplotypes whose a9 statistics the reference defines
            for s, g in enumerate(self.species):
                G = orc.Graph(g.node_len, g.path_off, g.path_nodes)
                T = orc.TrioTable(G)
                so, nid, ps, pe = select_reads(rd, np.nonzero(sp == s)[0])
                b, c, t, n_abort = orc.node_coverage(G, T, g.range_start, so, nid, ps, pe)
                assert n_abort == 0
                h0, h1 = self.hap_off[s], self.hap_off[s + 1]
                trio_mode = g.n_paths != 1 and T.n_unique != 0          # profile.rs:1098: only then are the statistics taken at all
                a, z, m = orc.hap_trio_stats(T, g.n_paths, t) if trio_mode else (np.zeros(g.n_paths),) * 3
                if keep[s]:
                    nt[h0:h1], nnz[h0:h1], mf[h0:h1] = a, z, m
                    stat[h0:h1] = trio_mode
                    rc, omet, nc, o1, o2 = orc.optimize_species(G, T, b, c, t, fr=self.fr, shift=self.shift)
                    assert rc == 0, (self.name, s)
                    ncand[s] = nc
                    has[h0:h1] = [omet[h].has & 3 for h in range(g.n_paths)]
                per.append(dict(G=G, T=T, bases=b, cov=c, tb=t, nt=np.asarray(a).astype(np.int64)))
            self._ref = dict(sp=sp, counts=counts, keep=keep, absolute=absolute, nt=nt, nnz=nnz, mean_filtered=mf, has=has, n_candidates=ncand, species=per, stat=stat)
        return self._ref

    def hap_windows(self, s, h):
        """(trio_bases, window length) of the unique trios of haplotype h of species s, as the oracle filed and counted them"""
        r = self.reference()["species"][s]
        b, e = int(r["T"].hap_off[h]), int(r["T"].hap_off[h + 1])
        return r["tb"][b:e], r["T"].len[b:e]


def chunk_rows(Hs, total_rows):
    """rows per chunk of a species of Hs haplotypes in a db of total_rows unique-trio rows: the rule of hap_stats_layout as the library documents it --
    1024 rows where that gives thousands of chunks, down to 128 in small dbs, and at least eight rows per haplotype, in whole stretches of 64"""
    ceil64 = lambda n: (n + 63) // 64 * 64
    return max(min(1024, max(128, ceil64(total_rows // 4096))), ceil64(8 * Hs))


def chunk_table(case, s=0):
    """Species s with its rows in the oracle's table order -- walk after walk, the order of the route that files rows by the pass over the walks -- cut into
    chunks -> per chunk (rows, non-zero rows, set of haplotypes with a row in it).  tests/test_hap_stats_cases.py pins the layout claims of the cases with it."""
    r = case.reference()
    sp = r["species"][s]
    total = sum(int(x["T"].n_unique) for x in r["species"] if x["G"].n_paths > 1)
    per = chunk_rows(case.species[s].n_paths, total)
    U = int(sp["T"].n_unique)
    return [(min(U, a + per) - a, int((sp["tb"][a:a + per] > 0).sum()), set(sp["T"].hap[a:a + per].tolist())) for a in range(0, U, per)]


def _varied(h, w):
    return (1 + (h * 7 + w * 3) % 5, NODE_LEN + 2 + (h * 13 + w * 29) % (WIN_LEN - NODE_LEN - 1))


def _route_plan(haps, nt, outliers=True):
    """every listed haplotype: varied windows, a quarter of them empty; every third one carries one window far above the others"""
    plan = {}
    for h in haps:
        plan[h] = {w: _varied(h, w) for w in range(nt) if (h + w) % 4 != 3}
        if outliers and h % 3 == 0:
            plan[h][0] = (60, 250)
    return plan


def _one(name, H, nt, plan, with_single=False, **kw):
    g = crafted_species("1", H, nt, 1)
    species, lists = [g], [window_reads(g, plan)]
    if with_single:
        g1, r1 = single_strain_species("2", g.range_end + 1)
        species.append(g1)
        lists.append(r1)
    return Case(name, species, lists, **kw)


def _case_count(H):
    """the routes of hap_rows_pass_kernel by haplotype count: <= 16 one register slab, 17..64 lane-owned, 65..1024 LDS, beyond the chunk's global row"""
    if H >= 1024:                                # a handful of haplotypes covered, at the ends of every 64 and of the table: the LP stays a few columns wide
        haps = [h for h in (0, 63, 64, 1023, 1024) if h < H]
        return _one("count_%d" % H, H, 9, _route_plan(haps, 9, outliers=False))      # 9 windows: more than ceil64(8 H) rows, two chunks
    return _one("count_%d" % H, H, 15, _route_plan(range(H), 15), with_single=H in (17, 65))


def _case_mixed():
    """1025, 70 and 3 haplotypes in one db: the LDS size comes from the 70, the global rows and their zero fill from the 1025"""
    a = crafted_species("1", 1025, 9, 1)
    b = crafted_species("2", 70, 5, a.range_end + 1)
    c = crafted_species("3", 3, 7, b.range_end + 1)
    return Case("mixed_1025_70_3", [a, b, c], [window_reads(a, _route_plan([0, 63, 64, 1023, 1024], 9, outliers=False)),
                                               window_reads(b, _route_plan(range(70), 5, outliers=False)), window_reads(c, _route_plan(range(3), 7, outliers=False))])


def _case_chunks(dense):
    """13 x 23 = 299 rows: chunks of 128, 128 and 43 rows (not a multiple of 64).  dense: every row non-zero (the 128-entry queue of pass 0 drains full
    batches).  sparse: filed walk by walk, one non-zero row in the first chunk, none in the second, and haplotype 12 -- all of whose rows lie in the
    last, partial chunk -- covered whole."""
    H, nt = 13, 23
    if dense:
        plan = {h: {w: _varied(h, w) for w in range(nt)} for h in range(H)}
    else:
        plan = {2: {5: (2, 170)}, 12: {w: _varied(12, w) for w in range(nt)}}
    return _one("chunks_dense" if dense else "chunks_sparse", H, nt, plan)


def _case_filters():
    nt = 13
    plan = {
        0: {**{w: (1, 150) for w in range(12)}, 12: (40, 150)},     # 12 x 0.5 and one 20.0: z = sqrt(12) = 3.46, dropped
        # nine values: the outlier's z is sqrt(8) = 2.83 and no |z| of n values exceeds sqrt(n - 1) -- kept.  (With ten values the outlier sits at
        # z = 3 exactly and with eleven beyond it, so nine is the largest count at which no |z| can reach 3.)
        1: {**{w: (1, 150) for w in range(8)}, 12: (40, 150)},
        2: {4: (3, 200)},                                           # one non-zero window: sd == 0 -> 0.0
        3: {w: (1, 300) for w in range(nt)},                        # all 1.0
        4: {w: (2, 300) for w in range(5)},                         # all 2.0
        5: {w: _varied(5, w) for w in range(nt)},
    }
    return _one("filters", 6, nt, plan, with_single=True)


def _case_degenerate(name, H, nt, which):
    """every haplotype: `count` windows of the same non-representable abundance, counts and ratios from degenerate_pairs -- alternately one the
    sequential sum misses (reference: x) and one only the tree misses (reference: 0.0)"""
    seq_off, tree_off = degenerate_pairs(nt)
    assert seq_off and tree_off
    plan = {}
    for h in range(H):
        src = seq_off if h % 2 == 0 else tree_off
        c, n, bases = which(src, h)
        ws = [(w * 7 + h) % nt for w in range(nt)][:c] if nt % 7 else list(range(c))   # the count windows spread over the walk
        plan[h] = {w: (n, bases) for w in ws}
    return _one(name, H, nt, plan, degenerate=[(0, h) for h in range(H)])


def _spread(src, h):
    """entries of `src` with different counts, small and large"""
    by_c = sorted({e[0]: e for e in src}.values())
    return by_c[(h // 2 * 5) % len(by_c)]


def _largest(src, h):
    return max(src)


def _case_thresholds(shift):
    nt = 10
    if not shift:
        plan = {0: {w: _varied(0, w) for w in (1, 4, 8)},            # 3 of 10 == fr: kept (frac < fr is false)
                1: {w: _varied(1, w) for w in (2, 7)},               # one window short: dropped
                2: {w: _varied(2, w) for w in range(nt)},
                3: {w: _varied(3, w) for w in (0, 5, 9)}}
        return _one("thresholds", 4, nt, plan)
    plan = {0: {1: (1, 294), 4: (1, 300), 8: (1, 297)},             # fm = 0.99 < 1: threshold fr * fm = 0.297 <= 3/10 -- kept
            1: {2: (1, 150), 5: (1, 300), 7: (3, 150)},             # fm = 1.0 exactly: threshold fr + (0.8 - fr) / 100 = 0.305 > 3/10 -- dropped
            2: {w: (150 + 100 * (w % 2), 300) for w in range(8)},   # fm = 200: the threshold is clamped to 0.8 == 8/10 -- kept
            3: {w: (150 + 100 * (w % 2), 300) for w in range(7)},   # 7/10 < 0.8 -- dropped
            4: {3: (1, 225), 6: (1, 150)},                          # fm = 0.625: fr * fm = 0.1875 <= 2/10 -- kept (dropped without the shift)
            5: {3: (1, 240), 6: (1, 300)},                          # fm = 0.9: fr * fm = 0.27 > 2/10 -- dropped
            6: {5: (2, 180)}}                                       # one window: fm = 0.0, threshold 0.0 -- kept, with frequencies_mean 0.0
    return _one("thresholds_shift", 7, nt, plan, shift=True)


def _case_dropped():
    """three species, the middle one without a genome length: the species level drops it (avg_len = 0), the resident step skips its rows"""
    a = crafted_species("1", 3, 7, 1)
    b = crafted_species("2", 5, 7, a.range_end + 1)
    c = crafted_species("3", 2, 9, b.range_end + 1)
    lists = [window_reads(g, {h: {w: _varied(h + i, w) for w in range(int(g.path_off[1]) - 2)} for h in range(g.n_paths)}) for i, g in enumerate((a, b, c))]
    return Case("dropped_species", [a, b, c], lists, dropped=(1,))


BUILDERS = {
    **{"count_%d" % H: functools.partial(_case_count, H) for H in (2, 16, 17, 64, 65, 1024, 1025)},
    "mixed_1025_70_3": _case_mixed,
    "chunks_dense": functools.partial(_case_chunks, True),
    "chunks_sparse": functools.partial(_case_chunks, False),
    "filters": _case_filters,
    "degenerate_4": functools.partial(_case_degenerate, "degenerate_4", 4, 23, _spread),        # one register slab
    "degenerate_16": functools.partial(_case_degenerate, "degenerate_16", 16, 23, _spread),
    "degenerate_2x64": functools.partial(_case_degenerate, "degenerate_2x64", 2, 64, _largest),  # up to 64 equal values (the one case beyond 12 sites)
    "degenerate_17": functools.partial(_case_degenerate, "degenerate_17", 17, 23, _spread),      # lane-owned sums, 391 rows in chunks of 192
    "degenerate_40": functools.partial(_case_degenerate, "degenerate_40", 40, 23, _spread),      # 920 rows in chunks of 320
    "thresholds": functools.partial(_case_thresholds, False),
    "thresholds_shift": functools.partial(_case_thresholds, True),
    "dropped_species": _case_dropped,
}
STEP_CASES = ("dropped_species",)                 # driven through the resident step (profile_step); the others through the stage calls
CASE_NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def get_case(name):
    return BUILDERS[name]()


def admit(case):
    """The conditions on the inputs, in exact arithmetic -> list of violations (empty: admitted).  Also the agreement of the oracle with the exact
    restatement: counts and kept / dropped decisions equal, means to 1e-12 -- except the degenerate haplotypes, where the exact variance is 0 by
    construction and the oracle's answer is either 0.0 or the common value (to 1e-12), whichever its sequential sum gives."""
    ref, bad = case.reference(), []
    for s, g in enumerate(case.species):
        if not ref["stat"][int(case.hap_off[s])]:
            continue
        for h in range(g.n_paths):
            gh = int(case.hap_off[s]) + h
            tb, ln = case.hap_windows(s, h)
            e = exact_stats(tb, ln)
            where = "%s species %d haplotype %d" % (case.name, s, h)
            if e["nnz"] != ref["nnz"][gh] or len(tb) != ref["nt"][gh]:
                bad.append("%s: counts %d/%d, oracle %d/%d" % (where, e["nnz"], len(tb), ref["nnz"][gh], ref["nt"][gh]))
            got = float(ref["mean_filtered"][gh])
            if (s, h) in case.degenerate:
                x = float(e["mean"])
                if e["var"] != 0 or e["nnz"] < 3 or Fraction(x) == e["mean"]:
                    bad.append("%s: not a degenerate haplotype (var %s, nnz %d)" % (where, e["var"], e["nnz"]))
                if not (got == 0.0 or abs(got - x) <= 1e-12 * x):
                    bad.append("%s: oracle %r is neither 0.0 nor the common value %r" % (where, got, x))
            else:
                if e["var"] != 0:
                    if e["var"] < (SD_FLOOR * e["mean"]) ** 2:
                        bad.append("%s: variance %g not clearly positive" % (where, float(e["var"])))
                    near = [z for z in e["z2"] if abs(z / 9 - 1) < 2 * Z_MARGIN]      # |z| within Z_MARGIN of 3 <=> z^2 within 2 Z_MARGIN of 9
                    if near:
                        bad.append("%s: |z| = %r too close to 3" % (where, [float(z) ** 0.5 for z in near]))
                want = float(e["mean_filtered"])
                if abs(got - want) > 1e-12 * max(abs(want), 1e-300):
                    bad.append("%s: oracle mean %r, exact %r" % (where, got, want))
            if len(tb) == 0:
                continue
            frac = float(e["nnz"]) / float(len(tb))
            thr, thr_exact = shift_threshold(case.fr, got, case.shift), shift_threshold(case.fr, float(e["mean_filtered"]) if (s, h) not in case.degenerate else got, case.shift)
            if frac != thr and abs(frac - thr) < FRAC_MARGIN * max(thr, 1e-300):
                bad.append("%s: fraction %r within %g of its threshold %r" % (where, frac, FRAC_MARGIN, thr))
            if (frac < thr) != (frac < thr_exact) or bool(ref["has"][gh] & 2) != (not frac < thr):
                bad.append("%s: first-filter decision: fraction %r, threshold %r / %r, oracle has %d" % (where, frac, thr, thr_exact, ref["has"][gh]))
    return bad
