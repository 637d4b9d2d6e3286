"""The corpus of tests/node_count_cases.py on the CPU: its numpy model equals the C oracle's coverage bit for bit on every set, every class holds what
the GPU cases (tests/test_gpu_node_count.py) count on -- checked against the launch geometry of the node pass as the module mirrors it -- and the sets
keep their size limits."""
import numpy as np
import pytest

from tests import node_count_cases as nc
from tests.helpers import oracle_coverage


def _world(corpus):
    from oracle import oracle as orc
    rd = corpus.reads
    sp = orc.bin_reads(rd.step_off, rd.node_id, [g.range_start for g in corpus.species], [g.range_end for g in corpus.species])
    bases, cov, covered = nc.model(corpus, sp)
    return SimpleWorld(corpus, sp, bases, cov, covered)


class SimpleWorld:
    def __init__(self, c, sp, bases, cov, covered):
        self.c, self.sp, self.bases, self.cov, self.covered = c, sp, bases, cov, covered


@pytest.fixture(scope="module")
def edges():
    return _world(nc.build_edges(False))


@pytest.fixture(scope="module")
def edges_long():
    return _world(nc.build_edges(True))


@pytest.fixture(scope="module")
def rounds():
    return _world(nc.build_rounds())


def _equals_oracle(w, sp, keep=None):
    c = w.c
    bases, cov, _ = nc.model(c, sp, keep)
    ref = oracle_coverage(c.species, c.reads, sp, keep)
    for si in range(len(c.species)):
        lo, hi = int(c.node_base[si]), int(c.node_base[si + 1])
        assert np.array_equal(ref[si][1], bases[lo:hi]) and np.array_equal(ref[si][2].astype(np.int64), cov[lo:hi]) and ref[si][4] == 0, si
    return ref


@pytest.mark.parametrize("which", ["edges", "edges_long", "rounds"])
def test_model_equals_the_oracle(which, request):
    w = request.getfixturevalue(which)
    c = w.c
    ref = _equals_oracle(w, w.sp)
    assert sum(r[0].n_unique for r in ref) > 0                      # U != 0: without it cov_clean_plan never chooses the cleaning readers
    assert (w.sp >= 0).all() and all((w.sp == s).sum() > 100 for s in range(len(c.species)))
    # ... and on a step's view of the reads: a dropped species, a subset
    keep = np.random.default_rng(3).random(c.reads.n_reads) < 0.6
    _equals_oracle(w, nc.step_species(c, w.sp, (1,)), keep)


@pytest.mark.parametrize("which", ["edges", "edges_long", "rounds"])
def test_sizes_and_the_species_level(which, request):
    from oracle import oracle as orc
    w = request.getfixturevalue(which)
    c = w.c
    V, L = len(c.node_len), int(c.bit_off[-1])
    if which == "rounds":
        assert 262144 < c.n_nodes[0] and V < 300000 and c.node_len[:c.n_nodes[0]].max() <= 8 and c.species[0].n_paths == 3
    else:
        assert 8192 <= V < 16384 and len(c.species) == 4
        assert (L // V < 48) == (which == "edges")                  # long_node_shape: the default route of `edges` is the per-lane variant
    assert c.node_len.min() >= 1
    assert all(int(g.genome_len.max()) < 1 << 24 for g in c.species)              # the f32 quotient of path_cov_ratio is exact
    rd = c.reads
    counts = orc.species_counts(w.sp, rd.qlen, rd.mapq, len(c.species))
    keep, _, _ = orc.species_profile(w.sp, rd.qlen, counts, nc.avg_len(c))
    assert keep.all()                                                # every species is kept by the species level ...
    if c.dropped is not None:
        keep, _, _ = orc.species_profile(w.sp, rd.qlen, counts, nc.avg_len(c, (c.dropped,)))
        assert not keep[c.dropped] and keep.sum() == len(c.species) - 1           # ... but the one without a genome length
    k = np.diff(rd.step_off.astype(np.int64))
    assert set(k[c.classes["walks"]].tolist()) == {3, 4, 5} and (k[np.setdiff1d(np.arange(rd.n_reads), c.classes["walks"])] == 1).all()
    assert sorted(np.concatenate(list(c.classes.values())).tolist()) == list(range(rd.n_reads))


def _border_words(w, rows):
    """of the waves `rows`: how many begin inside a word of the bit vector, and in how many of those the word carries marks on both sides"""
    c = w.c
    b = c.bit_off[rows[:, 3]]
    inside = b % 32 != 0
    both = 0
    for x in b[inside]:
        both += bool(w.covered[x - x % 32:x].any() and w.covered[x:x - x % 32 + 32].any())
    return int(inside.sum()), both


@pytest.mark.parametrize("which", ["edges", "edges_long"])
def test_edges_geometry_shares_nearly_every_word(which, request):
    w = request.getfixturevalue(which)
    c = w.c
    geo = nc.geometry(c.n_nodes)
    assert all(k == nc.STAT_CHUNKS for k, per in geo)
    assert all(3 <= -(-per // 4) <= 6 for k, per in geo), geo
    wv = c.waves
    first = np.concatenate([[True], wv[1:, 0] != wv[:-1, 0]])
    wave_b, wg_b = wv[(wv[:, 2] > 0)], wv[(wv[:, 2] == 0) & ~first]
    n_in, n_both = _border_words(w, wave_b)
    g_in, g_both = _border_words(w, wg_b)
    print("%s: wave borders %d, inside a word %d, marks on both sides %d; workgroup borders %d, inside %d, both %d" % (
        which, len(wave_b), n_in, n_both, len(wg_b), g_in, g_both))
    assert n_in > 0.85 * len(wave_b) and g_in > 0.85 * len(wg_b)
    assert n_both >= 500 and g_both >= 150
    if which == "edges":
        L, words = int(c.bit_off[-1]), set()
        for x in c.bit_off[wv[:, 3]]:
            if x % 32:
                words.add(int(x) >> 5)
        short = c.bit_off[c.word_end]                               # behind A's word class the nodes are short: there nearly every word is shared
        assert len([x for x in words if x * 32 >= short]) > 0.9 * ((L - short) // 32)


def test_word_class(edges):
    w, c = edges, edges.c
    seen = set()
    spans = set()
    for v, L, a, p in c.named["word"]:
        assert c.node_len[v] == L and c.bit_off[v] % 32 == a
        want = (1, 1, L - 1, L - 1, L, L)[p]
        assert w.cov[v] == want, (v, L, a, p)
        b0, b1 = int(c.bit_off[v]), int(c.bit_off[v + 1])
        if p == 2 and L > 1:
            assert not w.covered[b0] and w.covered[b0 + 1:b1].all()
        if p == 3 and L > 1:
            assert not w.covered[b1 - 1] and w.covered[b0:b1 - 1].all()
        spans.add(((b1 - 1) >> 5) - (b0 >> 5) + 1)
        seen.add((L, a, p))
    assert seen == {(L, a, p) for L in nc.WORD_LENS for a in range(32) for p in range(nc.N_PATTERNS)}
    assert spans == {1, 2, 3, 4, 5}                                  # w0 == w1, two words, and one to three interior words
    # beside a crafted node the neighbours' bits are there too: the filler in front ends marked, the one behind begins marked, often enough
    vs = np.array([v for v, L, a, p in c.named["word"]])
    assert w.covered[c.bit_off[vs] - 1].sum() > 0.4 * len(vs) and w.covered[c.bit_off[vs + 1]].sum() > 0.2 * len(vs)
    assert (c.node_base[0] <= vs).all() and (vs < c.node_base[1]).all()


def test_neighbours_class(edges):
    w, c = edges, edges.c
    wv = c.waves
    wlo = {int(r[3]): (int(r[0]), int(r[1]), int(r[2])) for r in wv}
    kinds = {}
    for u, a, which, kind in c.named["neighbours"]:
        x = int(c.bit_off[u + 1])
        assert x % 32 == a != 0                                      # the two nodes meet inside a word
        assert bool(w.covered[x - 1]) == (which == 0) and bool(w.covered[x]) == (which == 1)
        assert 0 < w.cov[u] < c.node_len[u] or c.node_len[u] == 2
        s, ch, wave = wlo[u + 1]                                     # u + 1 begins a wave: u belongs to the wave in front
        if kind == "wave":
            assert wave > 0
        elif kind == "workgroup":
            assert wave == 0 and ch > 0
        else:
            assert wave == 0 and ch == 0 and u + 1 == c.node_base[s] and s > 0
        kinds.setdefault((kind, s), set()).add(which)
    for s in (1, 2):
        assert kinds[("wave", s)] == kinds[("workgroup", s)] == {0, 1}
    assert {s for k, s in kinds if k == "species"} == {1, 2, 3}
    assert sum(1 for x in c.named["neighbours"] if x[3] == "wave") >= 80 and sum(1 for x in c.named["neighbours"] if x[3] == "workgroup") >= 70


def test_flags_class(edges):
    w, c = edges, edges.c
    fl = np.array(c.named["flags"])
    assert (w.cov[fl] == c.node_len[fl]).all() and len(c.named["flags_bits"]) >= 20
    wave_of = np.zeros(len(c.node_len), dtype=np.int64)
    for i, r in enumerate(c.waves):
        wave_of[r[3]:r[4]] = i
    per_species = {1: 0, 2: 0}
    for word in np.unique(fl >> 5):
        mine = fl[fl >> 5 == word]
        assert len(set(wave_of[mine].tolist())) >= 4                 # the flags of one `full` word belong to several waves: the atomicAnd arm
        s = int(np.searchsorted(c.node_base, word * 32, side="right")) - 1
        per_species[s] += 1
    assert per_species[1] >= 4 and per_species[2] >= 4
    assert any(len(fl[fl >> 5 == word]) == 32 for word in np.unique(fl >> 5)) and any(len(fl[fl >> 5 == word]) < 32 for word in np.unique(fl >> 5))
    rd = c.reads
    so = rd.step_off.astype(np.int64)
    for u in c.named["flags_bits"][:10]:                             # whole by the flag AND marked bit by bit
        mine = [r for r in c.classes["flags"] if rd.node_id[so[r]] == u + 1]
        assert len(mine) == 2


def test_dropped_class(edges):
    w, c = edges, edges.c
    s = c.dropped
    assert 0 < s < len(c.species) - 1 and (w.sp == s).sum() > 500
    for x in (int(c.bit_off[c.node_base[s]]), int(c.bit_off[c.node_base[s + 1]])):
        assert x % 32 != 0 and w.covered[x - x % 32:x].any() and w.covered[x:x - x % 32 + 32].any()      # a word shared with each active neighbour
    bases, cov, _ = nc.model(c, nc.step_species(c, w.sp, (s,)))
    lo, hi = int(c.node_base[s]), int(c.node_base[s + 1])
    assert not bases[lo:hi].any() and not cov[lo:hi].any() and w.cov[lo:hi].sum() > 1000 and cov[:lo].sum() > 0 and cov[hi:].sum() > 0


def test_prefix_class(edges_long):
    w, c = edges_long, edges_long.c
    P = nc.NCS_PWORDS
    assert set(c.named["prefix"]) == set(nc.PREFIX_KINDS)
    st = nc.stretches(c.waves)
    by_lo = {int(r[1]): (int(r[0]), int(r[2])) for r in st}
    for kind, u in c.named["prefix"].items():
        i, hi = by_lo[u]                                             # the three named nodes ARE one stretch: a wave's whole quarter
        assert hi == u + 3 and c.waves[i][0] == 3
        wa, nw = nc.stretch_words(c.bit_off, u, hi)
        b0 = int(c.bit_off[u])
        has_long = c.node_len[u:hi].max() > 64
        assert has_long
        if kind == "under256":
            assert nw < 256
        elif kind == "two_pass":
            assert 257 <= nw <= 512
        elif kind == "three_pass":
            assert 512 < nw <= P
        elif kind.startswith("fit"):
            assert nw == P and (b0 >> 5) & 3 == int(kind[-1])
        elif kind.startswith("nofit"):
            assert nw == P + 1 and (b0 >> 5) & 3 == int(kind[-1])
        elif kind == "single":
            assert (int(c.bit_off[u + 1]) - 1 >> 5) - (b0 >> 5) + 1 > P and nw > P
        else:
            assert hi == len(c.node_len) and int(c.bit_off[hi]) == int(c.bit_off[-1]) and nw < 256
        # the first word also holds marked bits of the node in front (another wave's): they must cancel in the difference of two prefix entries
        assert b0 % 32 != 0 and w.covered[b0 - b0 % 32:b0].any() and c.waves[i][3] == u
        assert all(0 < w.cov[v] for v in range(u, hi))
        if kind in ("two_pass", "three_pass"):                       # nodes whose first and last word lie in different passes of 256 words, bits set in the earlier pass
            passes = set()
            for v in range(u, hi):
                p0, p1 = ((int(c.bit_off[v]) >> 5) - wa) // 256, ((int(c.bit_off[v + 1]) - 1 >> 5) - wa) // 256
                if p0 != p1 and w.covered[wa * 32:(wa + 256 * p1) * 32].any() and w.cov[v] < c.node_len[v]:
                    passes.add(p1)
            assert passes == ({1} if kind == "two_pass" else {1, 2}), (kind, passes)
    # ... and stretches of P without a node over 64 bases: the per-lane loop inside the long-node variant
    mine = [r for r in st if c.waves[r[0]][0] == 3]
    assert sum(1 for r in mine if c.node_len[r[1]:r[2]].max() <= 64) > 500
    # the stage call counts the same marks in stretches of 64 ALIGNED nodes: what popcount_long_kernel reaches of its three kinds
    kinds = set()
    V = len(c.node_len)
    for lo in range(0, V, 64):
        hi = min(V, lo + 64)
        wa, nw = nc.stretch_words(c.bit_off, lo, hi)
        kinds.add("over" if nw > nc.PCL_WORDS else "coop" if c.node_len[lo:hi].max() > 64 else "short")
    assert kinds == {"over", "coop", "short"}


def test_rounds_class(rounds):
    w, c = rounds, rounds.c
    nR = c.n_nodes[0]
    geo = nc.geometry(c.n_nodes)
    assert geo[0] == (256, 1055)
    wv = c.waves
    big = wv[wv[:, 0] == 0]
    n_rounds = -(-(big[:, 4] - big[:, 3]) // nc.ROUND)
    assert (n_rounds[big[:, 1] < 255] == 2).all() and len(big) == 1024               # every wave but those of the last workgroup takes a second round
    part = (w.cov > 0) & (w.cov < c.node_len)
    print("rounds: %d nodes covered in part, %d whole" % (part.sum(), (w.cov == c.node_len).sum()))
    assert part[:nR].sum() >= 40000
    # the crafted round borders
    assert len(c.borders) >= 200
    starts = {int(r[3]) + nc.ROUND for r in big if r[4] - r[3] > nc.ROUND}
    kinds = {}
    for i, (vb, res, kind) in enumerate(c.borders):
        x = int(c.bit_off[vb])
        assert vb in starts and x % 32 == res
        m = i % 3
        assert bool(w.covered[x - 1]) == (m != 1) and bool(w.covered[x]) == (m != 0)
        assert 0 < w.cov[vb - 1] < c.node_len[vb - 1]
        kinds.setdefault(kind, set()).add(m)
    assert set(kinds) == {"boundary", "inside", "one_word_inside", "one_word_whole", "one_word_from_boundary", "two_words_whole"} and all(v == {0, 1, 2} for v in kinds.values())
    # what the cleaning variant meets at the ends of a round [round_b0, run): s_part / e_part both ways, rounds inside one word
    seen = set()
    for i, j, v0, v1 in nc.rounds_of(big):
        b0, b1 = int(c.bit_off[v0]), int(c.bit_off[v1])
        seen.add((j, b0 % 32 != 0, b1 % 32 != 0, b0 >> 5 == (b1 - 1) >> 5))
    for j in (0, 1):
        assert {(j, s, e, False) for s in (False, True) for e in (False, True)} <= seen, j
    assert {(1, True, True, True), (1, False, True, True), (1, False, False, True)} <= seen          # ws == we
    # flag words wholly inside one stretch of lanes (the plain store) and flag words cut by a round border with flags on both sides
    flagged = np.zeros(len(c.node_len), dtype=bool)
    rd = c.reads
    so = rd.step_off.astype(np.int64)
    one = np.nonzero(np.diff(so) == 1)[0]
    v1 = rd.node_id[so[one]].astype(np.int64) - 1
    whole = (rd.pstart[one] == 0) & (rd.pend[one] == c.node_len[v1])
    flagged[v1[whole]] = True
    inside = 0
    for i, lo, hi in nc.stretches(big):
        for word in range((lo + 31) >> 5, hi >> 5):
            inside += bool(word * 32 - lo <= 32 and flagged[word * 32:word * 32 + 32].any())
    cut = sum(1 for vb, res, kind in c.borders if vb % 32 and flagged[vb - vb % 32:vb].any() and flagged[vb:vb - vb % 32 + 32].any())
    print("rounds: %d flag words inside one run of lanes, %d cut by a crafted round border with flags on both sides" % (inside, cut))
    assert inside >= 1000 and cut >= 50
    assert (w.cov[flagged] == c.node_len[flagged]).all()


@pytest.mark.parametrize("which", ["edges", "rounds"])
def test_every_species_keeps_lp_columns(which, request):
    """at the fraction of hit unique-trio windows the GPU cases ask for (FR of tests/test_gpu_node_count.py), every haplotype of every species is an LP
    column of the oracle's strain level: path_cov_ratio exists for sums over whole species and over paths that leave nodes out"""
    from oracle import oracle as orc
    w = request.getfixturevalue(which)
    ref = _equals_oracle(w, w.sp)
    for g, (T, b, cv, tb, na) in zip(w.c.species, ref):
        rc, met, n_cand, o1, o2 = orc.optimize_species(orc.Graph(g.node_len, g.path_off, g.path_nodes), T, b, cv, tb, fr=0.005)
        assert rc == 0 and n_cand == g.n_paths and all(met[k].has & 4 for k in range(g.n_paths)), g.name
