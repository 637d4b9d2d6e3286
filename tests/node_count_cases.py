"""A corpus made for the covered-base counters of the resident step (node_cov_stats_kernel, stage_node_stats.hip; the stage call's popcount kernels see
the same marks): two dbs whose marks are placed with ONE-NODE reads -- a read [v] with (pstart, pend), pstart < pend <= len, marks the bits
[pstart, pend) of v, a read from 0 to len covers v by the whole-node flag -- so the bit pattern of every node is the test's own choice, beside a few
thousand ordinary walks of three to five steps along the paths (unique-trio rows, LP columns).  numpy only, seeded, no GPU, no oracle:
tests/test_node_count_cases.py shows on the CPU that every class holds what is said here and that model() equals the C oracle bit for bit.

The node pass cuts its work as node_stats_launch and the kernel do, mirrored by geometry() / waves() / stretches(): a species gets up to STAT_CHUNKS
workgroups, each cuts its range into four per-wave quarters, a wave walks its quarter in rounds of 64 * NCS_NR nodes, and a "stretch" is the (up to 64)
nodes of one wave in one quarter of a round.

build_edges(long_nodes) -> Corpus: four species A, B, C, P of about 12 500 nodes; every species gets 256 chunks, a wave's quarter is 3 to 5 nodes, so
nearly every word of the bit vector is shared by two waves.  Classes (named nodes are global 0-based node indices):
  word        (A) nodes of 1, 2, 31, 32, 33, 63, 64, 65 and 100 bases at each of the 32 bit alignments, each with one of six mark patterns
  neighbours  (B, C and the three species borders) two adjacent nodes that meet inside a word, one's last bit marked and the other's first bit not
  flags       (B, C) nodes whole by the flag in `full` words whose 32 nodes span several waves; some of them also carry bits
  prefix      (P, long_nodes only) stretches made for the LDS prefix of the long-node variant: see PREFIX_KINDS
  dropped     B is the species the tests give no genome length: its reads are there, the expectation leaves them out
build_rounds() -> Corpus: one species of 270 000 nodes of 1 to 8 bases with three paths and one small single-path species: every wave of the large one
takes a round of 256 nodes and a round of 8 (7 in a workgroup's last wave), with crafted marks and lengths at the round borders of every fourth workgroup.
"""
from types import SimpleNamespace

import numpy as np

STAT_CHUNKS = 256                 # lad_device.hpp: most workgroups of a species
NCS_NR = 4                        # stage_node_stats.hip: 64-node stretches per round
ROUND = 64 * NCS_NR
NCS_PWORDS = 2304                 # words of one stretch the LDS prefix holds
PCL_WORDS = 2304                  # ... of popcount_long_kernel (stage_cov.hip), whose stretches are 64 aligned nodes
WORD_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 100)
N_PATTERNS = 6                    # first bit | last bit | all but the first | all but the last | whole as the union of two marks | whole by the flag and by bits
EDGES_NODES = (4400, 2600, 2500, 3000)      # A, B, C, P
EDGES_DROPPED = 1
ROUNDS_NODES = (270000, 3000)
PREFIX_KINDS = ("under256", "two_pass", "three_pass", "fit0", "fit1", "fit2", "fit3", "nofit0", "nofit1", "nofit2", "nofit3", "single", "last")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the launch geometry of node_stats_launch / node_cov_stats_kernel, mirrored
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def geometry(n_nodes):
    """per species (chunks, nodes per chunk): target = max(1, V / 8192), k = min(256, max(1, floor(n / target + 0.5))), per = ceil(n / k)"""
    V = int(sum(n_nodes))
    target = max(1.0, V / 8192.0)
    out = []
    for n in n_nodes:
        k = int(min(float(STAT_CHUNKS), max(1.0, np.floor(n / target + 0.5))))
        out.append((k, -(-int(n) // k)))
    return out


def waves(n_nodes):
    """every wave that has nodes: rows (species, chunk, wave, wlo, whi), global node indices; quarter = ceil((hi - lo) / 4) of the chunk's own range"""
    rows, base = [], 0
    for s, (n, (k, per)) in enumerate(zip(n_nodes, geometry(n_nodes))):
        for ch in range(k):
            lo = base + ch * per
            hi = min(base + n, lo + per)
            if hi <= lo:
                continue
            q = (hi - lo + 3) // 4
            for w in range(4):
                wlo = min(hi, lo + w * q)
                whi = min(hi, wlo + q)
                if whi > wlo:
                    rows.append((s, ch, w, wlo, whi))
        base += int(n)
    return np.array(rows, dtype=np.int64)


def rounds_of(wv):
    """rows (wave row, round number, first node, end node) of every round of every wave"""
    out = []
    for i, (s, ch, w, wlo, whi) in enumerate(wv):
        for j, v0 in enumerate(range(int(wlo), int(whi), ROUND)):
            out.append((i, j, v0, min(int(whi), v0 + ROUND)))
    return np.array(out, dtype=np.int64)


def stretches(wv):
    """rows (wave row, first node, end node) of every stretch: the nodes v0 + 64 r .. of a round"""
    out = []
    for i, j, v0, v1 in rounds_of(wv):
        for lo in range(int(v0), int(v1), 64):
            out.append((i, lo, min(int(v1), lo + 64)))
    return np.array(out, dtype=np.int64)


def stretch_words(bit_off, lo, hi):
    """(wa, nw) of the long-node variant for the stretch [lo, hi): the words from the 16-byte boundary at or below its first bit to its last bit"""
    b0, b1 = int(bit_off[lo]), int(bit_off[hi])
    wa = (b0 >> 5) & ~3
    return wa, (((b1 - 1) >> 5) - wa + 1 if b1 > b0 else 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# lengths with crafted runs of nodes at chosen bit alignments
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class _Layout:
    """random lengths 1 .. fill_max; place(v, lens, residue, modulus, n_fill, cap) writes a run of lengths at node v and asks that v's first bit be
    `residue` modulo `modulus`: finish() gives the n_fill nodes in front of the run (1 .. cap bases each) the lengths that make it so"""

    def __init__(self, rng, V, fill_max):
        self.len = rng.integers(1, fill_max + 1, size=V).astype(np.int64)
        self.reserved = np.zeros(V, dtype=bool)
        self.items = []

    def place(self, v, lens, residue, modulus=32, n_fill=1, cap=32):
        lens = [int(x) for x in lens]
        assert v - n_fill >= 0 and not self.reserved[v - n_fill:v + len(lens)].any(), v
        self.reserved[v - n_fill:v + len(lens)] = True
        self.len[v:v + len(lens)] = lens
        self.items.append((int(v), int(residue) % modulus, modulus, n_fill, cap))

    def finish(self):
        pos, cum = 0, 0
        for v, residue, modulus, n_fill, cap in sorted(self.items):
            f0 = v - n_fill
            assert f0 >= pos
            cum += int(self.len[pos:f0].sum())
            s = (residue - cum) % modulus
            while s < n_fill:
                s += modulus
            assert s <= n_fill * cap, (v, s)
            fill = np.ones(n_fill, dtype=np.int64)
            rest = s - n_fill
            for i in range(n_fill):
                add = min(cap - 1, rest)
                fill[i] += add
                rest -= add
            self.len[f0:v] = fill
            cum += s
            pos = v
        return np.concatenate([[0], np.cumsum(self.len)]).astype(np.int64)


class _Reads:
    def __init__(self):
        self.walks, self.ps, self.pe, self.cls = [], [], [], {}

    def mark(self, cls, v, ps, pe):
        """a one-node read of the node with global index v (id v + 1); an empty interval is no read"""
        if ps < pe:
            self.add(cls, [v + 1], ps, pe)

    def add(self, cls, ids, ps, pe):
        self.cls.setdefault(cls, []).append(len(self.walks))
        self.walks.append(np.asarray(ids, dtype=np.int64))
        self.ps.append(int(ps))
        self.pe.append(int(pe))


def pattern_marks(L, p):
    """the intervals of mark pattern p on a node of L bases (empty ones are dropped by _Reads.mark)"""
    return ([(0, 1)], [(L - 1, L)], [(1, L)], [(0, L - 1)], [(0, L // 2), (L // 2, L)], [(0, L), (1, L - 1)])[p]


def _paths(n, n_paths):
    p0 = np.arange(n)
    return [p0, p0[p0 % 10 != 5], p0[p0 % 7 != 3]][:n_paths]


def _graphs(names, n_nodes, n_paths, node_len):
    import synthdata as synth
    out, base = [], 0
    for name, n, h in zip(names, n_nodes, n_paths):
        lens = node_len[base:base + n]
        paths = _paths(n, h)
        off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.uint64)
        gl = np.array([int(lens[p].sum()) for p in paths], dtype=np.int64)
        out.append(synth.SpeciesGraph(name, lens.copy(), off, np.concatenate(paths).astype(np.uint32), ["%s_h%02d" % (name, i) for i in range(h)],
                                      base + 1, base + n, gl, np.ones(h)))
        base += n
    return out


def _add_walks(rng, R, species, node_len, reserved, per_species):
    """ordinary walks of three to five steps along the paths, over nodes no class has named; they begin inside their first node and end inside their last"""
    for g, n_walks in zip(species, per_species):
        base, done, tries = g.range_start - 1, 0, 0
        while done < n_walks:
            tries += 1
            assert tries < 50 * n_walks + 1000
            h = int(rng.integers(0, g.n_paths))
            p0, p1 = int(g.path_off[h]), int(g.path_off[h + 1])
            k = int(rng.integers(3, 6))
            at = int(rng.integers(p0, p1 - k))
            w = g.path_nodes[at:at + k].astype(np.int64) + base
            if reserved[w].any():
                continue
            ln = node_len[w]
            ps = int(rng.integers(0, ln[0]))
            R.add("walks", w + 1, ps, int(ln.sum()) - int(rng.integers(0, ln[-1])))
            done += 1


def _finish(rng, R, species, classes_extra, **info):
    import synthdata as synth
    order = rng.permutation(len(R.walks))                            # file order: a seeded permutation
    where = np.empty(len(order), dtype=np.int64)
    where[order] = np.arange(len(order))
    walks = [R.walks[i] for i in order]
    n = len(walks)
    off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
    reads = synth.PackedReads(off, np.concatenate(walks).astype(np.uint32), np.zeros(int(off[-1]), np.uint8), np.array(R.ps, dtype=np.int64)[order],
                              np.array(R.pe, dtype=np.int64)[order], np.full(n, 150, np.int64), np.full(n, 60, np.int64), np.zeros(n, np.int64))
    classes = {name: np.sort(where[np.array(idx)]) for name, idx in R.cls.items()}
    node_len = np.concatenate([g.node_len for g in species])
    return SimpleNamespace(species=species, reads=reads, classes=classes, node_len=node_len,
                           bit_off=np.concatenate([[0], np.cumsum(node_len)]).astype(np.int64), n_nodes=tuple(g.n_nodes for g in species),
                           node_base=np.concatenate([[0], np.cumsum([g.n_nodes for g in species])]).astype(np.int64), **classes_extra, **info)


def avg_len(corpus, dropped=()):
    """the species lengths of a step; a species without one is dropped by the species level"""
    avg = np.array([g.genome_len.mean() for g in corpus.species], dtype=np.float64)
    avg[list(dropped)] = 0.0
    return avg


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def build_edges(long_nodes=False, seed=20261020):
    rng = np.random.default_rng(seed)
    n_nodes = EDGES_NODES
    base = np.concatenate([[0], np.cumsum(n_nodes)]).astype(np.int64)
    V = int(base[-1])
    wv = waves(n_nodes)
    lay = _Layout(rng, V, 8)
    R = _Reads()
    named = {"word": [], "neighbours": [], "flags": [], "flags_bits": [], "prefix": {}}
    # ---- word (A): filler, crafted node, filler, crafted node ...; the fillers carry marks that end on their last bit / begin on their first
    v = 1
    for L in WORD_LENS:
        for a in range(32):
            for p in range(N_PATTERNS):
                lay.place(v, [L], a)
                named["word"].append((v, L, a, p))
                for ps, pe in pattern_marks(L, p):
                    R.mark("word", v, ps, pe)
                v += 2
    word_end = v
    assert word_end + 600 < n_nodes[0]
    # ---- neighbours: pairs (u, u + 1) whose common border lies inside a word, over a wave border, a workgroup border, a species border
    def pair(u, a, which, kind):
        lu, lw = int(rng.integers(2, 9)), int(rng.integers(2, 9))
        lay.place(u, [lu, lw], (a - lu) % 32)
        named["neighbours"].append((u, a, which, kind))
        if which == 0:                                               # the last bit of u, and of u + 1 everything but its first
            R.mark("neighbours", u, lu - 1, lu)
            R.mark("neighbours", u + 1, 1, lw)
        else:                                                        # the first bit of u + 1, and of u everything but its last
            R.mark("neighbours", u, 0, lu - 1)
            R.mark("neighbours", u + 1, 0, 1)
    n_pair = 0
    for s in (1, 2):
        mine = wv[wv[:, 0] == s]
        inner = mine[(mine[:, 2] > 0) & (mine[:, 1] % 6 == 1)]        # a wave border inside a workgroup
        outer = mine[(mine[:, 2] == 0) & (mine[:, 1] % 6 == 4)]       # the first wave of a workgroup: a workgroup border in front of it
        for kind, rows in (("wave", inner[:45]), ("workgroup", outer[:40])):
            for row in rows:
                pair(int(row[3]) - 1, 1 + n_pair % 31, n_pair % 2, kind)
                n_pair += 1
    for s in (1, 2, 3):                                              # the last node of a species and the first node of the next
        pair(int(base[s]) - 1, (7, 19, 30)[s - 1], s % 2, "species")
    # ---- flags: whole `full` words of flagged nodes, scattered flagged nodes, flagged nodes that also carry bits (no alignment asked: no fillers)
    for s in (1, 2):
        lo, hi = int(base[s]), int(base[s + 1])
        free_words = [w for w in range((lo >> 5) + 1, hi >> 5) if not lay.reserved[w * 32:w * 32 + 32].any()]
        for j, w in enumerate(free_words[1::4][:12]):
            for u in range(w * 32, w * 32 + 32):
                if j % 3 == 2 and u % 5 == 0:
                    continue                                         # (every third such word keeps a few nodes unflagged)
                lay.reserved[u] = True
                L = int(lay.len[u])
                R.mark("flags", u, 0, L)
                named["flags"].append(u)
                if u % 4 == 1 and L > 2:
                    R.mark("flags", u, 1, L - 1)
                    named["flags_bits"].append(u)
    # ---- prefix (P, the long variant): stretches -- here a wave's whole quarter of three nodes -- of chosen word counts
    if long_nodes:
        mine = wv[wv[:, 0] == 3]
        spots = mine[(mine[:, 2] == 1) & (mine[:, 1] % 6 == 2)]       # the second wave of a workgroup: the node in front belongs to the first wave
        kinds = {"under256": (37, [100, 200, 50]), "two_pass": (70, [5000, 4000, 3000]), "three_pass": (101, [10000, 9000, 5000]),
                 "single": (9, [80000, 7, 9])}
        for rho in range(4):
            a = 5 + rho
            T = 32 * (NCS_PWORDS - rho) - a                          # from bit a of word 4 q + rho to the last bit of word 4 q + 2303
            kinds["fit%d" % rho] = (32 * rho + a, [30000, 25000, T - 55000])
            kinds["nofit%d" % rho] = (32 * rho + a, [30000, 25000, T - 55000 + 1])
        for (kind, (res, lens)), row in zip(kinds.items(), spots):
            assert row[4] - row[3] == 3
            lay.place(int(row[3]), lens, res, modulus=128, cap=128)
            named["prefix"][kind] = int(row[3])
        lay.place(V - 3, [300, 200, 100], 37, modulus=128, cap=128)  # the last stretch of the db: it ends on bit_off[V]
        named["prefix"]["last"] = V - 3
        for kind, u in named["prefix"].items():
            L0, L1, L2 = (int(x) for x in lay.len[u:u + 3])
            R.mark("prefix", u, 1, L0 - 1)
            if kind.startswith("nofit"):
                R.mark("prefix", u, 0, 1)
            R.mark("prefix", u + 1, L1 // 3, 2 * L1 // 3)
            R.mark("prefix", u + 1, 0, 1)
            R.mark("prefix", u + 2, L2 - 1, L2)
            R.mark("prefix", u + 2, L2 // 4, L2 // 2)
            if kind in ("under256", "fit2"):
                R.mark("prefix", u + 1, 0, L1)                       # ... and a long node whole by the flag
    bit_off = lay.finish()
    node_len = lay.len
    # ---- the fillers: marks that end on their last bit and marks that begin on their first (the neighbour's bits beside a crafted node's)
    is_item = np.zeros(V, dtype=bool)
    for u, L, a, p in named["word"]:
        is_item[u] = True
    for u, a, which, kind in named["neighbours"]:
        is_item[u:u + 2] = True
    for u in named["prefix"].values():
        is_item[u:u + 3] = True
    is_item[named["flags"]] = True
    for u in named["prefix"].values():                               # the node in front of a prefix stretch (another wave's) ends marked, in the stretch's first word
        R.mark("prefix", u - 1, max(int(node_len[u - 1]) - 3, 0), int(node_len[u - 1]))
    for u in np.nonzero(lay.reserved & ~is_item)[0]:
        L = int(node_len[u])
        if rng.random() < 0.6:
            R.mark("fillers", int(u), int(rng.integers(0, L)), L)
        if rng.random() < 0.4 and L > 1:
            R.mark("fillers", int(u), 0, int(rng.integers(1, L)))
    # ---- everything else: a random proper sub-interval on two fifths of the nodes, a flag on a twentieth
    free = np.nonzero(~lay.reserved)[0]
    for u in free[rng.random(len(free)) < 0.4]:
        L = int(node_len[u])
        if L >= 2:
            a = int(rng.integers(0, L - 1))
            R.mark("partial", int(u), a, int(rng.integers(a + 1, L + (a > 0))))
    for u in free[rng.random(len(free)) < 0.05]:
        R.mark("whole", int(u), 0, int(node_len[u]))
    species = _graphs("ABCP", n_nodes, (2, 2, 1, 1), node_len)
    _add_walks(rng, R, species, node_len, lay.reserved, (500, 900, 900, 900))
    return _finish(rng, R, species, {"named": named}, waves=wv, word_end=word_end, long_nodes=long_nodes, dropped=EDGES_DROPPED)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# rounds
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def build_rounds(seed=20261021):
    rng = np.random.default_rng(seed)
    n_nodes = ROUNDS_NODES
    V = int(sum(n_nodes))
    wv = waves(n_nodes)
    lay = _Layout(rng, V, 8)
    R = _Reads()
    borders = []                                                     # (first node of round two, residue asked of its first bit, kind)
    two = wv[(wv[:, 0] == 0) & (wv[:, 4] - wv[:, 3] > ROUND) & (wv[:, 1] % 4 == 0)]
    for i, row in enumerate(two):
        vb = int(row[3]) + ROUND
        n2 = int(row[4]) - vb                                        # nodes of round two: 8, and 7 in a workgroup's last wave
        assert n2 in (7, 8)
        kind = ("boundary", "inside", "one_word_inside", "one_word_whole", "one_word_from_boundary", "two_words_whole")[(i // 3) % 6]
        res = {"boundary": 0, "inside": 1 + (7 * i) % 31, "one_word_inside": 4, "one_word_whole": 0, "one_word_from_boundary": 0, "two_words_whole": 0}[kind]
        second = {"boundary": [6, 3, 5, 2, 8, 4, 7, 3], "inside": [6, 3, 5, 2, 8, 4, 7, 3], "one_word_inside": [2] * 8, "one_word_whole": [4] * 8,
                  "one_word_from_boundary": [2] * 8, "two_words_whole": [8] * 8}[kind][:n2]
        if kind == "one_word_whole":
            second[-1] = 32 - 4 * (n2 - 1)                           # ... exactly the 32 bits of one word
        lay.place(vb - 1, [5] + second, (res - 5) % 32, n_fill=8, cap=8)
        borders.append((vb, res, kind))
        m = i % 3                                                    # the last bit of round one | the first bit of round two | both
        if m != 1:
            R.mark("border", vb - 1, 4, 5)
        else:
            R.mark("border", vb - 1, 0, 4)
        if m != 0:
            R.mark("border", vb, 0, 1)
        else:
            R.mark("border", vb, 1, second[0])
        for j in range(1, n2):                                       # the rest of round two: a proper part of every node, the last node to its last bit
            R.mark("border", vb + j, 1 if j < n2 - 1 else 0, second[j] if j % 2 or j == n2 - 1 else second[j] - 1)
        if i % 2 == 0:                                               # a flag word cut by the round border, flags on both sides (a filler and a node of round two)
            R.mark("border_flags", vb - 2, 0, 8)
            R.mark("border_flags", vb + 2, 0, second[2])
    bit_off = lay.finish()
    node_len = lay.len
    for vb, res, kind in borders[::2]:
        assert node_len[vb - 2] <= 8
    # the flag reads of the fillers were written before finish() chose their lengths: whole means 0 .. len
    for k in R.cls.get("border_flags", []):
        u = int(R.walks[k][0]) - 1
        R.pe[k] = int(node_len[u])
    free = np.nonzero(~lay.reserved)[0]
    pick = rng.random(len(free))
    for u in free[pick < 0.2]:                                       # a proper sub-interval on a fifth of the nodes
        L = int(node_len[u])
        if L >= 2:
            a = int(rng.integers(0, L - 1))
            R.mark("partial", int(u), a, int(rng.integers(a + 1, L + (a > 0))))
    for u in free[(pick >= 0.2) & (pick < 0.28)]:                    # whole by the flag
        R.mark("whole", int(u), 0, int(node_len[u]))
    for u in free[(pick >= 0.28) & (pick < 0.29)]:                   # ... and by bits as well
        L = int(node_len[u])
        R.mark("whole", int(u), 0, L)
        R.mark("whole", int(u), 0, max(L - 1, 1))
    species = _graphs(("R", "S"), n_nodes, (3, 1), node_len)
    _add_walks(rng, R, species, node_len, lay.reserved, (3000, 800))
    return _finish(rng, R, species, {"borders": borders}, waves=wv, dropped=None, long_nodes=False)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the expectation in numpy
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def model(corpus, sp, keep=None):
    """(bases [V] int64, cov [V] int64, covered [L] bool) of the reads whose species sp[r] >= 0 (and keep[r]): the union of the marked intervals per node.
    One-node reads: bases += pend - pstart when that is >= 0, bits [pstart, pend) when pstart < pend <= len.  Walks (no node twice, pstart <= len of
    the first node): the first node from pstart, the nodes between whole, the last one max(pend - pstart - seen, 0) bases from its first, cut at its length."""
    rd, node_len, bit_off = corpus.reads, corpus.node_len, corpus.bit_off
    V, L = len(node_len), int(bit_off[-1])
    so = rd.step_off.astype(np.int64)
    k = np.diff(so)
    live = (sp >= 0) if keep is None else (sp >= 0) & keep
    bases = np.zeros(V, dtype=np.int64)
    diff = np.zeros(L + 1, dtype=np.int64)

    def put(v, a, b):                                                # intervals [a, b) of the nodes v, a < b <= len
        np.add.at(diff, bit_off[v] + a, 1)
        np.add.at(diff, bit_off[v] + b, -1)
    one = np.nonzero(live & (k == 1))[0]
    v1 = rd.node_id[so[one]].astype(np.int64) - 1
    a1, b1 = rd.pstart[one], rd.pend[one]
    ok = b1 >= a1
    np.add.at(bases, v1[ok], (b1 - a1)[ok])
    bits = (a1 < b1) & (b1 <= node_len[v1])
    put(v1[bits], a1[bits], b1[bits])
    for r in np.nonzero(live & (k > 1))[0]:
        w = rd.node_id[so[r]:so[r + 1]].astype(np.int64) - 1
        ln = node_len[w]
        assert len(set(w.tolist())) == len(w) and rd.pstart[r] <= ln[0]
        aln = ln.copy()
        aln[0] = ln[0] - rd.pstart[r]
        seen = int(aln[:-1].sum())
        aln[-1] = max(int(rd.pend[r] - rd.pstart[r]), seen) - seen
        np.add.at(bases, w, aln)
        a = np.zeros(len(w), dtype=np.int64)
        a[0] = rd.pstart[r]
        b = np.minimum(a + aln, ln)
        put(w[a < b], a[a < b], b[a < b])
    covered = np.cumsum(diff[:-1]) > 0
    cc = np.concatenate([[0], np.cumsum(covered)])
    return bases, (cc[bit_off[1:]] - cc[bit_off[:-1]]).astype(np.int64), covered


def step_species(corpus, sp, dropped=()):
    """the species of every read as a step sees it: the reads of a dropped species count for nothing"""
    out = sp.copy()
    for s in dropped:
        out[sp == s] = -1
    return out
