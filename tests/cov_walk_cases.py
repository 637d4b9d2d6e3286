"""Crafted walks for the short-read coverage kernel (coverage_fast_kernel, its read layout build_step_read and the two popcount kernels): a db of
three species and reads of at most 64 steps -- but for a few controls -- grouped in named classes, each there for one branch of the kernel that random
150-bp reads do not reach (tests/test_gpu_cov_walk_edges.py names the line per class).  numpy only, seeded, no GPU, no oracle.

build() -> (species: list of synthdata.SpeciesGraph, reads: synthdata.PackedReads, classes: dict name -> indices of its reads in `reads`); named() ->
the named nodes.  Ids are global (1-based, as in a GAF); a walk is any sequence of ids of one species: neither the reference nor the kernels
ask for an edge between two steps.
"""
import numpy as np

BLOCK = 2048                      # ids per node block of the read layout (COV_BLK_SHIFT = 11)
A_START, A_N = 1001, 6001         # ids 1001 .. 7001: blocks 0 .. 3
B_START, B_N = 7002, 3000         # ids 7002 .. 10001: the A|B border inside block 3 (6144 .. 8191)
C_START, C_N = 10002, 2500        # ids 10002 .. 12501: the B|C border inside block 4 (8192 .. 10239)
GIANT_70K, GIANT_300K = 300, 700  # local nodes of B: 70 000 bases (> the 65 536-bit LDS window), 300 000 bases (>= 2^18)
CROWD_BLOCK = 2                   # ids 4096 .. 6143 of A: the crowd's block, which no other class starts a read in
HUBS = (300, 1021, 1800, 2285)    # local nodes of C at which seven paths diverge (ids 10302, 11023, 11802, 12287: the last one is the last id of block 5)
N_DIV = 7                         # paths 0 .. 6 of C take their own way around every hub
N20 = 2900                        # a local node of A of 20 bases
XYX = 600                         # path 6 of C walks XYX, XYX + 1, XYX, XYX + 1: the x,y,x windows
REV = 2400                        # path 7 of C walks REV + 30 down to REV, leaving out REV + 15
WORD_B = 440                      # local node of B that pads the bits in front of B's word-edge nodes (WORD_B + 1 ..) to a word border
# lengths of the first nodes of A (from bit 0 of the bit vector) and of the nodes behind B's node WORD_B:
# 31 | 1 at bit 31 | 1 at bit 32 | 31 to a word's end | 32 = one word | 40 from a border: two words | 24 to a border | 33: two words | 31 | 40 | 22 | 40 from bit 30: three words
WORD_LENS = (31, 1, 1, 31, 32, 40, 24, 33, 31, 40, 22, 40)


def _graphs(rng):
    import synthdata as synth
    la = rng.integers(1, 41, size=A_N).astype(np.int64)
    la[:len(WORD_LENS)] = WORD_LENS
    la[N20] = 20
    lb = rng.integers(1, 41, size=B_N).astype(np.int64)
    lb[WORD_B + 1:WORD_B + 1 + len(WORD_LENS)] = WORD_LENS
    lb[WORD_B + 13] = 200                                            # ... in a stretch of 64 nodes that holds a node over 64 bases
    lb[GIANT_70K], lb[GIANT_300K] = 70000, 300000
    mids = 1500 + 97 * np.arange(12)                                 # a dozen nodes of 65 .. 1024 bases
    lb[mids] = (65, 66, 127, 128, 129, 255, 256, 500, 777, 1000, 1023, 1024)
    lb[2700:2900] = rng.integers(1, 65, size=200)                    # 64 + consecutive nodes of at most 64 bases (whole stretches of them)
    lb[WORD_B] = 32 - (int(la.sum()) + int(lb[:WORD_B].sum())) % 32  # B's node WORD_B + 1 begins a word of the bit vector
    lc = rng.integers(1, 41, size=C_N).astype(np.int64)

    def two_paths(n):                                                # the backbone, and the backbone without every tenth node
        p0 = np.arange(n)
        return [p0, p0[p0 % 10 != 5]]

    def c_path(i):                                                   # backbone that reaches hub m from m - 1 - i and leaves it to m + 1 + i
        keep = np.ones(C_N, dtype=bool)
        for m in HUBS:
            keep[m - i:m] = False
            keep[m + 1:m + 1 + i] = False
        return np.arange(C_N)[keep]
    cp = [c_path(i) for i in range(N_DIV)]
    at = int(np.nonzero(cp[6] == XYX + 1)[0][0])
    cp[6] = np.concatenate([cp[6][:at + 1], [XYX, XYX + 1], cp[6][at + 1:]])
    cp.append(np.array([REV + d for d in range(30, -1, -1) if d != 15]))

    def graph(name, lens, paths, start):
        off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.uint64)
        gl = np.array([int(lens[p].sum()) for p in paths], dtype=np.int64)
        return synth.SpeciesGraph(name, lens, off, np.concatenate(paths).astype(np.uint32), ["%s_h%02d" % (name, h) for h in range(len(paths))],
                                  start, start + len(lens) - 1, gl, np.ones(len(paths)))
    return [graph("A", la, two_paths(A_N), A_START), graph("B", lb, two_paths(B_N), B_START), graph("C", lc, cp, C_START)]


class _Reads:
    def __init__(self):
        self.walks, self.ps, self.pe, self.cls = [], [], [], {}

    def add(self, cls, walk, ps, pe):
        self.cls.setdefault(cls, []).append(len(self.walks))
        self.walks.append(np.asarray(walk, dtype=np.int64))
        self.ps.append(int(ps))
        self.pe.append(int(pe))


def build(seed=20261019):
    import synthdata as synth
    rng = np.random.default_rng(seed)
    species = _graphs(rng)
    A, B, C = species
    R = _Reads()
    lens = np.zeros(C.range_end + 2, dtype=np.int64)                 # node length by global id
    for g in species:
        lens[g.range_start:g.range_end + 1] = g.node_len

    def total(walk):
        return int(lens[np.asarray(walk)].sum())

    def exact(cls, walk, ps=None):                                   # pend - pstart = the walk's bases from pstart
        ps = int(rng.integers(0, lens[walk[0]])) if ps is None else ps
        R.add(cls, walk, ps, total(walk))

    # ---- len_edges: 1 .. 64 steps, up and down, from the first / last id of a block and from inside one, in every species
    starts = {"A": (2048, 4095, 3000), "B": (8192, 8191, 9000), "C": (12288, 10239, 11000)}
    for g in species:
        for s in starts[g.name]:
            for k in (1, 2, 3, 31, 32, 33, 63, 64):
                exact("len_edges", s + np.arange(k))
                exact("len_edges", s - np.arange(k))
    # ---- revisit: the first-occurrence codes (STEP_DIST) and read_nodes_len of a node whose first occurrence is step 0 (at_step0)
    for g, s in ((A, 2500), (B, 9100), (C, 10500), (A, 2047), (C, 12287)):
        for k in (3, 4, 33, 63, 64):
            up = s + np.arange(k - 1) if s + k < g.range_end else s - np.arange(k - 1)
            for ps in (0, 1):                                        # pstart > 0: len0 - ps is not the node's length
                if lens[s] < 2 and ps:
                    continue
                exact("revisit", np.concatenate([up, [up[0]]]), ps)  # the last step is step 0 again: distance k - 1
                exact("revisit", np.concatenate([up, [up[1]]]), ps)  # ... step 1 again
        for ps in (0, 1):
            if lens[s] < 2 and ps:
                continue
            exact("revisit", [s, s], ps)
            exact("revisit", [s, s, s], ps)
            exact("revisit", np.tile([s, s - 1], 32), ps)            # a,b,a,b ... to 64 steps
            exact("revisit", [s - 2, s - 1, s - 3, s - 1, s - 4, s - 1, s - 5], ps)   # a node three times, first at step 1
            R.add("revisit", [s - 2, s - 1, s - 3, s - 1, s - 4, s - 1], ps, total([s - 2, s - 1, s - 3]) + 1)   # ... and as the last step, target inside it
    # ---- offsets: profile.rs:821-859
    for g, s in ((A, 3500), (B, 9500), (C, 11500), (B, 8190)):
        w = s + np.arange(5)
        l0, tot, seen = int(lens[s]), total(w), total(w[:4])
        R.add("offsets", w, l0, tot)                                 # pstart == len(first): nothing of the first node
        R.add("offsets_abort", w, l0 + 1, tot)                       # the assert: the read is an abort
        R.add("offsets_abort", w[:2], l0 + 1, tot)
        R.add("offsets", w, 3 if l0 > 3 else 0, 1)                   # pend < pstart (or a tiny target)
        R.add("offsets", w, l0, 0)
        for ps in (0, l0 // 2):
            seen_ps = seen - ps                                      # aligned before the last step
            R.add("offsets", w, ps, ps + max(seen_ps - 1, 0))        # target < seen
            R.add("offsets", w, ps, ps + seen_ps)                    # == seen
            R.add("offsets", w, ps, ps + seen_ps + 1)                # seen + 1
            R.add("offsets", w, ps, ps + tot + 1000)                 # beyond the walk
        ln = l0
        one = [s]
        R.add("offsets", one, ln // 3, ln // 3 + max(ln // 3, 1) if ln > 2 else ln)    # inside the node
        R.add("offsets", one, ln // 2, ln // 2)                      # pend == pstart
        R.add("offsets", one, ln, 0)                                 # pend < pstart
        R.add("offsets", one, 0, ln)                                 # pend == len
        R.add("offsets", one, 0, ln + 1)                             # pend == len + 1: bases, no bits
    n20 = A_START + N20                                              # a 20-base node of A
    for span in ((1 << 18) - 1, 1 << 18, 400000):                    # a one-node read adds its target unclipped (profile.rs:828)
        R.add("two18", [n20], 0, span)
        R.add("two18", [n20], 7, 7 + span)
    g300, g70 = B_START + GIANT_300K, B_START + GIANT_70K
    R.add("two18", [g300], 0, 300000)                                # whole: a flag
    R.add("two18", [g300], 5, 299999)                                # bits, inside and outside the LDS bit window
    R.add("two18", [g300], 0, 300001)
    R.add("two18", [g300 - 1, g300, g300 + 1], 0, total([g300 - 1, g300, g300 + 1]))   # an interior step of 300 000 bases
    R.add("two18", [g300, g300 + 1], 11, 300000)                     # a first step of 299 989
    R.add("giant", [g70], 0, 70000)
    R.add("giant", [g70], 65, 69999)
    R.add("giant", [g70], 30000, 40000)
    R.add("giant", [g70 - 1, g70], 0, int(lens[g70 - 1]) + 66000)    # a last step that ends inside the node
    R.add("giant", [g70 + 2, g70 + 1, g70, g70 - 1], 0, total([g70 + 2, g70 + 1, g70, g70 - 1]))
    # ---- words: the named nodes at the word edges of the bit vector (A: per-lane counts; B: the cooperative prefix), as one-node reads
    for base in (A_START, B_START + WORD_B + 1):
        flip = base != A_START
        for j, ln in enumerate(WORD_LENS):
            nid = base + j
            if ln == 1:
                if (j == 1) == flip:
                    R.add("words", [nid], 0, 1)                      # A: bit 32 covered, bit 31 not; B: the other way round
                continue
            if j % 3 == 0:                                           # whole only as the union of two partial marks
                R.add("words", [nid], 0, ln // 2)
                R.add("words", [nid], ln // 2, ln)
            elif j % 3 == 1:                                         # all but the first base / all but the last
                R.add("words", [nid], 1, ln)
                if j != 4:
                    R.add("words", [nid], 0, ln - 1)
            else:                                                    # whole by a flag and also by bits
                R.add("words", [nid], 0, ln)
                R.add("words", [nid], 1, ln - 1)
    for m in B_START + 1500 + 97 * np.arange(12):                    # the nodes of 65 .. 1024 bases and their neighbours: partial marks in cooperative stretches
        ln = int(lens[m])
        R.add("words", [m], 1, ln - 1)
        R.add("words", [m - 1, m, m + 1], 0, total([m - 1, m]) + 1)
        if ln % 2:
            R.add("words", [m], 0, ln)
    # ---- far: out of a block to nodes 4096 + ids ahead of its start and 200 + behind it, and back (block 1 of A; C and B are too small for 4096: in C
    # 2100 ahead, beyond the windows of 2048 nodes only)
    for g, s, ahead, behind in ((A, 2600, 2048 + 4096 + 300, 2048 - 300), (A, 2048, 6960, 1100), (C, 10300, 10240 + 2100, 10240 - 205)):
        for ps in (0, 1):
            exact("far", [s, ahead, s + 1], ps)                      # the far node whole, as an interior step
            exact("far", [s, s + 1, behind, s + 2], ps)
            R.add("far", [s, s + 1, ahead + 1], ps, total([s, s + 1]) + max(int(lens[ahead + 1]) // 2, 1))    # partly, as the last step
            R.add("far", [s + 3, behind - 1], ps, total([s + 3]) + max(int(lens[behind - 1]) // 2, 1))
            exact("far", [s, ahead, behind, ahead, s], ps)
            exact("far", np.concatenate([[s], ahead + np.arange(30), [s + 1], behind - np.arange(30), [s]]), ps)
    # ... and B, from block 4 back to nodes of block 3 below the window, the two giants among them: 300 000 bases as an interior step (a flag and
    # `bases` on the global path), the 70 000-base node partly, as a last step
    s, behind = 8300, 8192 - 200
    for ps in (0, 1):
        exact("far", [s, behind, s + 1], ps)
        exact("far", [s, s + 1, g300, s + 2], ps)
        R.add("far", [s + 3, g70], ps, total([s + 3]) + 33333)
        R.add("far", [s + 4, behind - 1], ps, total([s + 4]) + max(int(lens[behind - 1]) // 2, 1))
        exact("far", np.concatenate([[s], behind - np.arange(30), [s]]), ps)
    # ---- border: reads of both species that start in the block of a species border
    for lo_g, hi_g in ((A, B), (B, C)):
        e, b = lo_g.range_end, hi_g.range_start
        for k in (1, 2, 5, 17, 40, 64):
            exact("border", e - np.arange(k))                        # from the last id of the lower species down
            exact("border", e - k + 1 + np.arange(k))                # ... up to it
            exact("border", b + np.arange(k))
            exact("border", b + k - 1 - np.arange(k))
            exact("border", e - 3 * k - np.arange(k) % 3)
            exact("border", b + 3 * k + np.arange(k) % 3)
    # ---- heads: the rows filed under a hub of C, each searched from both sides; 64-step walks fill a 64-step group, so step i is lane i
    for m in HUBS:
        mid = C_START + m
        for i in range(N_DIV):
            a, c = mid - 1 - i, mid + 1 + i
            exact("heads", [a, mid, c])
            exact("heads", [c, mid, a])
            exact("heads", [a - 1, a, mid, c, c + 1])
            for j in range(N_DIV):
                a2, c2 = mid - 1 - j, mid + 1 + j
                bounce = np.tile([c + 1, c], 29)                     # 58 steps between the two windows
                exact("heads64", np.concatenate([[a, mid, c], bounce, [c2, mid, a2]]))          # probed from lanes 2 and 63
                if j == (i + 3) % N_DIV:
                    exact("heads64", np.concatenate([[a - 1, a, mid, c], bounce[:56], [c2, mid, a2, a2 - 1]]))   # ... lanes 3 and 62
    x = C_START + XYX
    for w in ([x, x + 1, x], [x + 1, x, x + 1], [x - 1, x, x + 1, x, x + 1, x + 2], [x + 2, x + 1, x, x + 1, x, x - 1]):
        exact("heads", w)                                            # a == c: both ends of the row are one node
    r = C_START + REV
    for w in ([r + 13, r + 14, r + 16, r + 17], [r + 17, r + 16, r + 14, r + 13], r + np.arange(12, 20), r + np.arange(19, 11, -1)):
        exact("heads", w)                                            # rows of the path that runs down, read up and down
    # ---- crowd: one block of A with more than COV_ITEM_GROUPS groups of steps; starts ascend with the read's number
    lo = CROWD_BLOCK * BLOCK
    for j in range(700):
        s = lo + j * BLOCK // 700
        k = int(rng.integers(10, 21))
        exact("crowd", s + np.cumsum(rng.integers(0, 3, size=k)))
    # ---- fill: random walks of 1 .. 64 steps of +-2 ids, the four offset modes of test_long_walks_with_revisits
    n_fill = 0
    while n_fill < 2000:
        g = species[int(rng.integers(0, 3))]
        s = int(rng.integers(g.range_start + 70, g.range_end - 70))
        if s // BLOCK == CROWD_BLOCK or (g is B and min(abs(s - g300), abs(s - g70), abs(s - B_START - WORD_B - 6)) < 140):
            continue                                                 # (the giants and B's word-edge nodes are walked by their own classes alone)
        k = int(rng.integers(1, 65))
        walk = np.clip(s + np.cumsum(np.concatenate([[0], rng.integers(-2, 3, size=k - 1)])), g.range_start, g.range_end)
        tot = total(walk)
        a = int(rng.integers(0, lens[walk[0]] + 1))
        b = a + [tot - a - int(rng.integers(0, lens[walk[-1]] + 1)), int(rng.integers(0, 50)), tot + 77, tot // 2][n_fill % 4]
        R.add("fill", walk, a, max(b, 0))
        n_fill += 1
    for _ in range(5):
        R.add("empty", [], 0, 10)
    # ---- controls: three walks of 65 steps (the other kernel), two that leave their species (no species: "U")
    exact("control_long", 3100 + np.arange(65))
    exact("control_long", 9300 - np.arange(65))
    exact("control_long", np.concatenate([11200 + np.arange(64), [11200]]))
    exact("control_u", [A.range_end - 1, A.range_end, B.range_start])
    exact("control_u", [C.range_start + 1, C.range_start, B.range_end, B.range_end - 1])

    order = rng.permutation(len(R.walks))                            # file order: a seeded permutation
    where = np.empty(len(order), dtype=np.int64)
    where[order] = np.arange(len(order))
    walks = [R.walks[i] for i in order]
    n = len(walks)
    off = np.concatenate([[0], np.cumsum([len(w) for w in walks])]).astype(np.uint64)
    reads = synth.PackedReads(off, np.concatenate(walks).astype(np.uint32), np.zeros(int(off[-1]), np.uint8),
                              np.array(R.ps, dtype=np.int64)[order], np.array(R.pe, dtype=np.int64)[order], np.full(n, 150, np.int64),
                              np.full(n, 60, np.int64), np.zeros(n, np.int64))
    classes = {name: np.sort(where[np.array(idx)]) for name, idx in R.cls.items()}
    return species, reads, classes


def named():
    """the named nodes of build()'s graphs, as ids (word_v: as indices into the concatenated node arrays of the db)"""
    return {"n20": A_START + N20, "g300": B_START + GIANT_300K, "g70": B_START + GIANT_70K, "word_nodes": (A_START, B_START + WORD_B + 1),
            "word_v": (0, A_N + WORD_B + 1), "mids": B_START + 1500 + 97 * np.arange(12)}


ID_SHIFT = 16 * BLOCK             # shifted(): whole blocks, so every id keeps its place in its block


def shifted(species, reads, delta=ID_SHIFT):
    """the same db and reads with every id `delta` higher: nothing local to a species changes, so the reference's results are those of build()'s.
    From 32 768 ids on there are more than 2^10 buckets of 32 ids: the least cap the option group_bucket_bits can set then widens the buckets."""
    import dataclasses
    sp = [dataclasses.replace(g, range_start=g.range_start + delta, range_end=g.range_end + delta) for g in species]
    return sp, dataclasses.replace(reads, node_id=(reads.node_id.astype(np.int64) + delta).astype(np.uint32))
