"""The mosaic read contract (DESIGN.md "Mosaic reads", include/pantax_hip.h) read row by row: plain Python sets, no numpy in the decisions.  The
yardstick of tests/test_gpu_mosaic.py, itself pinned on hand-written cases in tests/test_mosaic_ref.py.  Its `reads` are those of
tests/read_support_ref.read_support: they carry the nodes of every walk in walk order."""
import numpy as np

COUNTED, COMPATIBLE, MOSAIC1, MOSAIC2, MOSAIC3PLUS, FOREIGN = range(6)
N_SEGMENTS, N_BREAKS, FOREIGN_STEPS = range(3)


def class_of(k):
    return COMPATIBLE if k == 1 else MOSAIC1 if k == 2 else MOSAIC2 if k == 3 else MOSAIC3PLUS


def cut(member):
    """member = per step the set M(v) of candidates that walk it, none empty -> the segments [(first step, one past the last, A_j)] of the greedy cut
    from the left: a segment grows while the intersection stays non-empty, the step that would empty it opens the next one"""
    segs, first, run = [], 0, set(member[0])
    for i in range(1, len(member)):
        if run & member[i]:
            run = run & member[i]
        else:
            segs.append((first, i, run))
            first, run = i, set(member[i])
    segs.append((first, len(member), run))
    return segs


def assigned(A, cand_hap, cand_w):
    """argmax of the weight over A (candidate entries), ties to the smallest haplotype index"""
    wmax = max(float(cand_w[c]) for c in A)
    return min((c for c in A if float(cand_w[c]) == wmax), key=lambda c: int(cand_hap[c]))


def mosaic(hap_nodes, reads, cand_off, cand_hap, cand_w):
    """hap_nodes[s][h] = the set of nodes the walk of haplotype h of species s visits.
    reads = iterable of (species or -1, counted, nodes of the walk in walk order (repeats allowed), pstart, pend).
    -> species [S][6][3], extra [S][3], hap [C][2], pair_off [S+1], pair [pair_off[S]] as uint64, junction [J][3] uint32 = the distinct
    (species, node_a, node_b) in ascending order, junction_count [J] uint64, n_breaks_total"""
    S = len(hap_nodes)
    C = int(cand_off[S])
    species = [[[0, 0, 0] for _ in range(6)] for _ in range(S)]
    extra = [[0, 0, 0] for _ in range(S)]
    hap = [[0, 0] for _ in range(C)]
    pair_off = [0]
    for s in range(S):
        K = int(cand_off[s + 1]) - int(cand_off[s])
        pair_off.append(pair_off[-1] + (K * K if K <= 64 else 0))
    pair = [0] * pair_off[S]
    junction = {}

    def add(dst, q):
        for i in range(3):
            dst[i] += q[i]

    for sp, counted, nodes, pstart, pend in reads:
        if sp < 0 or not counted:
            continue
        s = int(sp)
        q = (1, len(nodes), int(pend) - int(pstart) if int(pend) >= int(pstart) else 0)
        add(species[s][COUNTED], q)
        c0, c1 = int(cand_off[s]), int(cand_off[s + 1])
        K = c1 - c0
        if K == 0 or K > 64:
            continue
        member = [set(c for c in range(c0, c1) if int(v) in hap_nodes[s][int(cand_hap[c])]) for v in nodes]
        empty = sum(1 for m in member if not m)
        if empty:
            add(species[s][FOREIGN], q)
            extra[s][FOREIGN_STEPS] += empty
            continue
        segs = cut(member)
        k = len(segs)
        add(species[s][class_of(k)], q)
        if k < 2:
            continue
        extra[s][N_SEGMENTS] += k
        extra[s][N_BREAKS] += k - 1
        who = [assigned(A, cand_hap, cand_w) for _, _, A in segs]
        for (a, b, _), c in zip(segs, who):
            hap[c][0] += 1
            hap[c][1] += b - a
        for j in range(k - 1):
            pair[pair_off[s] + (who[j] - c0) * K + (who[j + 1] - c0)] += 1
            key = (s, int(nodes[segs[j][1] - 1]), int(nodes[segs[j + 1][0]]))
            junction[key] = junction.get(key, 0) + 1
    keys = sorted(junction)
    u = lambda x, shape: np.array(x, dtype=np.uint64).reshape(shape)
    return (u(species, (S, 6, 3)), u(extra, (S, 3)), u(hap, (C, 2)), u(pair_off, (S + 1,)), u(pair, (pair_off[S],)),
            np.array(keys, dtype=np.uint32).reshape(len(keys), 3), u([junction[k] for k in keys], (len(keys),)), sum(junction.values()))


def top(junction, junction_count, s, n):
    """the first n junctions of species s: count descending, then node_a, then node_b ascending -> indices into junction"""
    idx = [i for i in range(len(junction)) if int(junction[i][0]) == s]
    idx.sort(key=lambda i: (-int(junction_count[i]), int(junction[i][1]), int(junction[i][2])))
    return idx[:n]


def check_identities(species, extra, hap, pair_off, pair, junction, junction_count, cand_off, support_species=None):
    """the identities of the contract, for every species of 1 <= K_s <= 64 (all three numbers of Q); support_species = species_out of the read support
    pass on the same candidates"""
    S = len(species)
    for s in range(S):
        c0, c1 = int(cand_off[s]), int(cand_off[s + 1])
        K = c1 - c0
        sp = species[s].astype(np.int64)
        if K == 0 or K > 64:
            assert not sp[1:].any() and not extra[s].any() and pair_off[s + 1] == pair_off[s]
            assert not hap[c0:c1].any() and not (junction[:, 0] == s).any()
            continue
        assert np.array_equal(sp[COUNTED], sp[1:].sum(axis=0))
        mos = sp[MOSAIC1] + sp[MOSAIC2] + sp[MOSAIC3PLUS]
        if support_species is not None:
            sup = support_species[s].astype(np.int64)
            assert np.array_equal(sup[0], sp[COUNTED])
            assert np.array_equal(sp[COMPATIBLE], sup[0] - sup[1]) and np.array_equal(mos + sp[FOREIGN], sup[1])
        h = hap[c0:c1].astype(np.int64)
        assert h[:, 0].sum() == int(extra[s, N_SEGMENTS]) and h[:, 1].sum() == mos[1]
        m = pair[int(pair_off[s]):int(pair_off[s + 1])].reshape(K, K).astype(np.int64)
        mine = junction[:, 0] == s
        assert m.sum() == int(extra[s, N_BREAKS]) == int(junction_count[mine].sum()) == int(extra[s, N_SEGMENTS]) - mos[0]
        assert not np.diag(m).any()
        assert int(extra[s, N_SEGMENTS]) >= 2 * sp[MOSAIC1, 0] + 3 * sp[MOSAIC2, 0] + 4 * sp[MOSAIC3PLUS, 0]
        assert (int(extra[s, FOREIGN_STEPS]) > 0) == (sp[FOREIGN, 0] > 0) and int(extra[s, FOREIGN_STEPS]) <= sp[FOREIGN, 1]
        if K == 1:
            assert not mos.any() and not h.any() and not mine.any()
