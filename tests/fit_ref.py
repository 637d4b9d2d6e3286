"""The contract of pantax_hip_strain_fit (include/pantax_hip.h, "model fit per strain") in numpy, written from the header comment alone: every node v
of a species is counted once; M(v) = the selected haplotypes whose walk visits v at least once, m(v) = |M(v)|; p(v) = the f64 sum of the weights over
M(v), from +0.0, added in ascending haplotype index whatever the order of the selection; t = p * (double)len; E = 0 when !(t > 0), 2^62 when t >= 2^62,
else t rounded to the nearest integer, ties to even (np.rint); b = bases_per_node; Q(v) = (1, len, b, E, max(b - E, 0), max(E - b, 0), blind, blind ? E : 0)
with blind = (b == 0 and E > 0).  Per selection entry: all = sum of Q over the nodes its haplotype visits, private = over the nodes only it visits among
the selected.  Per species: total = every node, explained = m(v) >= 1, orphan = m(v) = 0.  u64 sums (they wrap)."""
import numpy as np

COLUMNS = ("n_nodes", "len", "bases", "expected", "excess", "deficit", "blind_nodes", "blind_expected")
E_MAX = 1 << 62


def expected_bases(p, node_len):
    """E(v) of the contract from p(v) float64 [V] and node_len [V] -> uint64 [V]"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(p, dtype=np.float64) * np.asarray(node_len).astype(np.float64)
    E = np.zeros(len(t), dtype=np.uint64)
    pos = t > 0                                                          # (a NaN is not)
    big = pos & (t >= float(E_MAX))
    mid = pos & ~big
    E[mid] = np.rint(t[mid]).astype(np.uint64)
    E[big] = E_MAX
    return E


def species_fit(node_len, haps, walks, w, bases):
    """one species: node_len / bases [V]; haps = the selected haplotype indices in the caller's order, walks / w their walks (local node ids, a node
    may repeat) and weights in the same order -> (hap uint64 [K, 2, 8] in the caller's order, species uint64 [3, 8])"""
    V, K = len(node_len), len(haps)
    sets = [np.unique(np.asarray(x, dtype=np.int64)) for x in walks]    # node-level membership: a node walked twice counts once
    p = np.zeros(V, dtype=np.float64)
    m = np.zeros(V, dtype=np.int64)
    for k in sorted(range(K), key=lambda k: int(haps[k])):               # ascending haplotype index: one IEEE addition per node and haplotype
        p[sets[k]] += np.float64(w[k])
        m[sets[k]] += 1
    E = expected_bases(p, node_len)
    b = np.asarray(bases, dtype=np.uint64)
    zero = np.uint64(0)
    blind = (b == 0) & (E > 0)
    Q = np.stack([np.ones(V, dtype=np.uint64), np.asarray(node_len, dtype=np.uint64), b, E, np.where(b > E, b - E, zero), np.where(E > b, E - b, zero),
                  blind.astype(np.uint64), np.where(blind, E, zero)], axis=1)
    hap = np.zeros((K, 2, 8), dtype=np.uint64)
    for c, nodes in enumerate(sets):
        hap[c, 0] = Q[nodes].sum(axis=0, dtype=np.uint64)
        hap[c, 1] = Q[nodes[m[nodes] == 1]].sum(axis=0, dtype=np.uint64)
    sp = np.zeros((3, 8), dtype=np.uint64)
    sp[0] = Q.sum(axis=0, dtype=np.uint64)
    sp[1] = Q[m >= 1].sum(axis=0, dtype=np.uint64)
    sp[2] = Q[m == 0].sum(axis=0, dtype=np.uint64)
    return hap, sp


def fit(species, sel_off, sel_hap, sel_w, bases):
    """species: graphs with node_len, path_off, path_nodes (species-local ids) in db order; bases [V] over the concatenated nodes.
    -> (hap uint64 [C, 2, 8] in the order of sel_hap, species uint64 [S, 3, 8])"""
    node_off = np.concatenate([[0], np.cumsum([len(g.node_len) for g in species])]).astype(np.int64)
    haps, sps = [], []
    for s, g in enumerate(species):
        lo, hi = int(node_off[s]), int(node_off[s + 1])
        cs = range(int(sel_off[s]), int(sel_off[s + 1]))
        hs = [int(sel_hap[c]) for c in cs]
        walks = [g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])] for h in hs]
        h, sp = species_fit(g.node_len, hs, walks, [sel_w[c] for c in cs], bases[lo:hi])
        haps.append(h)
        sps.append(sp)
    hap = np.concatenate(haps) if haps else np.zeros((0, 2, 8), dtype=np.uint64)
    return hap, (np.stack(sps) if sps else np.zeros((0, 3, 8), dtype=np.uint64))


def check_identities(hap, sp):
    """the identities of the contract that need nothing but the call's own output, column by column, modulo 2^64"""
    for q in (hap.reshape(-1, 8), sp.reshape(-1, 8)):
        assert np.array_equal(q[:, 2] + q[:, 5], q[:, 3] + q[:, 4])      # bases + deficit == expected + excess
        assert np.all(q[:, 7] <= q[:, 5])                                # blind_expected <= deficit
        assert np.all(q[:, 6] <= q[:, 0])
    assert np.array_equal(sp[:, 0], sp[:, 1] + sp[:, 2])                 # total == explained + orphan
    assert not sp[:, 2, 3].any() and np.array_equal(sp[:, 2, 4], sp[:, 2, 2]) and not sp[:, 2, 5:].any()   # orphan: E = 0, excess = bases
