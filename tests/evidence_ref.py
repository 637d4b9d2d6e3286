"""The contract of pantax_hip_strain_evidence (include/pantax_hip.h, "per-strain node evidence") in numpy, written from the header comment alone:
every node v of a species is counted once; M(v) = the selected haplotypes whose walk visits v at least once, m(v) = |M(v)|,
Q(v) = (1, node_len[v], node_base_cov[v], bases_per_node[v]).  Per selection entry: all = sum of Q over the nodes its haplotype visits, private = over the
nodes only it visits among the selected.  Per species: total = every node, orphan = m(v) = 0, core = m(v) = K (K >= 1; zeros when K = 0).  Integers."""
import numpy as np


def species_evidence(node_len, walks, cov, bases):
    """one species: node_len / cov / bases [V], walks = the selected haplotypes' walks (local node ids, a node may repeat)
    -> (hap uint64 [K, 2, 4], species uint64 [3, 4])"""
    V, K = len(node_len), len(walks)
    Q = np.stack([np.ones(V, dtype=np.uint64), np.asarray(node_len, dtype=np.uint64), np.asarray(cov, dtype=np.uint64), np.asarray(bases, dtype=np.uint64)], axis=1)
    sets = [np.unique(np.asarray(w, dtype=np.int64)) for w in walks]     # node-level membership: a node walked twice counts once
    m = np.zeros(V, dtype=np.int64)
    for nodes in sets:
        m[nodes] += 1
    hap = np.zeros((K, 2, 4), dtype=np.uint64)
    for c, nodes in enumerate(sets):
        hap[c, 0] = Q[nodes].sum(axis=0, dtype=np.uint64)
        hap[c, 1] = Q[nodes[m[nodes] == 1]].sum(axis=0, dtype=np.uint64)
    sp = np.zeros((3, 4), dtype=np.uint64)
    sp[0] = Q.sum(axis=0, dtype=np.uint64)
    sp[1] = Q[m == 0].sum(axis=0, dtype=np.uint64)
    if K >= 1:
        sp[2] = Q[m == K].sum(axis=0, dtype=np.uint64)
    return hap, sp


def evidence(species, sel_off, sel_hap, cov, bases):
    """species: graphs with node_len, path_off, path_nodes (species-local ids) in db order; cov / bases [V] over the concatenated nodes.
    -> (hap uint64 [C, 2, 4] in the order of sel_hap, species uint64 [S, 3, 4])"""
    node_off = np.concatenate([[0], np.cumsum([len(g.node_len) for g in species])]).astype(np.int64)
    haps, sps = [], []
    for s, g in enumerate(species):
        lo, hi = int(node_off[s]), int(node_off[s + 1])
        walks = [g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])] for h in (int(sel_hap[c]) for c in range(int(sel_off[s]), int(sel_off[s + 1])))]
        h, sp = species_evidence(g.node_len, walks, cov[lo:hi], bases[lo:hi])
        haps.append(h)
        sps.append(sp)
    hap = np.concatenate(haps) if haps else np.zeros((0, 2, 4), dtype=np.uint64)
    return hap, (np.stack(sps) if sps else np.zeros((0, 3, 4), dtype=np.uint64))
