"""The contract of pantax_hip_strain_near_miss (include/pantax_hip.h, "unreported-strain near misses") in numpy, written from the header comment alone:
every node v of a species is counted once; M(v) / N(v) = the reported / candidate haplotypes whose walk visits v at least once, m = |M|, n = |N|,
Q(v) = (1, node_len[v], node_base_cov[v], bases_per_node[v]).  Per candidate entry: novel = sum of Q over m(v) = 0 and h in N(v), exclusive = over
m(v) = 0 and N(v) = {h}.  Per species: orphan = m(v) = 0, claimed = m(v) = 0 and n(v) >= 1, contested = m(v) = 0 and n(v) >= 2.  Integers.
near_miss_rank restates pantax_hip_near_miss_rank."""
import numpy as np


def species_near_miss(node_len, sel_walks, cand_walks, cov, bases):
    """one species: node_len / cov / bases [V]; sel_walks / cand_walks = the walks of the reported haplotypes / of the candidates (local node ids, a node
    may repeat) -> (cand uint64 [J, 2, 4], species uint64 [3, 4])"""
    V, J = len(node_len), len(cand_walks)
    Q = np.stack([np.ones(V, dtype=np.uint64), np.asarray(node_len, dtype=np.uint64), np.asarray(cov, dtype=np.uint64), np.asarray(bases, dtype=np.uint64)], axis=1)
    m = np.zeros(V, dtype=np.int64)
    for w in sel_walks:
        m[np.unique(np.asarray(w, dtype=np.int64))] += 1                 # node-level membership: a node walked twice counts once
    sets = [np.unique(np.asarray(w, dtype=np.int64)) for w in cand_walks]
    n = np.zeros(V, dtype=np.int64)
    for nodes in sets:
        n[nodes] += 1
    cand = np.zeros((J, 2, 4), dtype=np.uint64)
    for c, nodes in enumerate(sets):
        cand[c, 0] = Q[nodes[m[nodes] == 0]].sum(axis=0, dtype=np.uint64)
        cand[c, 1] = Q[nodes[(m[nodes] == 0) & (n[nodes] == 1)]].sum(axis=0, dtype=np.uint64)
    sp = np.zeros((3, 4), dtype=np.uint64)
    sp[0] = Q[m == 0].sum(axis=0, dtype=np.uint64)
    sp[1] = Q[(m == 0) & (n >= 1)].sum(axis=0, dtype=np.uint64)
    sp[2] = Q[(m == 0) & (n >= 2)].sum(axis=0, dtype=np.uint64)
    return cand, sp


def near_miss(species, sel_off, sel_hap, cand_off, cand_hap, cov, bases):
    """species: graphs with node_len, path_off, path_nodes (species-local ids) in db order; cov / bases [V] over the concatenated nodes.
    -> (cand uint64 [J, 2, 4] in the order of cand_hap, species uint64 [S, 3, 4])"""
    node_off = np.concatenate([[0], np.cumsum([len(g.node_len) for g in species])]).astype(np.int64)
    cands, sps = [], []
    for s, g in enumerate(species):
        lo, hi = int(node_off[s]), int(node_off[s + 1])
        walk = lambda h: g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])]
        sel = [walk(int(sel_hap[c])) for c in range(int(sel_off[s]), int(sel_off[s + 1]))]
        cnd = [walk(int(cand_hap[c])) for c in range(int(cand_off[s]), int(cand_off[s + 1]))]
        c, sp = species_near_miss(g.node_len, sel, cnd, cov[lo:hi], bases[lo:hi])
        cands.append(c)
        sps.append(sp)
    cand = np.concatenate(cands) if cands else np.zeros((0, 2, 4), dtype=np.uint64)
    return cand, (np.stack(sps) if sps else np.zeros((0, 3, 4), dtype=np.uint64))


def near_miss_rank(cand_hap, cand_out, top=0):
    """positions of one species' candidates: novel bases descending, novel covered descending, haplotype index ascending; without novel bases: left out;
    the first `top` (0: all)"""
    keep = [c for c in range(len(cand_hap)) if int(cand_out[c][0][3]) > 0]
    keep.sort(key=lambda c: (-int(cand_out[c][0][3]), -int(cand_out[c][0][2]), int(cand_hap[c])))
    return keep[:top] if top else keep
