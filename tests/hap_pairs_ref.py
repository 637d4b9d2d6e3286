"""The contract of pantax_hip_db_hap_pairs and of the --db-pairs table (include/pantax_hip.h, "pairwise strain distinguishability") in numpy, written from
the header comment alone: every node v of a species is counted once; M(v) = the selected haplotypes whose walk visits v at least once, m(v) = |M(v)|,
Q(v) = (1, node_len[v]).  pair[a][b] = the sum of Q over the nodes with the haplotypes at positions a and b of the species' list both in M(v): with B the 0/1
visits matrix [V, K] that is B^T diag(Q) B.  Per species: total = every node, none = m(v) = 0, core = m(v) = K (K >= 1; zeros when K = 0).  Integers."""
import numpy as np

MAX_K = 256   # selected haplotypes of a species the call serves


def visits(n_nodes, walks):
    """B int64 [V, K]: 1 where walk k visits the node (a node walked twice counts once)"""
    B = np.zeros((n_nodes, len(walks)), dtype=np.int64)
    for k, w in enumerate(walks):
        B[np.asarray(w, dtype=np.int64), k] = 1
    return B


def species_pairs(node_len, walks):
    """one species: node_len [V], walks = the selected haplotypes' walks (local node ids, a node may repeat) -> (pair uint64 [K, K, 2], species uint64 [3, 2])"""
    ln = np.asarray(node_len, dtype=np.int64)
    V, K = len(ln), len(walks)
    B = visits(V, walks)
    pair = np.stack([B.T @ B, B.T @ (B * ln[:, None])], axis=2).astype(np.uint64)
    m = B.sum(axis=1)
    Q = np.stack([np.ones(V, dtype=np.int64), ln], axis=1)
    sp = np.zeros((3, 2), dtype=np.uint64)
    sp[0] = Q.sum(axis=0)
    sp[1] = Q[m == 0].sum(axis=0)
    if K >= 1:
        sp[2] = Q[m == K].sum(axis=0)
    return pair, sp


def hap_pairs(species, sel_off, sel_hap):
    """species: graphs with node_len, path_off, path_nodes (species-local ids) in db order -> (pair_off uint64 [S+1], pair uint64 [pair_off[S], 2], with the
    K_s x K_s block of species s row-major from pair_off[s], species uint64 [S, 3, 2])"""
    pair_off, pairs, sps = [0], [], []
    for s, g in enumerate(species):
        haps = [int(sel_hap[c]) for c in range(int(sel_off[s]), int(sel_off[s + 1]))]
        walks = [g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])] for h in haps]
        p, sp = species_pairs(g.node_len, walks)
        pairs.append(p.reshape(-1, 2))
        sps.append(sp)
        pair_off.append(pair_off[-1] + len(haps) ** 2)
    pair = np.concatenate(pairs) if pairs else np.zeros((0, 2), dtype=np.uint64)
    return np.array(pair_off, dtype=np.uint64), pair, (np.stack(sps) if sps else np.zeros((0, 3, 2), dtype=np.uint64))


def derived(pair, a, b):
    """the derived quantities of one pair of a species' block pair [K, K, 2] -> (only_a_len, only_b_len, distance, class, jaccard or None)"""
    la, lb, lab = int(pair[a, a, 1]), int(pair[b, b, 1]), int(pair[a, b, 1])
    only_a, only_b = la - lab, lb - lab
    cls = "identical" if only_a == 0 and only_b == 0 else ("nested" if only_a == 0 or only_b == 0 else "distinct")
    union = la + lb - lab
    return only_a, only_b, only_a + only_b, cls, (np.float64(lab) / np.float64(union) if union else None)


HEADER = ["species_taxid", "genome_ID_a", "genome_ID_b", "class", "n_nodes_a", "len_a", "n_nodes_b", "len_b", "shared_nodes", "shared_len", "only_a_len",
          "only_b_len", "distance", "jaccard"]


def table(species, genome_id, max_distance=None):
    """the --db-pairs table over the given species (each with every haplotype selected), in their order: a list of rows of cells, the header first; every
    cell a string but jaccard, which is a float64 (to compare with the parsed cell) or "-".  genome_id(g, h) names haplotype h of graph g."""
    pair_rows, sp_rows = [], []
    for g in species:
        K = g.n_paths
        if K > MAX_K:
            sp_rows.append([g.name, str(K), "-", "skipped"] + ["-"] * 10)
            continue
        walks = [g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])] for h in range(K)]
        pair, sp = species_pairs(g.node_len, walks)
        best = None
        for a in range(K):
            for b in range(a + 1, K):
                only_a, only_b, dist, cls, jac = derived(pair, a, b)
                best = dist if best is None else min(best, dist)
                if max_distance is not None and dist > max_distance:
                    continue
                pair_rows.append([g.name, genome_id(g, a), genome_id(g, b), cls] + [str(int(x)) for x in (*pair[a, a], *pair[b, b], *pair[a, b], only_a, only_b, dist)]
                                 + ["-" if jac is None else jac])
        sp_rows.append([g.name, str(K), "-", "species", str(int(sp[0, 0])), str(int(sp[0, 1])), "-", "-", str(int(sp[2, 0])), str(int(sp[2, 1])), "-", "-",
                        "-" if best is None else str(best), "-"])
    return [HEADER] + pair_rows + sp_rows
