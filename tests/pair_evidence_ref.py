"""The contract of pantax_hip_strain_pair_evidence and of the --strain-pair-evidence table (include/pantax_hip.h, "pairwise strain evidence") in numpy,
written from the header comment alone: every node v of a species is counted once; M(v) = the selected haplotypes whose walk visits v at least once,
m(v) = |M(v)|, Q(v) = (1, node_len[v], node_base_cov[v], bases_per_node[v]), all u64.  pair[a][b] = the sum of Q over the nodes with the haplotypes at
positions a and b of the species' list both in M(v): with B the 0/1 visits matrix [V, K] that is B^T diag(q) B per column q of Q.  Per species: total =
every node, orphan = m(v) = 0, core = m(v) = K (K >= 1; zeros when K = 0).  Integers; a u64 sum wraps."""
import numpy as np

MAX_K = 256   # selected haplotypes of a species the call serves


def species_pair_evidence(node_len, walks, cov, bases):
    """one species: node_len / cov / bases [V], walks = the selected haplotypes' walks (local node ids, a node may repeat)
    -> (pair uint64 [K, K, 4], species uint64 [3, 4])"""
    V, K = len(node_len), len(walks)
    Q = np.stack([np.ones(V, dtype=np.uint64), np.asarray(node_len, dtype=np.uint64), np.asarray(cov, dtype=np.uint64), np.asarray(bases, dtype=np.uint64)], axis=1)
    B = np.zeros((V, K), dtype=np.uint64)
    for k, w in enumerate(walks):
        B[np.asarray(w, dtype=np.int64), k] = 1                              # a node walked twice counts once
    pair = np.stack([B.T @ (B * Q[:, q][:, None]) for q in range(4)], axis=2).astype(np.uint64) if K else np.zeros((0, 0, 4), dtype=np.uint64)
    m = B.sum(axis=1).astype(np.int64)
    sp = np.zeros((3, 4), dtype=np.uint64)
    sp[0] = Q.sum(axis=0, dtype=np.uint64)
    sp[1] = Q[m == 0].sum(axis=0, dtype=np.uint64)
    if K >= 1:
        sp[2] = Q[m == K].sum(axis=0, dtype=np.uint64)
    return pair, sp


def pair_evidence(species, sel_off, sel_hap, cov, bases):
    """species: graphs with node_len, path_off, path_nodes (species-local ids) in db order; cov / bases [V] over the concatenated nodes
    -> (pair_off uint64 [S+1], pair uint64 [pair_off[S], 4] with the K_s x K_s block of species s row-major from pair_off[s], species uint64 [S, 3, 4])"""
    node_off = np.concatenate([[0], np.cumsum([len(g.node_len) for g in species])]).astype(np.int64)
    pair_off, pairs, sps = [0], [], []
    for s, g in enumerate(species):
        lo, hi = int(node_off[s]), int(node_off[s + 1])
        haps = [int(sel_hap[c]) for c in range(int(sel_off[s]), int(sel_off[s + 1]))]
        walks = [g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])] for h in haps]
        p, sp = species_pair_evidence(g.node_len, walks, cov[lo:hi], bases[lo:hi])
        pairs.append(p.reshape(-1, 4))
        sps.append(sp)
        pair_off.append(pair_off[-1] + len(haps) ** 2)
    pair = np.concatenate(pairs) if pairs else np.zeros((0, 4), dtype=np.uint64)
    return np.array(pair_off, dtype=np.uint64), pair, (np.stack(sps) if sps else np.zeros((0, 3, 4), dtype=np.uint64))


def only(pair, a, b):
    """only_a(a, b) = pair[a][a] - pair[a][b] of a species' block [K, K, 4]: what a walks and b does not, uint64 [4]"""
    return pair[a, a] - pair[a, b]


def pair_class(pair, a, b):
    """identical / nested / distinct from the len column, as the --db-pairs table derives it"""
    la, lb = int(only(pair, a, b)[1]), int(only(pair, b, a)[1])
    return "identical" if la == 0 and lb == 0 else ("nested" if la == 0 or lb == 0 else "distinct")


HEADER = ["species_taxid", "strain_taxid", "genome_ID", "other_strain_taxid", "other_genome_ID", "class", "n_nodes", "len", "covered", "bases", "depth", "breadth",
          "predicted_coverage", "pair_class"]


def _row(name, head, other, cls, q, pc, pcls):
    q = [int(x) for x in q]
    ratios = [np.float64(q[3]) / np.float64(q[1]), np.float64(q[2]) / np.float64(q[1])] if q[1] else ["-", "-"]
    return [name, head[0], head[1], other[0], other[1], cls] + [str(x) for x in q] + ratios + [pc, pcls]


def table(species):
    """the --strain-pair-evidence table.  species: in the order they went through the device, (name, entries, pair) with entries = the species' rows of
    strain_abundance.txt in ascending haplotype index as (strain_taxid, genome_ID, second_sol float64) and pair = its block uint64 [K, K, 4] (not looked
    at for K < 2 or K > 256).  -> a list of rows of cells, the header first; every cell a string but depth, breadth and predicted_coverage, which are
    float64 (to compare with the parsed cell) or "-"."""
    rows = [HEADER]
    for name, entries, pair in species:
        K = len(entries)
        if K < 2:
            continue
        if K > MAX_K:
            rows.append([name, "-", "-", "-", "-", "skipped"] + ["-"] * 8)
            continue
        for a in range(K):
            for b in range(a + 1, K):
                ea, eb, pcls = entries[a], entries[b], pair_class(pair, a, b)
                rows.append(_row(name, ea, eb, "shared", pair[a, b], np.float64(ea[2]) + np.float64(eb[2]), pcls))
                rows.append(_row(name, ea, eb, "only", only(pair, a, b), np.float64(ea[2]), pcls))
                rows.append(_row(name, eb, ea, "only", only(pair, b, a), np.float64(eb[2]), pcls))
    return rows
