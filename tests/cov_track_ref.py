"""The contract of pantax_hip_strain_cov_track (include/pantax_hip.h, "per-strain coverage track") in numpy, written from the header comment alone:
step i of a walk starts at the path offset o_i = sum of the node lengths before it and belongs to window o_i // W (the window of the node's first
base; a node is never cut); a haplotype of G bases has ceil(G / W) windows; a window carries the number of its steps and the sums of node_len,
node_base_cov and bases_per_node over them.  Everything is an integer."""
import numpy as np


def walk_windows(walk, node_len, cov, bases, W):
    """walk: global node indices in path order (a node visited twice counts twice) -> (n_nodes uint32, len, covered, bases uint64), [n_win] each"""
    walk = np.asarray(walk, dtype=np.int64)
    W = int(W)
    assert W >= 1
    ln = np.asarray(node_len, dtype=np.uint64)[walk]
    end = np.cumsum(ln, dtype=np.uint64)
    G = int(end[-1]) if len(walk) else 0
    n_win = -(-G // W)
    off = end - ln                                     # o_i
    w = (off // np.uint64(W)).astype(np.int64)
    n_nodes = np.zeros(n_win, dtype=np.uint32)
    out = [np.zeros(n_win, dtype=np.uint64) for _ in range(3)]
    np.add.at(n_nodes, w, np.uint32(1))
    np.add.at(out[0], w, ln)
    np.add.at(out[1], w, np.asarray(cov, dtype=np.uint64)[walk])
    np.add.at(out[2], w, np.asarray(bases, dtype=np.uint64)[walk])
    return (n_nodes, *out)


def track(species, sel_off, sel_hap, W, cov, bases):
    """species: graphs with node_len, path_off, path_nodes (species-local ids) in db order; cov / bases [V] over the concatenated nodes.
    -> (win_off uint64 [C+1], n_nodes, len, covered, bases) in the order of sel_hap"""
    node_off = np.concatenate([[0], np.cumsum([len(g.node_len) for g in species])]).astype(np.int64)
    node_len = np.concatenate([np.asarray(g.node_len, dtype=np.int64) for g in species]) if species else np.zeros(0, dtype=np.int64)
    parts = []
    for s, g in enumerate(species):
        for c in range(int(sel_off[s]), int(sel_off[s + 1])):
            h = int(sel_hap[c])
            walk = np.asarray(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], dtype=np.int64) + node_off[s]
            parts.append(walk_windows(walk, node_len, cov, bases, W))
    win_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    cat = lambda k, dt: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, dtype=dt)
    return win_off, cat(0, np.uint32), cat(1, np.uint64), cat(2, np.uint64), cat(3, np.uint64)
