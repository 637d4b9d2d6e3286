"""The two contracts of the replication index report (include/pantax_hip.h, "own-node windows and the replication index of a strain") restated in numpy and
plain Python, written from the header comment alone.

pantax_hip_strain_growth: step i of a walk starts at the path offset o_i = the sum of the node lengths before it and belongs to window o_i // W; a
haplotype of G bases has ceil(G / W) windows.  A step of selection entry c is OWN when, among the selected haplotypes of its species, only c's haplotype
walks the step's node.  A window carries n_own (its own steps), len (node_len over all its steps), len_own and bases_own (node_len and bases_per_node
over its own steps).  Everything is an integer.

pantax_hip_growth_fit: keep the windows with len_own >= min_own; set those without bases aside; sort by depth bases / len as an exact rational (Python
integers), ties by window index; drop what lies outside [median / 8, median x 8] around the lower median; trim floor(n_f x trim_permille / 1000) from
each end; least squares of log2 depth against (t_lo + j + 0.5) / n_f in centred two-pass sums; index = 2^slope."""
import math
from functools import cmp_to_key

import numpy as np

STATUS = ("ok", "empty", "few_windows", "low_depth", "flat")
MIN_WINDOWS, MIN_DEPTH = 20, 5.0      # the constants of the report (PANTAX_HIP_GROWTH_MIN_WINDOWS, PANTAX_HIP_GROWTH_MIN_DEPTH)
WINDOW, MIN_OWN_PERMILLE, TRIM_PERMILLE = 5000, 500, 100   # the defaults of the file seam


def walk_windows(walk, own, node_len, bases, W):
    """walk: global node indices in path order; own [len(walk)] bool -> (n_own uint32, len, len_own, bases_own uint64), [n_win] each"""
    walk = np.asarray(walk, dtype=np.int64)
    own = np.asarray(own, dtype=bool)
    W = int(W)
    assert W >= 1
    ln = np.asarray(node_len, dtype=np.uint64)[walk]
    end = np.cumsum(ln, dtype=np.uint64)
    G = int(end[-1]) if len(walk) else 0
    n_win = -(-G // W)
    w = ((end - ln) // np.uint64(W)).astype(np.int64)
    n_own = np.zeros(n_win, dtype=np.uint32)
    out = [np.zeros(n_win, dtype=np.uint64) for _ in range(3)]
    np.add.at(n_own, w[own], np.uint32(1))
    np.add.at(out[0], w, ln)
    np.add.at(out[1], w[own], ln[own])
    np.add.at(out[2], w[own], np.asarray(bases, dtype=np.uint64)[walk][own])
    return (n_own, *out)


def windows(species, sel_off, sel_hap, W, bases):
    """species: graphs with node_len, path_off, path_nodes (species-local ids) in db order; bases [V] over the concatenated nodes.
    -> (win_off uint64 [C+1], n_own uint32, len, len_own, bases_own uint64) in the order of sel_hap"""
    node_off = np.concatenate([[0], np.cumsum([len(g.node_len) for g in species])]).astype(np.int64)
    node_len = np.concatenate([np.asarray(g.node_len, dtype=np.int64) for g in species]) if species else np.zeros(0, dtype=np.int64)
    parts = []
    for s, g in enumerate(species):
        haps = [int(sel_hap[c]) for c in range(int(sel_off[s]), int(sel_off[s + 1]))]
        walks = [np.asarray(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], dtype=np.int64) for h in haps]
        walkers = np.zeros(len(g.node_len), dtype=np.int64)          # how many SELECTED haplotypes walk the node (a haplotype counts once)
        for wk in walks:
            walkers[np.unique(wk)] += 1
        for wk in walks:
            parts.append(walk_windows(wk + node_off[s], walkers[wk] == 1, node_len, bases, W))
    win_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    cat = lambda k, dt: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, dtype=dt)
    return win_off, cat(0, np.uint32), cat(1, np.uint64), cat(2, np.uint64), cat(3, np.uint64)


def fit(len_own, bases_own, min_own, trim_permille=TRIM_PERMILLE, min_windows=MIN_WINDOWS, min_depth=MIN_DEPTH):
    """the windows of ONE entry -> dict(n_kept, n_zero, n_f, n_fit, own_len, median_depth, slope, intercept, r2, index, status)"""
    ln = [int(x) for x in len_own]
    bs = [int(x) for x in bases_own]
    assert len(ln) == len(bs) and int(min_own) >= 1 and 0 <= int(trim_permille) < 500
    kept = [i for i in range(len(ln)) if ln[i] >= int(min_own)]
    pos = [i for i in kept if bs[i] > 0]

    def order(a, b):                                                 # the depth as an exact rational, then the window index
        l, h = bs[a] * ln[b], bs[b] * ln[a]
        return -1 if l < h else 1 if l > h else a - b
    pos.sort(key=cmp_to_key(order))
    depth = lambda i: float(bs[i]) / float(ln[i])
    r = dict(n_kept=len(kept), n_zero=len(kept) - len(pos), own_len=sum(ln[i] for i in kept), median_depth=0.0, slope=0.0, intercept=0.0, r2=0.0, index=1.0)
    d = []
    if pos:
        r["median_depth"] = med = depth(pos[(len(pos) - 1) // 2])
        d = [depth(i) for i in pos if med / 8.0 <= depth(i) <= med * 8.0]
    n_f = len(d)
    t_lo = n_f * int(trim_permille) // 1000
    m = n_f - 2 * t_lo
    r["n_f"], r["n_fit"] = n_f, m
    flat = True
    if m:
        y = [math.log2(d[t_lo + j]) for j in range(m)]
        x = [(float(t_lo + j) + 0.5) / float(n_f) for j in range(m)]
        flat = all(v == y[0] for v in y)
        if flat:
            r["intercept"] = y[0]
        else:
            sx = sy = 0.0
            for j in range(m):
                sx += x[j]
                sy += y[j]
            mx, my = sx / float(m), sy / float(m)
            sxx = sxy = syy = 0.0
            for j in range(m):
                dx, dy = x[j] - mx, y[j] - my
                sxx += dx * dx
                sxy += dx * dy
                syy += dy * dy
            r["slope"] = sxy / sxx
            r["intercept"] = my - r["slope"] * mx
            r["r2"] = (sxy * sxy) / (sxx * syy)
            r["index"] = 2.0 ** r["slope"]
    r["status"] = "empty" if m == 0 else "few_windows" if m < min_windows else "low_depth" if r["median_depth"] < min_depth else "flat" if flat else "ok"
    return r


def min_own_of(W, permille=MIN_OWN_PERMILLE):
    """the report's min_own: the thousandths of the window, at least one base"""
    return max(1, int(W) * int(permille) // 1000)
