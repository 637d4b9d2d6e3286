"""The contract of pantax_hip_strain_depth and its host helpers (include/pantax_hip.h, "per-strain depth distribution") read row by row in plain Python,
written from the header comment alone: loops over nodes, Python integers, no numpy arithmetic (arrays are only read element by element and, at the
very end, filled for the comparison).

Every node v of a species is counted once; M(v) = the selected haplotypes whose walk visits v at least once, m(v) = |M(v)|; the depth of a node is
d(v) = bases_per_node[v] // node_len[v] (0 when node_len[v] = 0) and falls into bin depth_bin(d) of 96.  A histogram is [96][2]: per bin the sums of
(1, node_len[v]).  Per selection entry: all (its haplotype visits v), private (only it does among the selected).  Per species: total (every node),
orphan (m(v) = 0)."""
import numpy as np

BINS = 96
U64_MAX = 2 ** 64 - 1
HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "n_nodes", "len", "len_zero", "q05", "q25", "q50", "q75", "q95", "q50_hi", "predicted_coverage"]
QUANTILES = (50, 250, 500, 750, 950)     # per mille: q05 q25 q50 q75 q95


def depth_bin(d):
    """d < 32: the bin is d; else four bins per octave from 2^5, bin 95 takes everything from 2^21 up"""
    assert 0 <= d <= U64_MAX
    if d < 32:
        return d
    e = d.bit_length() - 1               # floor(log2 d)
    return min(95, 32 + 4 * (e - 5) + ((d >> (e - 2)) & 3))


def _lo(b):
    if b < 32:
        return b
    return (4 + (b - 32) % 4) << (3 + (b - 32) // 4)


def bin_range(b):
    """(lo, hi) of bin b: lo <= d < hi for its depths; hi(95) = 2^64 - 1 (and 2^64 - 1 itself belongs to bin 95)"""
    assert 0 <= b < BINS
    return _lo(b), (_lo(b + 1) if b < BINS - 1 else U64_MAX)


def quantile(hist, per_mille):
    """hist [96][2] -> the smallest bin whose cumulative len is at least max(1, ceil(T per_mille / 1000)), T = the sum of len; None when T = 0"""
    assert 0 <= per_mille <= 1000
    T = 0
    for b in range(BINS):
        T += int(hist[b][1])
    if T == 0:
        return None
    target = max(1, -((-T * per_mille) // 1000))
    cum = 0
    for b in range(BINS):
        cum += int(hist[b][1])
        if cum >= target:
            return b
    raise AssertionError("unreachable")


def node_depth(bases, length):
    return 0 if length == 0 else int(bases) // int(length)


def _empty():
    return [[0, 0] for _ in range(BINS)]


def species_depth(node_len, walks, bases):
    """one species: node_len / bases [V], walks = the selected haplotypes' walks (local node ids, a node may repeat)
    -> (hap [K][2] histograms as nested lists: all, private; species [2] histograms: total, orphan)"""
    V, K = len(node_len), len(walks)
    M = [[] for _ in range(V)]                      # M(v), node-level: a node walked twice by k is listed once
    for k in range(K):
        for v in walks[k]:
            v = int(v)
            if not M[v] or M[v][-1] != k:
                M[v].append(k)
    hap = [[_empty(), _empty()] for _ in range(K)]
    sp = [_empty(), _empty()]

    def add(hist, b, length):
        hist[b][0] += 1
        hist[b][1] += length

    for v in range(V):
        length = int(node_len[v])
        b = depth_bin(node_depth(int(bases[v]), length))
        add(sp[0], b, length)
        if len(M[v]) == 0:
            add(sp[1], b, length)
        for k in M[v]:
            add(hap[k][0], b, length)
            if len(M[v]) == 1:
                add(hap[k][1], b, length)
    return hap, sp


def depth(species, sel_off, sel_hap, cov, bases):
    """species: graphs with node_len, path_off, path_nodes (species-local ids) in db order; bases [V] over the concatenated nodes (cov, the node_base_cov
    of the same coverage pass, is taken for symmetry with evidence_ref.evidence: the contract does not read it).
    -> (hap uint64 [C, 2, 96, 2] in the order of sel_hap, species uint64 [S, 2, 96, 2])"""
    assert len(cov) == len(bases)
    haps, sps, lo = [], [], 0
    for s, g in enumerate(species):
        hi = lo + len(g.node_len)
        walks = [g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])] for h in (int(sel_hap[c]) for c in range(int(sel_off[s]), int(sel_off[s + 1])))]
        h, sp = species_depth(g.node_len, walks, bases[lo:hi])
        haps += h
        sps.append(sp)
        lo = hi
    return np.array(haps, dtype=np.uint64).reshape(len(haps), 2, BINS, 2), np.array(sps, dtype=np.uint64).reshape(len(sps), 2, BINS, 2)


def hist_row(species_taxid, strain_taxid, genome_id, cls, hist, predicted_coverage):
    """one row of the --strain-depth TSV (its columns as strings) for one histogram; predicted_coverage is the text to print ("-" on species rows)"""
    n = length = 0
    for b in range(BINS):
        n += int(hist[b][0])
        length += int(hist[b][1])
    row = [species_taxid, strain_taxid, genome_id, cls, str(n), str(length), str(int(hist[0][1]))]
    for pm in QUANTILES:
        b = quantile(hist, pm)
        row.append("-" if b is None else str(bin_range(b)[0]))
    b50 = quantile(hist, 500)
    row.append("-" if b50 is None else str(bin_range(b50)[1]))
    row.append(predicted_coverage)
    return row


def report_rows(strains, species):
    """strains: (species_taxid, strain_taxid, genome_ID, hist all, hist private, predicted_coverage text) in the order of strain_abundance.txt;
    species: (species_taxid, hist total, hist orphan) in the run's order -> every line of the TSV, the header first"""
    rows = [list(HEADER)]
    for sp, st, gid, h_all, h_priv, pc in strains:
        rows.append(hist_row(sp, st, gid, "all", h_all, pc))
        rows.append(hist_row(sp, st, gid, "private", h_priv, pc))
    for sp, h_total, h_orphan in species:
        rows.append(hist_row(sp, "-", "-", "total", h_total, "-"))
        rows.append(hist_row(sp, "-", "-", "orphan", h_orphan, "-"))
    return rows
