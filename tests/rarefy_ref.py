"""Plain-Python restatement of the rarefaction of the strain fit (include/pantax_hip.h, "rarefaction of the strain fit"): the depth rule on Python ints, the
per-level bases_per_node of a species (the C oracle's node_coverage over the kept reads: the rule of get_node_abundances, oracle/pantax_oracle.c:224-253),
the rows, counters and member counts of every entry, and the rows of the report.  tests/test_rarefy_ref.py pins this file on a hand-computed case and the
library's host helper against it; tests/test_gpu_rarefy.py compares the stage call with it."""
import numpy as np

from tests import bootstrap_ref as bref
from tests.helpers import select_reads

M64 = (1 << 64) - 1
DEPTH_MAX = 63
HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "level", "fraction", "n_solved", "predicted_coverage", "refit", "mean", "sd", "min", "max",
          "scaled_mean", "zero_fraction", "n_member", "n_only", "n_reads", "bases", "n_rows", "objective"]


def depth(seed, b, r):
    """min(63, leading zero bits of sm(sm(seed ^ sm(b)) + r))"""
    h = bref.sm((bref.sm((seed ^ bref.sm(b)) & M64) + r) & M64)
    return min(DEPTH_MAX, 64 - h.bit_length())


def depths(seed, b, n_reads):
    return np.array([depth(seed, b, r) for r in range(n_reads)], dtype=np.int64)


def entry(n_levels, b, level):
    """entry of level >= 1 of replicate b >= 1; entry 0 is the full sample"""
    return 1 + (b - 1) * n_levels + (level - 1)


def species_bases(g, reads, keep):
    """bases_per_node (int64 [V_s]) of species graph g over the reads `keep` (indices or a mask over reads)"""
    from oracle import oracle as orc
    G = orc.Graph(g.node_len, g.path_off, g.path_nodes)
    idx = np.nonzero(keep)[0] if np.asarray(keep).dtype == bool else np.asarray(keep)
    so, nid, ps, pe = select_reads(reads, idx)
    return orc.node_coverage(G, None, g.range_start, so, nid, ps, pe)[0]


def visits(g):
    v = np.zeros((g.n_nodes, g.n_paths), dtype=bool)
    for h in range(g.n_paths):
        v[g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], h] = True
    return v


def entry_rows(g, bases, sel):
    """the LP rows of one entry of one species over the selected haplotypes `sel` (column order): (mask, a) sorted by (mask, a)"""
    member = visits(g)[:, sel] if len(sel) else np.zeros((g.n_nodes, 0), dtype=bool)
    mask, a, _ = bref.species_rows(g.node_len, bases, member)
    order = np.lexsort((a, mask))
    return mask[order], a[order]


def member_counts(mask, K):
    """uint64 [K, 2] = {rows with bit k, rows with mask == 1 << k}"""
    out = np.zeros((K, 2), dtype=np.uint64)
    for k in range(K):
        out[k, 0] = int(((mask >> np.uint64(k)) & np.uint64(1)).sum())
        out[k, 1] = int((mask == np.uint64(1 << k)).sum())
    return out


def stage_reference(species, reads, sp, counted, sel_off, sel_hap, seed, n_levels, n_replicates):
    """sp int [R]: the species every read is binned to (< 0: none); counted bool [R]: the read carries no drop flag -> per entry e a list over the species of
    dict(served, rows=(mask, a), n_rows, status (0 / 1 / 'limit'), reads=[counted reads, bases added], member uint64 [K, 2])"""
    R = len(sp)
    out = []
    for e in range(1 + n_replicates * n_levels):
        b, level = (0, 0) if e == 0 else (1 + (e - 1) // n_levels, 1 + (e - 1) % n_levels)
        d = depths(seed, b, R) if e else np.zeros(R, dtype=np.int64)
        per = []
        for s, g in enumerate(species):
            sel = np.asarray(sel_hap[int(sel_off[s]):int(sel_off[s + 1])], dtype=np.int64)
            K = len(sel)
            served = 1 <= K <= 64
            rec = dict(served=served, rows=(np.zeros(0, np.uint64), np.zeros(0)), n_rows=0, status=1 if K <= 64 else "limit", reads=[0, 0],
                       member=np.zeros((K, 2), dtype=np.uint64))
            if served:
                keep = (sp == s) & counted & (d >= level)
                bases = species_bases(g, reads, keep)
                mask, a = entry_rows(g, bases, sel)
                rec.update(rows=(mask, a), n_rows=len(a), status=0 if len(a) else 1, reads=[int(keep.sum()), int(bases.sum())], member=member_counts(mask, K))
            per.append(rec)
        out.append(per)
    return out


def _mean(values):
    s = np.float64(0.0)
    for v in values:
        s = s + np.float64(v)
    return s / np.float64(len(values))


def level_entries(n_levels, n_replicates, level):
    return [0] if level == 0 else [entry(n_levels, b, level) for b in range(1, n_replicates + 1)]


def strain_rows(head, predicted_coverage, x, status, member, n_levels, n_replicates):
    """the report's rows of one strain: head = [species_taxid, strain_taxid, genome_ID]; x [E], status [E] (of its species), member [E, 2] of its entry"""
    rows = []
    for level in range(n_levels + 1):
        es = level_entries(n_levels, n_replicates, level)
        o = bref.summary([x[e] for e in es], [status[e] for e in es])
        solved = [x[e] for e in es if status[e] == 0]
        scale = np.float64(2.0 ** level)
        stats = [o[1], o[2], o[9], np.float64(max(solved)), o[1] * scale, o[8]] if o[0] > 0 else ["-"] * 6
        rows.append(head + ["strain", level, np.float64(1.0) / scale, int(o[0]), np.float64(predicted_coverage), np.float64(x[0])] + stats +
                    [_mean([member[e][0] for e in es]), _mean([member[e][1] for e in es]), "-", "-", "-", "-"])
    return rows


def species_rows(head, obj, status, n_rows, reads, n_levels, n_replicates):
    """the report's rows of one served species: obj / status / n_rows [E], reads [E, 2]"""
    rows = []
    for level in range(n_levels + 1):
        es = level_entries(n_levels, n_replicates, level)
        o = bref.summary([obj[e] for e in es], [status[e] for e in es])
        rows.append(head + ["-", "-", "species", level, np.float64(1.0) / np.float64(2.0 ** level), int(o[0])] + ["-"] * 10 +
                    [_mean([reads[e][0] for e in es]), _mean([reads[e][1] for e in es]), _mean([n_rows[e] for e in es]), o[1] if o[0] > 0 else "-"])
    return rows


def skipped_row(head):
    return head + ["-", "-", "skipped"] + ["-"] * 17


def parse_row(cells):
    """a row of the file as values: the text columns as they are, level and n_solved as ints, every other cell a float64 or '-'"""
    out = list(cells[:4])
    for i, c in enumerate(cells[4:], 4):
        out.append(c if c == "-" else int(c) if i in (4, 6) else np.float64(c))
    return out
