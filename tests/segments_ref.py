"""The contract of pantax_hip_strain_segments and pantax_hip_segment_chain (include/pantax_hip.h, "absent and amplified segments along a strain") restated,
written from the header comment alone.  Step i of a walk has class 1 (gap) when node_base_cov is 0, else 2 (peak) when peak_depth > 0 and bases_per_node >=
peak_depth * node_len, else 0; a segment is a maximal run of consecutive steps with one non-zero class and carries its first step, its steps, its path
offset, its summed node length and its summed bases.  The run totals count every run, the segment arrays those of at least min_len bases.  The chain
rule is plain Python.  Everything is an integer."""
import numpy as np

GAP, PEAK = 1, 2


def step_classes(walk, node_len, cov, bases, peak_depth):
    walk = np.asarray(walk, dtype=np.int64)
    ln = np.asarray(node_len, dtype=np.uint64)[walk]
    cv = np.asarray(cov, dtype=np.uint64)[walk]
    bs = np.asarray(bases, dtype=np.uint64)[walk]
    peak = (bs >= np.uint64(peak_depth) * ln) if int(peak_depth) > 0 else np.zeros(len(walk), dtype=bool)
    return np.where(cv == 0, GAP, np.where(peak, PEAK, 0)).astype(np.uint8)


def walk_runs(walk, node_len, cov, bases, peak_depth):
    """every run of class gap or peak of one walk, in walk order -> (class uint8, step uint64, n_steps uint32, start, len, bases uint64)"""
    walk = np.asarray(walk, dtype=np.int64)
    n = len(walk)
    if n == 0:
        return (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    cls = step_classes(walk, node_len, cov, bases, peak_depth)
    ln = np.asarray(node_len, dtype=np.uint64)[walk]
    bs = np.asarray(bases, dtype=np.uint64)[walk]
    end = np.cumsum(ln, dtype=np.uint64)
    cb = np.concatenate([[0], np.cumsum(bs, dtype=np.uint64)]).astype(np.uint64)
    off = np.concatenate([[0], end]).astype(np.uint64)                 # o_i, and G behind the last step
    first = np.concatenate([[0], np.nonzero(cls[1:] != cls[:-1])[0] + 1])   # a run begins where the class changes
    last = np.concatenate([first[1:], [n]])
    keep = cls[first] != 0
    first, last = first[keep], last[keep]
    return (cls[first], first.astype(np.uint64), (last - first).astype(np.uint32), off[first], off[last] - off[first], cb[last] - cb[first])


def segments(species, sel_off, sel_hap, peak_depth, min_len, cov, bases):
    """species: graphs with node_len, path_off, path_nodes (species-local ids) in db order; cov / bases [V] over the concatenated nodes; peak_depth one
    number per selection entry (or one for all) -> what Engine.strain_segments returns: (seg_off uint64 [C+1], hap_len uint64 [C], n_runs, run_len,
    run_max uint64 [C, 2], seg_class, seg_step, seg_n_steps, seg_start, seg_len, seg_bases)"""
    min_len = int(min_len)
    assert min_len >= 1
    node_off = np.concatenate([[0], np.cumsum([len(g.node_len) for g in species])]).astype(np.int64)
    node_len = np.concatenate([np.asarray(g.node_len, dtype=np.int64) for g in species]) if species else np.zeros(0, dtype=np.int64)
    C = int(sel_off[-1])
    pd = np.broadcast_to(np.asarray(peak_depth, dtype=np.uint64), (C,))
    hap_len = np.zeros(C, dtype=np.uint64)
    n_runs, run_len, run_max = (np.zeros((C, 2), dtype=np.uint64) for _ in range(3))
    parts = []
    for s, g in enumerate(species):
        for c in range(int(sel_off[s]), int(sel_off[s + 1])):
            h = int(sel_hap[c])
            assert int(pd[c]) <= 2 ** 31
            walk = np.asarray(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])], dtype=np.int64) + node_off[s]
            hap_len[c] = np.asarray(node_len, dtype=np.uint64)[walk].sum(dtype=np.uint64)
            r = walk_runs(walk, node_len, cov, bases, pd[c])
            for k, cl in enumerate((GAP, PEAK)):
                m = r[0] == cl
                n_runs[c, k] = int(m.sum())
                run_len[c, k] = r[4][m].sum(dtype=np.uint64)
                run_max[c, k] = r[4][m].max() if m.any() else 0
            keep = r[4] >= np.uint64(min_len)
            parts.append(tuple(a[keep] for a in r))
    seg_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    dts = (np.uint8, np.uint64, np.uint32, np.uint64, np.uint64, np.uint64)
    cat = lambda k: np.concatenate([p[k] for p in parts]).astype(dts[k]) if parts else np.zeros(0, dtype=dts[k])
    return (seg_off, hap_len, n_runs, run_len, run_max, *[cat(k) for k in range(6)])


def chain(seg_class, seg_start, seg_len, seg_n_steps, seg_bases, bridge, min_span):
    """the segments of ONE haplotype in ascending start -> the chains of span >= min_span in ascending start, as a list of dicts: class, first, last (its
    first and last member) and start, end, span, in_class, n_segments, n_steps, bases.  Per class separately: a segment that begins at most `bridge`
    bases behind the end of the class's previous segment goes on with its chain."""
    chains, open_ = [], {}
    for i in range(len(seg_class)):
        k, st, ln = int(seg_class[i]), int(seg_start[i]), int(seg_len[i])
        assert k in (GAP, PEAK)
        ch = open_.get(k)
        if ch is not None and st - ch["end"] <= int(bridge):
            ch["last"] = i
            ch["end"] = st + ln
            ch["in_class"] += ln
            ch["n_segments"] += 1
            ch["n_steps"] += int(seg_n_steps[i])
            ch["bases"] += int(seg_bases[i])
        else:
            ch = {"class": k, "first": i, "last": i, "start": st, "end": st + ln, "in_class": ln, "n_segments": 1, "n_steps": int(seg_n_steps[i]),
                  "bases": int(seg_bases[i])}
            open_[k] = ch
            chains.append(ch)
    for ch in chains:
        ch["span"] = ch["end"] - ch["start"]
    return [ch for ch in chains if ch["span"] >= int(min_span)]   # (a chain begins with its first member: they stand in ascending start)


def chain_arrays(chains):
    """the list of chain() in the layout of pantax_amd.engine.segment_chain: (class uint8 [M], first, last uint64 [M], q uint64 [M, 7])"""
    q = np.array([[c[k] for k in ("start", "end", "span", "in_class", "n_segments", "n_steps", "bases")] for c in chains], dtype=np.uint64).reshape(len(chains), 7)
    return (np.array([c["class"] for c in chains], dtype=np.uint8), np.array([c["first"] for c in chains], dtype=np.uint64),
            np.array([c["last"] for c in chains], dtype=np.uint64), q)
