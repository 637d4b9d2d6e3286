"""The link support contract (DESIGN.md "Link support", include/pantax_hip.h) read row by row: plain Python dicts and sets, no numpy in the decisions.  The
yardstick of tests/test_gpu_links.py, itself pinned on hand-written cases in tests/test_links_ref.py.  Its `reads` are those of
tests/read_support_ref.read_support: they carry the nodes of every walk in walk order."""
import numpy as np

COUNTED, CROSSINGS, KNOWN, SKIP, SWITCH, FOREIGN = range(6)
CROSSING_NAMES = ("crossings", "known", "skip", "switch", "foreign")
DISTINCT, DISTINCT_CROSSED, CORE, CORE_CROSSED = range(4)
LINKS, CROSSED, OPEN, BROKEN, PRIVATE, PRIVATE_CROSSED, PRIVATE_BROKEN, SUPPORT = range(8)


def link(u, v):
    """the unordered pair"""
    return (min(int(u), int(v)), max(int(u), int(v)))


def crossing_class(known, ma, mb):
    """known: the crossing is a link of a member; ma, mb: the members that walk its two nodes -> KNOWN, SKIP, SWITCH or FOREIGN"""
    if known:
        return KNOWN
    if not ma or not mb:
        return FOREIGN
    return SKIP if set(ma) & set(mb) else SWITCH


def crossings(masks, known, K):
    """pantax_hip_link_crossings: masks[i] = the list positions (as an int of bits) that walk step i, known[i] = the crossing {i, i + 1} is a link
    -> [known, skip, switch, foreign]"""
    assert len(masks) >= 1 and len(known) == len(masks) - 1 and K <= 64
    out = [0, 0, 0, 0]
    bits = lambda m: {p for p in range(K) if (int(m) >> p) & 1}
    for i in range(len(masks) - 1):
        out[crossing_class(bool(known[i]), bits(masks[i]), bits(masks[i + 1])) - KNOWN] += 1
    return out


def top(flank, start, n_top=0):
    """pantax_hip_link_top: flank descending, then start ascending (then index ascending); n_top = 0 keeps all -> indices"""
    idx = sorted(range(len(flank)), key=lambda i: (-int(flank[i]), int(start[i]), i))
    return idx[:n_top] if n_top else idx


def links(walks, node_len, bases, reads, sel_off, sel_hap):
    """walks[s][h] = the walk of haplotype h of species s as a list of species-local nodes; node_len[s][v], bases[s][v] per species-local node.
    reads = iterable of (species or -1, counted, nodes of the walk in walk order (repeats allowed), pstart, pend).
    -> species [S][6], link [S][4], hap [C][8], brk_off [C+1] as uint64 and the break records as a list of
       (step, start, node_a, node_b, flank, mask) in the order of the entries, per entry in ascending step"""
    S = len(walks)
    C = int(sel_off[S])
    species = [[0] * 6 for _ in range(S)]
    table = [[0] * 4 for _ in range(S)]
    hap = [[0] * 8 for _ in range(C)]
    brk_off, records = [0], []
    reads = list(reads)
    for s in range(S):
        c0, c1 = int(sel_off[s]), int(sel_off[s + 1])
        K = c1 - c0
        mine = [nodes for sp, counted, nodes, _, _ in reads if sp == s and counted]
        species[s][COUNTED] = len(mine)
        species[s][CROSSINGS] = sum(len(nodes) - 1 for nodes in mine)
        if K > 64:
            brk_off += [brk_off[-1]] * K                                   # skipped: the first two only, no links, no records
            continue
        sel_walks = [[int(v) for v in walks[s][int(sel_hap[c])]] for c in range(c0, c1)]
        L = {}                                                             # link -> the list positions that walk it
        for p, w in enumerate(sel_walks):
            for i in range(len(w) - 1):
                L.setdefault(link(w[i], w[i + 1]), set()).add(p)
        M = {}                                                             # node -> the list positions that walk it
        for p, w in enumerate(sel_walks):
            for v in w:
                M.setdefault(v, set()).add(p)
        support = {e: 0 for e in L}
        for nodes in mine:
            for i in range(len(nodes) - 1):
                e = link(nodes[i], nodes[i + 1])
                if e in L:
                    support[e] += 1
                species[s][crossing_class(e in L, M.get(int(nodes[i]), set()), M.get(int(nodes[i + 1]), set()))] += 1
        assert species[s][KNOWN] == sum(support.values())                 # known = the sum of support over the distinct links
        everyone = set(range(K))
        table[s] = [len(L), sum(1 for e in L if support[e] > 0), sum(1 for e in L if L[e] == everyone),
                    sum(1 for e in L if L[e] == everyone and support[e] > 0)]
        for p, w in enumerate(sel_walks):
            q = hap[c0 + p]
            o = 0
            for i in range(len(w) - 1):
                e = link(w[i], w[i + 1])
                o += int(node_len[s][w[i]])                                # o_{i+1}
                crossed = support[e] > 0
                broken = not crossed and int(bases[s][w[i]]) > 0 and int(bases[s][w[i + 1]]) > 0
                private = L[e] == {p}
                q[LINKS] += 1
                q[CROSSED if crossed else BROKEN if broken else OPEN] += 1
                q[SUPPORT] += support[e]
                if private:
                    q[PRIVATE] += 1
                    q[PRIVATE_CROSSED] += 1 if crossed else 0
                    q[PRIVATE_BROKEN] += 1 if broken else 0
                if broken:
                    depth = lambda v: int(bases[s][v]) // int(node_len[s][v]) if int(node_len[s][v]) else 0
                    records.append((i, o, w[i], w[i + 1], min(depth(w[i]), depth(w[i + 1])), sum(1 << b for b in L[e])))
            brk_off.append(len(records))
    u = lambda x, shape: np.array(x, dtype=np.uint64).reshape(shape)
    return u(species, (S, 6)), u(table, (S, 4)), u(hap, (C, 8)), u(brk_off, (C + 1,)), records


def check_identities(species, table, hap, brk_off, walk_steps, sel_off):
    """the identities of the contract; walk_steps[c] = the steps of the walk of entry c"""
    S = len(species)
    for s in range(S):
        c0, c1 = int(sel_off[s]), int(sel_off[s + 1])
        K = c1 - c0
        sp, lt, hp = species[s].astype(np.int64), table[s].astype(np.int64), hap[c0:c1].astype(np.int64)
        if K > 64:
            assert not sp[KNOWN:].any() and not lt.any() and not hp.any() and int(brk_off[c1]) == int(brk_off[c0])
            continue
        assert sp[CROSSINGS] == sp[KNOWN] + sp[SKIP] + sp[SWITCH] + sp[FOREIGN]
        assert lt[DISTINCT_CROSSED] <= lt[DISTINCT] and lt[CORE_CROSSED] <= lt[CORE] <= lt[DISTINCT] and lt[CORE_CROSSED] <= lt[DISTINCT_CROSSED]
        if K == 0:
            assert sp[FOREIGN] == sp[CROSSINGS] and not lt.any()
        for c in range(c0, c1):
            q = hap[c].astype(np.int64)
            assert q[LINKS] == max(int(walk_steps[c]) - 1, 0) == q[CROSSED] + q[OPEN] + q[BROKEN]
            assert q[PRIVATE_CROSSED] <= q[CROSSED] and q[PRIVATE_BROKEN] <= q[BROKEN] and q[PRIVATE_CROSSED] + q[PRIVATE_BROKEN] <= q[PRIVATE] <= q[LINKS]
            assert int(brk_off[c + 1]) - int(brk_off[c]) == q[BROKEN]
            assert q[SUPPORT] >= q[CROSSED]
        if K == 1:
            assert hp[0, PRIVATE] == hp[0, LINKS] and sp[SWITCH] == 0 and lt[CORE] == lt[DISTINCT]
