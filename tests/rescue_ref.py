"""The read rescue contract (DESIGN.md "Read rescue", include/pantax_hip.h) read row by row: plain Python sets, no numpy in the decisions.  The yardstick
of tests/test_gpu_rescue.py, itself pinned on hand-written cases in tests/test_rescue_ref.py.  Its `reads` are those of
tests/read_support_ref.read_support: they carry the nodes of every walk in walk order."""
import numpy as np

COUNTED, COMPATIBLE, FOREIGN, FOREIGN_RESCUED, FOREIGN_PATCHWORK, FOREIGN_NOVEL, MOSAIC, MOSAIC_RESCUED, CONTESTED = range(9)
NAMES = ("counted", "compatible", "foreign", "foreign_rescued", "foreign_patchwork", "foreign_novel", "mosaic", "mosaic_rescued", "contested")
FOREIGN_STEPS, CLAIMED_STEPS, NOVEL_STEPS = range(3)
RESCUED, ALONE, FROM_FOREIGN = range(3)
# the six outcomes of one walk, as pantax_hip_rescue_walk numbers them
W_COMPATIBLE, W_FOREIGN_RESCUED, W_FOREIGN_PATCHWORK, W_FOREIGN_NOVEL, W_MOSAIC_RESCUED, W_MOSAIC_UNRESCUED = range(6)


def walk(M, N):
    """M, N = per step the set of reported members / of candidates that walk it -> (outcome, D(r), [foreign_steps, claimed_steps, novel_steps])"""
    assert len(M) == len(N) and len(M) > 0
    C = set.intersection(*[set(m) for m in M])
    D = set.intersection(*[set(n) for n in N])
    foreign = [i for i in range(len(M)) if not M[i]]
    novel = [i for i in foreign if not N[i]]
    steps = [len(foreign), len(foreign) - len(novel), len(novel)]
    if C:
        return W_COMPATIBLE, D, steps
    if foreign:
        return (W_FOREIGN_RESCUED if D else W_FOREIGN_NOVEL if novel else W_FOREIGN_PATCHWORK), D, steps
    return (W_MOSAIC_RESCUED if D else W_MOSAIC_UNRESCUED), D, steps


def rescue(hap_nodes, reads, sel_off, sel_hap, cand_off, cand_hap):
    """hap_nodes[s][h] = the set of nodes the walk of haplotype h of species s visits.
    reads = iterable of (species or -1, counted, nodes of the walk in walk order (repeats allowed), pstart, pend).
    -> species [S][9][3], step [S][3], cand [J][3][3], cand_steps [J] as uint64"""
    S = len(hap_nodes)
    J = int(cand_off[S])
    species = [[[0, 0, 0] for _ in range(9)] for _ in range(S)]
    step = [[0, 0, 0] for _ in range(S)]
    cand = [[[0, 0, 0] for _ in range(3)] for _ in range(J)]
    cand_steps = [0] * J

    def add(dst, q):
        for i in range(3):
            dst[i] += q[i]

    for sp, counted, nodes, pstart, pend in reads:
        if sp < 0 or not counted:
            continue
        s = int(sp)
        q = (1, len(nodes), int(pend) - int(pstart) if int(pend) >= int(pstart) else 0)
        add(species[s][COUNTED], q)
        k0, k1, c0, c1 = int(sel_off[s]), int(sel_off[s + 1]), int(cand_off[s]), int(cand_off[s + 1])
        if (k1 - k0) + (c1 - c0) > 64:
            continue                                                        # skipped: counted only
        M = [set(k for k in range(k0, k1) if int(v) in hap_nodes[s][int(sel_hap[k])]) for v in nodes]
        N = [set(c for c in range(c0, c1) if int(v) in hap_nodes[s][int(cand_hap[c])]) for v in nodes]
        outcome, D, st = walk(M, N)
        for i in range(3):
            step[s][i] += st[i]
        for m, n in zip(M, N):
            if not m:
                for c in n:
                    cand_steps[c] += 1
        if outcome == W_COMPATIBLE:
            add(species[s][COMPATIBLE], q)
            continue
        is_foreign = outcome in (W_FOREIGN_RESCUED, W_FOREIGN_PATCHWORK, W_FOREIGN_NOVEL)
        add(species[s][FOREIGN if is_foreign else MOSAIC], q)
        if outcome == W_FOREIGN_PATCHWORK:
            add(species[s][FOREIGN_PATCHWORK], q)
        elif outcome == W_FOREIGN_NOVEL:
            add(species[s][FOREIGN_NOVEL], q)
        if not D:
            continue
        add(species[s][FOREIGN_RESCUED if is_foreign else MOSAIC_RESCUED], q)
        if len(D) >= 2:
            add(species[s][CONTESTED], q)
        for c in D:
            add(cand[c][RESCUED], q)
            if len(D) == 1:
                add(cand[c][ALONE], q)
            if is_foreign:
                add(cand[c][FROM_FOREIGN], q)
    u = lambda x, shape: np.array(x, dtype=np.uint64).reshape(shape)
    return u(species, (S, 9, 3)), u(step, (S, 3)), u(cand, (J, 3, 3)), u(cand_steps, (J,))


def rank(cand_hap, cand, top=0):
    """the printed order of one species' candidates: rescued span descending, then rescued reads descending, then haplotype index ascending; a candidate
    that rescues no read is left out; top = 0 keeps all -> positions"""
    idx = [c for c in range(len(cand_hap)) if int(cand[c][RESCUED][0]) > 0]
    idx.sort(key=lambda c: (-int(cand[c][RESCUED][2]), -int(cand[c][RESCUED][0]), int(cand_hap[c])))
    return idx[:top] if top else idx


def check_identities(species, step, cand, cand_steps, sel_off, cand_off):
    """the identities of the contract, for every species (all three numbers of Q)"""
    S = len(species)
    for s in range(S):
        K = int(sel_off[s + 1]) - int(sel_off[s])
        c0, c1 = int(cand_off[s]), int(cand_off[s + 1])
        J = c1 - c0
        sp = species[s].astype(np.int64)
        st = step[s].astype(np.int64)
        cd = cand[c0:c1].astype(np.int64)
        if K + J > 64:
            assert not sp[1:].any() and not st.any() and not cd.any() and not cand_steps[c0:c1].any()
            continue
        assert np.array_equal(sp[COUNTED], sp[COMPATIBLE] + sp[FOREIGN] + sp[MOSAIC])
        assert np.array_equal(sp[FOREIGN], sp[FOREIGN_RESCUED] + sp[FOREIGN_PATCHWORK] + sp[FOREIGN_NOVEL])
        assert np.array_equal(cd[:, ALONE].sum(axis=0) + sp[CONTESTED], sp[FOREIGN_RESCUED] + sp[MOSAIC_RESCUED])
        assert (cd[:, ALONE] <= cd[:, RESCUED]).all() and (cd[:, FROM_FOREIGN] <= cd[:, RESCUED]).all()
        assert st[FOREIGN_STEPS] == st[CLAIMED_STEPS] + st[NOVEL_STEPS]
        total = int(cand_steps[c0:c1].astype(np.int64).sum())
        assert total >= st[CLAIMED_STEPS] and (J != 1 or total == st[CLAIMED_STEPS])
        if J == 0:
            assert np.array_equal(sp[FOREIGN], sp[FOREIGN_NOVEL]) and not sp[FOREIGN_RESCUED].any() and not sp[MOSAIC_RESCUED].any() and not sp[CONTESTED].any()
        if K == 0:
            assert np.array_equal(sp[FOREIGN], sp[COUNTED])
        assert (st[NOVEL_STEPS] > 0) == (sp[FOREIGN_NOVEL, 0] > 0)
