"""The per-strain read support contract (DESIGN.md "Per-strain read support", include/pantax_hip.h) read row by row: plain Python sets, no numpy in
the decisions.  The yardstick of tests/test_gpu_read_support.py, itself pinned on hand-written cases in tests/test_read_support_ref.py."""
import numpy as np

COMPATIBLE, UNIQUE, ASSIGNED = 0, 1, 2
COUNTED, UNEXPLAINED, AMBIGUOUS, UNINFORMATIVE = 0, 1, 2, 3


def read_support(hap_nodes, reads, cand_off, cand_hap, cand_w):
    """hap_nodes[s][h] = the set of nodes the walk of haplotype h of species s visits.
    reads = iterable of (species or -1, counted, nodes of the walk in walk order (repeats allowed), pstart, pend).
    cand_off [S+1], cand_hap [C] (species-local, any order), cand_w [C].
    -> hap [C][3][3], species [S][4][3], pair_off [S+1], pair [pair_off[S]] as uint64 arrays; last axis {n_reads, n_steps, span}."""
    S = len(hap_nodes)
    C = int(cand_off[S])
    hap = [[[0, 0, 0] for _ in range(3)] for _ in range(C)]
    species = [[[0, 0, 0] for _ in range(4)] for _ in range(S)]
    pair_off = [0]
    for s in range(S):
        K = int(cand_off[s + 1]) - int(cand_off[s])
        pair_off.append(pair_off[-1] + (K * K if K <= 64 else 0))
    pair = [0] * pair_off[S]

    def add(dst, q):
        for i in range(3):
            dst[i] += q[i]

    for sp, counted, nodes, pstart, pend in reads:
        if sp < 0 or not counted:
            continue
        s = int(sp)
        q = (1, len(nodes), int(pend) - int(pstart) if int(pend) >= int(pstart) else 0)
        add(species[s][COUNTED], q)
        c0, c1 = int(cand_off[s]), int(cand_off[s + 1])
        K = c1 - c0
        if K == 0:
            continue
        need = set(int(v) for v in nodes)                                     # N(r)
        comp = [c for c in range(c0, c1) if need <= hap_nodes[s][int(cand_hap[c])]]   # C(r), as candidate entries
        if not comp:
            add(species[s][UNEXPLAINED], q)
        if len(comp) >= 2:
            add(species[s][AMBIGUOUS], q)
        if len(comp) == K:
            add(species[s][UNINFORMATIVE], q)
        for c in comp:
            add(hap[c][COMPATIBLE], q)
        if len(comp) == 1:
            add(hap[comp[0]][UNIQUE], q)
        if comp:
            wmax = max(float(cand_w[c]) for c in comp)
            best = min((c for c in comp if float(cand_w[c]) == wmax), key=lambda c: int(cand_hap[c]))   # ties: the smallest haplotype index
            add(hap[best][ASSIGNED], q)
        if K <= 64:
            for a in comp:
                for b in comp:
                    pair[pair_off[s] + (a - c0) * K + (b - c0)] += 1
    u = lambda x, shape: np.array(x, dtype=np.uint64).reshape(shape)
    return u(hap, (C, 3, 3)), u(species, (S, 4, 3)), u(pair_off, (S + 1,)), u(pair, (pair_off[S],))


def check_identities(hap, species, pair_off, pair, cand_off):
    """the identities of the contract, for every species of K_s >= 1 (all three numbers of Q)"""
    S = len(species)
    for s in range(S):
        c0, c1 = int(cand_off[s]), int(cand_off[s + 1])
        K = c1 - c0
        if K == 0:
            assert not species[s, 1:].any()
            continue
        h = hap[c0:c1].astype(np.int64)
        sp = species[s].astype(np.int64)
        assert np.array_equal(sp[COUNTED], sp[UNEXPLAINED] + h[:, ASSIGNED].sum(axis=0))
        assert np.array_equal(h[:, UNIQUE].sum(axis=0) + sp[AMBIGUOUS] + sp[UNEXPLAINED], sp[COUNTED])
        assert np.all(h[:, UNIQUE] <= h[:, ASSIGNED]) and np.all(h[:, ASSIGNED] <= h[:, COMPATIBLE])
        if K == 1:
            assert np.array_equal(h[0, UNIQUE], h[0, ASSIGNED]) and np.array_equal(h[0, ASSIGNED], h[0, COMPATIBLE])
            assert np.array_equal(sp[UNINFORMATIVE], sp[COUNTED] - sp[UNEXPLAINED])
        if K <= 64:
            m = pair[int(pair_off[s]):int(pair_off[s + 1])].reshape(K, K)
            assert np.array_equal(m, m.T)
            assert np.array_equal(np.diag(m).astype(np.int64), h[:, COMPATIBLE, 0])
        else:
            assert pair_off[s + 1] == pair_off[s]
