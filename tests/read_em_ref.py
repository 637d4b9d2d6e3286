"""The read class contract (DESIGN.md "Read classes and the read-based estimate", include/pantax_hip.h) read row by row: plain Python sets and ints in the
classes, plain Python floats (IEEE f64, one rounding per operation) in the estimate, written as the header's pseudo-code.  The yardstick of
tests/test_gpu_read_em.py, itself pinned on hand-written cases in tests/test_read_em_ref.py."""
import numpy as np

COUNTED, UNEXPLAINED = 0, 1
MAX_K = 64


def read_classes(hap_nodes, reads, cand_off, cand_hap, per_read=None):
    """hap_nodes[s][h] = the set of nodes the walk of haplotype h of species s visits.
    reads = iterable of (species or -1, counted, nodes of the walk in walk order (repeats allowed), pstart, pend), as read_support_ref.read_support takes them.
    cand_off [S+1], cand_hap [C] (species-local, any order).
    -> species [S][2][3], cls_off [S+1], cls_mask [J], cls_q [J][3] as uint64 arrays; last axis {n_reads, n_steps, span}.  Bit i of a mask = the candidate
    of the species with the i-th smallest haplotype index; the classes of a species in ascending mask; a species of more than 64 candidates has none.
    per_read: a list that receives, per read in order, (species, mask) of a read that went to a class or to unexplained (mask 0), else None."""
    S = len(hap_nodes)
    species = [[[0, 0, 0] for _ in range(2)] for _ in range(S)]
    table = [dict() for _ in range(S)]
    canon = [sorted(int(cand_hap[c]) for c in range(int(cand_off[s]), int(cand_off[s + 1]))) for s in range(S)]   # ascending haplotype index

    def add(dst, q):
        for i in range(3):
            dst[i] += q[i]

    for sp, counted, nodes, pstart, pend in reads:
        if per_read is not None:
            per_read.append(None)
        if sp < 0 or not counted:
            continue
        s = int(sp)
        q = (1, len(nodes), int(pend) - int(pstart) if int(pend) >= int(pstart) else 0)
        add(species[s][COUNTED], q)
        K = len(canon[s])
        if K == 0 or K > MAX_K:
            continue
        need = set(int(v) for v in nodes)                                     # N(r)
        mask = 0
        for i, h in enumerate(canon[s]):
            if need <= hap_nodes[s][h]:
                mask |= 1 << i                                                # C(r)
        if per_read is not None:
            per_read[-1] = (s, mask)
        if mask == 0:
            add(species[s][UNEXPLAINED], q)
        else:
            add(table[s].setdefault(mask, [0, 0, 0]), q)
    cls_off, cls_mask, cls_q = [0], [], []
    for s in range(S):
        for m in sorted(table[s]):
            cls_mask.append(m)
            cls_q.append(table[s][m])
        cls_off.append(len(cls_mask))
    u = lambda x, shape: np.array(x, dtype=np.uint64).reshape(shape)
    return u(species, (S, 2, 3)), u(cls_off, (S + 1,)), u(cls_mask, (len(cls_mask),)), u(cls_q, (len(cls_mask), 3))


def read_em(mask, b, length, max_iter=1000, tol=1e-6, trace=None):
    """The estimate for one species: mask / b [J] (classes in ascending mask, their spans), length [K] (G of the candidate at bit k).
    -> (x float64 [K], n_iter, converged, delta).  trace: a list that receives a copy of x after every iteration."""
    mask = [int(m) for m in mask]
    b = [int(v) for v in b]
    G = [int(g) for g in length]
    K, J = len(G), len(mask)
    assert K <= MAX_K and max_iter >= 1 and tol >= 0.0 and all(m >> K == 0 for m in mask)
    bits = [[k for k in range(K) if (mask[j] >> k) & 1] for j in range(J)]       # the set bits of m_j, ascending k
    held = [[j for j in range(J) if (mask[j] >> k) & 1] for k in range(K)]       # the classes with bit k set, ascending j
    x = [1.0 if G[k] > 0 else 0.0 for k in range(K)]
    n_iter, converged, delta = 0, 0, 0.0
    for t in range(1, max_iter + 1):
        r = []
        for j in range(J):
            D = 0.0
            for k in bits[j]:
                D = D + x[k]
            r.append(float(b[j]) / D if D > 0.0 else 0.0)
        y = []
        for k in range(K):
            R = 0.0
            for j in held[k]:
                R = R + r[j]
            v = (x[k] * R) / float(G[k]) if G[k] > 0 else 0.0
            if v < 1e-200:
                v = 0.0
            y.append(v)
        delta, top = 0.0, 0.0
        for k in range(K):
            delta = max(delta, abs(y[k] - x[k]))
            top = max(top, y[k])
        x = y
        n_iter = t
        if trace is not None:
            trace.append(list(x))
        if delta <= tol * top:
            converged = 1
            break
    return np.array(x, dtype=np.float64), n_iter, converged, delta


def species_estimates(cand_off, cand_hap, cand_len, cls_off, cls_mask, cls_q, max_iter=1000, tol=1e-6):
    """the stage call's x [C] (caller's order), n_iter, converged, delta [S] from the classes: a species without candidates, of more than 64, or without
    classes gets zeros and n_iter = 0"""
    S = len(cand_off) - 1
    C = int(cand_off[S])
    x = np.zeros(C, dtype=np.float64)
    n_iter = np.zeros(S, dtype=np.uint32)
    converged = np.zeros(S, dtype=np.int32)
    delta = np.zeros(S, dtype=np.float64)
    for s in range(S):
        c0, c1 = int(cand_off[s]), int(cand_off[s + 1])
        j0, j1 = int(cls_off[s]), int(cls_off[s + 1])
        if c1 - c0 == 0 or c1 - c0 > MAX_K or j1 == j0:
            continue
        order = sorted(range(c0, c1), key=lambda c: int(cand_hap[c]))         # canonical order -> caller's entries
        xs, n_iter[s], converged[s], delta[s] = read_em(cls_mask[j0:j1], cls_q[j0:j1, 2], [int(cand_len[c]) for c in order], max_iter, tol)
        for i, c in enumerate(order):
            x[c] = xs[i]
    return x, n_iter, converged, delta
