"""numpy restatement of the leave-one-out test of the strain fit (include/pantax_hip.h, "leave-one-out test of the strain fit"): the rows of a species are
those of tests/bootstrap_ref.py (species_rows), entry 0 is the plain refit and entry k + 1 the same LP with column k pinned to zero -- both solved by the
oracle's own LAD solver (oracle.lad_solve with ub[k] = 0) -- and the four row counts, the index arithmetic of the outputs and the substitute are plain
numpy.  tests/test_dropout_ref.py checks this file on crafted species against SciPy's HiGHS on the same LP; tests/test_gpu_dropout.py compares the device
with it."""
import numpy as np

from tests import bootstrap_ref as bref


def sort_rows(mask, a):
    """the rows in the call's order: by (mask, a)"""
    order = np.lexsort((a, mask))
    return np.asarray(mask, dtype=np.uint64)[order], np.asarray(a, dtype=np.float64)[order]


def predictions(mask, x):
    """s_v = the f64 sum of x_j over the set bits of mask_v in ascending j (adding 0.0 for a clear bit changes nothing: x >= 0)"""
    mask = np.asarray(mask, dtype=np.uint64)
    s = np.zeros(len(mask), dtype=np.float64)
    for j in range(len(x)):
        bit = ((mask >> np.uint64(j)) & np.uint64(1)).astype(bool)
        s = s + np.where(bit, np.float64(x[j]), 0.0)
    return s


def residuals(mask, a, x):
    return np.abs(predictions(mask, x) - np.asarray(a, dtype=np.float64))


def counts(mask, a, x_full, x_drop, k):
    """{n_member, n_only, n_worse, n_better} of entry k + 1 from the two delivered solutions"""
    mask = np.asarray(mask, dtype=np.uint64)
    r0, r1 = residuals(mask, a, x_full), residuals(mask, a, x_drop)
    member = ((mask >> np.uint64(k)) & np.uint64(1)).astype(bool)
    return np.array([member.sum(), (mask == np.uint64(1 << k)).sum(), (r1 > r0).sum(), (r1 < r0).sum()], dtype=np.uint64)


def box(a, K, k=None):
    ub = np.full(K, 1.05 * np.max(a))
    if k is not None:
        ub[k] = 0.0
    return ub


def solve_entry(mask, a, K, k=None):
    """-> (x, objective as a SUM, status) of the refit (k None) or of the fit without column k, by the oracle's solver"""
    from oracle import oracle as orc
    ub = box(a, K, k)
    if not ub.any():                       # K = 1 without its one column: x = 0 is the one point of the box
        return np.zeros(K), float(np.sum(a)), 0
    x, obj, _, st = orc.lad_solve(mask, a, K, ub)
    return x, obj * len(a), st


def species_dropout(node_len, bases, member):
    """member bool [V, K] -> dict(rows, mask, a (sorted), x [K + 1, K], obj [K + 1], status [K + 1], count [K + 1, 4]) of one species by the contract"""
    member = np.asarray(member, dtype=bool)
    K = member.shape[1]
    mask, a, _ = bref.species_rows(node_len, bases, member) if K <= 64 else (np.zeros(0, np.uint64), np.zeros(0), None)
    mask, a = sort_rows(mask, a)
    n, E = len(a), K + 1
    out = dict(rows=n, mask=mask, a=a, x=np.zeros((E, K)), obj=np.zeros(E), status=np.ones(E, dtype=np.int32), count=np.zeros((E, 4), dtype=np.uint64))
    if K > 64:
        out["status"][:] = -4
        return out
    if K == 0 or n == 0:
        return out
    for e in range(E):
        x, obj, st = solve_entry(mask, a, K, None if e == 0 else e - 1)
        out["x"][e], out["obj"][e], out["status"][e] = x, obj, 0 if st == 0 else -5
    out["count"][0] = [n, 0, 0, 0]
    for k in range(K):
        out["count"][k + 1] = counts(mask, a, out["x"][0], out["x"][k + 1], k)
    return out


def x_offsets(sel_off):
    K = np.diff(np.asarray(sel_off, dtype=np.int64))
    return np.concatenate([[0], np.cumsum((K + 1) * K)]).astype(np.int64)


def entry(sel_off, s, e):
    return int(sel_off[s]) + s + e


def substitute(k, x_full, x_drop):
    """-> (column or -1, gain, shift) of pantax_hip_dropout_substitute"""
    best, arg, shift = np.float64(0.0), -1, np.float64(0.0)
    for j in range(len(x_full)):
        if j == k:
            continue
        d = np.float64(x_drop[j]) - np.float64(x_full[j])
        if d > best:
            best, arg = d, j
        shift = shift + abs(d)
    return arg, float(best if arg >= 0 else 0.0), float(shift)


def highs_objective(mask, a, K, ub):
    """the optimum of the same LP by SciPy's HiGHS: min sum t, t_v >= +-(a_v - m_v . x), 0 <= x <= ub"""
    from scipy.optimize import linprog
    mask = np.asarray(mask, dtype=np.uint64)
    n = len(a)
    M = np.array([[(int(m) >> j) & 1 for j in range(K)] for m in mask], dtype=np.float64).reshape(n, K)
    c = np.concatenate([np.zeros(K), np.ones(n)])
    A = np.block([[M, -np.eye(n)], [-M, -np.eye(n)]])
    b = np.concatenate([a, -np.asarray(a)])
    res = linprog(c, A_ub=A, b_ub=b, bounds=[(0.0, float(u)) for u in ub] + [(0.0, None)] * n, method="highs")
    assert res.status == 0, res.message
    return float(res.fun)
