"""numpy restatement of the add-one test of the strain fit (include/pantax_hip.h, "add-one test of the strain fit"): the columns of a species are its K
reported haplotypes and behind them its J candidates; the rows are those of tests/bootstrap_ref.py (species_rows) over all K + J columns; entry 0 pins every
candidate column to zero, entry c + 1 frees candidate c alone -- every entry solved by the oracle's own LAD solver (oracle.lad_solve with ub = 0 on the
pinned columns) -- and the four row counts, the index arithmetic of the outputs and the donor are plain numpy.  tests/test_addin_ref.py checks this file on
crafted species against SciPy's HiGHS on the same LP; tests/test_gpu_addin.py compares the device with it."""
import numpy as np

from tests import bootstrap_ref as bref
from tests.dropout_ref import highs_objective, predictions, residuals, sort_rows  # noqa: F401  (the same rows, predictions and LP)


def box(a, K, J, e):
    """upper bounds of entry e: the reported columns free, candidate c free only in entry c + 1"""
    ub = np.full(K + J, 1.05 * np.max(a))
    for c in range(J):
        if c + 1 != e:
            ub[K + c] = 0.0
    return ub


def no_reported_bit(mask, K):
    mask = np.asarray(mask, dtype=np.uint64)
    low = np.uint64((1 << K) - 1) if K < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    return (mask & low) == np.uint64(0)


def counts(mask, a, K, x_base, x_add, c):
    """{n_member, n_novel, n_better, n_worse} of entry c + 1 from the two delivered solutions"""
    mask = np.asarray(mask, dtype=np.uint64)
    r0, r1 = residuals(mask, a, x_base), residuals(mask, a, x_add)
    member = ((mask >> np.uint64(K + c)) & np.uint64(1)).astype(bool)
    return np.array([member.sum(), (member & no_reported_bit(mask, K)).sum(), (r1 < r0).sum(), (r1 > r0).sum()], dtype=np.uint64)


def counts0(mask, K):
    return np.array([len(mask), no_reported_bit(mask, K).sum(), 0, 0], dtype=np.uint64)


def solve_entry(mask, a, K, J, e):
    """-> (x, objective as a SUM, status) of entry e by the oracle's solver"""
    from oracle import oracle as orc
    ub = box(a, K, J, e)
    if not ub.any():                       # K = 0, entry 0: x = 0 is the one point of the box
        return np.zeros(K + J), float(np.sum(a)), 0
    x, obj, _, st = orc.lad_solve(mask, a, K + J, ub)
    return x, obj * len(a), st


def species_addin(node_len, bases, member, K):
    """member bool [V, W], the first K columns reported, the others candidates -> dict(rows, mask, a (sorted), x [J + 1, W], obj [J + 1], status [J + 1],
    count [J + 1, 4]) of one species by the contract"""
    member = np.asarray(member, dtype=bool)
    W = member.shape[1]
    J, E = W - K, W - K + 1
    mask, a, _ = bref.species_rows(node_len, bases, member) if 1 <= W <= 64 else (np.zeros(0, np.uint64), np.zeros(0), None)
    mask, a = sort_rows(mask, a)
    n = len(a)
    out = dict(rows=n, mask=mask, a=a, x=np.zeros((E, W)), obj=np.zeros(E), status=np.ones(E, dtype=np.int32), count=np.zeros((E, 4), dtype=np.uint64))
    if W > 64:
        out["status"][:] = -4
        return out
    if W == 0 or n == 0:
        return out
    for e in range(E):
        x, obj, st = solve_entry(mask, a, K, J, e)
        out["x"][e], out["obj"][e], out["status"][e] = x, obj, 0 if st == 0 else -5
    out["count"][0] = counts0(mask, K)
    for c in range(J):
        out["count"][c + 1] = counts(mask, a, K, out["x"][0], out["x"][c + 1], c)
    return out


def x_offsets(sel_off, cand_off):
    K, J = np.diff(np.asarray(sel_off, dtype=np.int64)), np.diff(np.asarray(cand_off, dtype=np.int64))
    return np.concatenate([[0], np.cumsum((J + 1) * (K + J))]).astype(np.int64)


def entry(cand_off, s, e):
    return int(cand_off[s]) + s + e


def donor(K, x_base, x_add):
    """-> (column or -1, loss, shift) of pantax_hip_addin_donor"""
    best, arg, shift = np.float64(0.0), -1, np.float64(0.0)
    for j in range(K):
        d = np.float64(x_base[j]) - np.float64(x_add[j])
        if d > best:
            best, arg = d, j
        shift = shift + abs(np.float64(x_add[j]) - np.float64(x_base[j]))
    return arg, float(best if arg >= 0 else 0.0), float(shift)


# ---- the crafted species of tests/test_addin_ref.py (hand-written depths) and tests/test_gpu_addin.py (reads drawn at `depth`): explicit walks, the
# haplotypes that are reported and the candidates, in column order
CRAFTED = {
    # (a) candidate 1 has the walk of reported haplotype 0; haplotype 2 overlaps both
    "twin": dict(n_nodes=36, walks=[list(range(24)), list(range(24)), list(range(12, 36))], sel=[0, 2], cand=[1], depth=[6.0, 0.0, 3.0],
                 a=[6.0] * 12 + [9.0] * 12 + [3.0] * 12),
    # (b) haplotype 1 has reads and covered private nodes (30 .. 39) but is left out of Sel; the other candidates walk stretches of reported haplotype 0
    "dropped": dict(n_nodes=40, walks=[list(range(30)), list(range(10, 40)), list(range(10, 22)), list(range(16, 30)), list(range(6, 16)), list(range(20, 28))],
                    sel=[0], cand=[3, 1, 4, 2, 5], depth=[5.0, 8.0, 0.0, 0.0, 0.0, 0.0], a=[5.0] * 10 + [13.0] * 20 + [8.0] * 10),
    # (c) no reported strain, one candidate
    "alone": dict(n_nodes=20, walks=[list(range(20))], sel=[], cand=[0], depth=[4.0], a=[4.0] * 20),
}


def crafted_member(case):
    """bool [n_nodes, W]: the columns Sel ++ Cand of a crafted species"""
    cols = list(case["sel"]) + list(case["cand"])
    member = np.zeros((case["n_nodes"], len(cols)), dtype=bool)
    for j, h in enumerate(cols):
        member[case["walks"][h], j] = True
    return member


def assert_crafted(who, name, d):
    """the stated answers of the crafted species, asked of `d` = dict(a (the rows' depths), x [E, W], obj [E], count [E, 4]) -- the reference's or the device's"""
    case = CRAFTED[name]
    K, J = len(case["sel"]), len(case["cand"])
    x, obj, count = d["x"], d["obj"], d["count"]
    gain = [float(obj[0] - obj[c + 1]) for c in range(J)]
    print("%s %s: obj %s, gain %s, coverage %s" % (who, name, [float(o) for o in obj], gain, [float(x[c + 1][K + c]) for c in range(J)]))
    if name == "twin":
        assert obj[0] > 0 and gain[0] <= 1e-9 * obj[0], (who, name)
        assert int(count[1][1]) == 0 and int(count[1][0]) == 24, (who, name)
    elif name == "dropped":
        c = case["cand"].index(1)
        assert gain[c] > 0 and x[c + 1][K + c] > 0 and int(count[c + 1][1]) > 0 and int(count[c + 1][2]) > 0, (who, name)
        assert int(count[c + 1][0]) == 30 and int(count[c + 1][1]) == 10 and int(count[0][1]) == 10, (who, name)
        assert all(gain[c] > gain[o] for o in range(J) if o != c), (who, name, gain)
        assert all(int(count[o + 1][1]) == 0 for o in range(J) if o != c), (who, name)
    elif name == "alone":
        # (the sum of a in the order of the call's slices, or in numpy's: equal to the rounding of a sum of len(a) doubles)
        assert abs(obj[0] - np.sum(d["a"])) <= len(d["a"]) * 2.0 ** -52 * np.sum(d["a"]) and not np.any(x[0]) and x.shape == (2, 1), (who, name)
        assert x[1][0] > 0 and obj[1] < obj[0], (who, name)
        assert count[0].tolist() == [len(d["a"]), len(d["a"]), 0, 0] and count[1].tolist()[:2] == [len(d["a"]), len(d["a"])], (who, name)
