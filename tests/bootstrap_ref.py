"""numpy restatement of the bootstrap of the strain fit (include/pantax_hip.h, "bootstrap of the strain fit"): the rows of a species from (node_len,
bases, membership), the weight hash with its Poisson(1) table, the expanded rows of a replicate and the summary over replicates.  The table is computed
here with `decimal` at 60 digits, not copied from the library's header.  tests/test_bootstrap_ref.py pins this file on a hand-computed case and the
library's host helpers against it; tests/test_gpu_bootstrap.py feeds the expanded rows to the oracle's LAD solver."""
from decimal import Decimal, ROUND_FLOOR, getcontext

import numpy as np

M64 = (1 << 64) - 1
W_MAX = 16


def poisson_table():
    """T[j] = floor(2^64 * sum_{i <= j} e^-1 / i!), j = 0 .. 15, as Python ints"""
    getcontext().prec = 60
    e_inv = Decimal(1) / Decimal(1).exp()
    out, cum, fact = [], Decimal(0), Decimal(1)
    for j in range(W_MAX):
        if j:
            fact *= j
        cum += e_inv / fact
        out.append(int((cum * (1 << 64)).to_integral_value(rounding=ROUND_FLOOR)))
    return out


T = poisson_table()
_T_NP = np.array(T, dtype=np.uint64)


def sm(x):
    """splitmix64's output function on Python ints"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def weight(seed, sp_key, b, v_local):
    if b == 0:
        return 1
    r = sm((sm((seed ^ sm(sp_key)) & M64) + (b << 40) + v_local) & M64)
    return sum(1 for t in T if r >= t)


def _sm_np(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def weights(seed, sp_key, b, v_local):
    """the weights of the nodes v_local (uint64 array) of one species in replicate b, vectorised"""
    v = np.asarray(v_local, dtype=np.uint64)
    if b == 0:
        return np.ones(len(v), dtype=np.int64)
    h = np.uint64(sm((seed ^ sm(sp_key)) & M64))
    with np.errstate(over="ignore"):
        r = _sm_np(h + np.uint64((b << 40) & M64) + v)
    return (r[:, None] >= _T_NP[None, :]).sum(axis=1).astype(np.int64)


def species_rows(node_len, bases, member):
    """member bool [V, K] (column k = selection entry k of the species) -> (mask uint64, a float64, v_local uint64) of the species' rows, in node order"""
    node_len = np.asarray(node_len)
    a = np.asarray(bases, dtype=np.uint64).astype(np.int64).astype(np.float64) / node_len.astype(np.float64)
    member = np.asarray(member, dtype=bool)
    K = member.shape[1]
    assert K <= 64
    mask = np.zeros(len(a), dtype=np.uint64)
    for k in range(K):
        mask |= member[:, k].astype(np.uint64) << np.uint64(k)
    keep = (a > 0) & (mask != 0)
    return mask[keep], a[keep], np.nonzero(keep)[0].astype(np.uint64)


def expand(mask, a, w):
    """the replicate's rows: row i repeated w[i] times, sorted by (mask, a)"""
    m, x = np.repeat(mask, w), np.repeat(a, w)
    order = np.lexsort((x, m))
    return m[order], x[order]


def summary(x, status=None):
    """pantax_hip_bootstrap_summary: float64 [10] = {n_solved, mean, sd, q025, q25, q50, q75, q975, zero_fraction, min}"""
    x = np.asarray(x, dtype=np.float64)
    v = x if status is None else x[np.asarray(status) == 0]
    out = np.zeros(10, dtype=np.float64)
    m = len(v)
    out[0] = m
    if m == 0:
        return out
    s = np.float64(0.0)
    for t in v:                      # ascending b, plain additions
        s = s + t
    mean = s / np.float64(m)
    ss = np.float64(0.0)
    for t in v:
        d = t - mean
        ss = ss + d * d
    out[1] = mean
    out[2] = np.sqrt(ss / np.float64(m - 1)) if m >= 2 else 0.0
    srt = np.sort(v)
    for i, pm in enumerate((25, 250, 500, 750, 975)):
        out[3 + i] = srt[pm * (m - 1) // 1000]
    out[8] = np.float64((v == 0.0).sum()) / np.float64(m)
    out[9] = srt[0]
    return out
