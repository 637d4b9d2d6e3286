"""The fragment support contract (DESIGN.md "Fragment support", include/pantax_hip.h) read row by row: plain Python dicts, sets and lists, no numpy in
the decisions.  Key and tag of a read id, the mates of every read from keys and tags, and the fragment pass.  C(r) and the assigned strain of a read
are taken from tests/read_support_ref.py (one read at a time), so the two passes cannot drift apart.  The yardstick of tests/test_gpu_fragments.py,
itself pinned on hand-written cases in tests/test_fragments_ref.py."""
import numpy as np

from tests import read_support_ref as sup
from tests.helpers import gaf_id_hash

MATE_NONE, MATE_AMBIGUOUS = 0xFFFFFFFF, 0xFFFFFFFE
COUNTED, PAIRED, CONCORDANT, DISCORDANT, HALF, UNEXPLAINED, SINGLE, MULTI, ELSEWHERE = range(9)
NAMES = ("counted", "paired", "concordant", "discordant", "half", "unexplained", "single", "multi", "mate_elsewhere")
COMPATIBLE, UNIQUE, UNIQUE_BY_PAIR, ASSIGNED = range(4)
HAP_NAMES = ("compatible", "unique", "unique_by_pair", "assigned")
E_LIMIT = -4


def fragment_key(id_bytes):
    """-> (key, tag): "<stem>/1" and "<stem>/2" with a stem of at least one byte have the stem's id hash and the tag 1 or 2; every other id its own, tag 0"""
    b = bytes(id_bytes)
    if len(b) >= 3 and b[-2:] in (b"/1", b"/2"):
        return gaf_id_hash(b[:-2]), int(b[-1:])
    return gaf_id_hash(b), 0


def fragment_mates(key, tag):
    """-> (mate uint32 [n], counts uint64 [4] = pairs, reads without a mate, ambiguous reads, keys seen three times or more)"""
    n = len(key)
    runs = {}
    for i in range(n):
        runs.setdefault(int(key[i]), []).append(i)
    mate = [MATE_NONE] * n
    pairs = none = ambiguous = crowded = 0
    for idx in runs.values():
        if len(idx) == 1:
            none += 1
            continue
        if len(idx) == 2 and sorted(int(tag[i]) for i in idx) in ([0, 0], [1, 2]):
            mate[idx[0]], mate[idx[1]] = idx[1], idx[0]
            pairs += 1
            continue
        for i in idx:
            mate[i] = MATE_AMBIGUOUS
        ambiguous += len(idx)
        crowded += 1 if len(idx) >= 3 else 0
    return np.array(mate, dtype=np.uint32), np.array([pairs, none, ambiguous, crowded], dtype=np.uint64)


def check_mates(mate):
    """the validation of the fragment pass: an entry that is no code is the index of another read that names this one back"""
    R = len(mate)
    for r in range(R):
        m = int(mate[r])
        if m in (MATE_NONE, MATE_AMBIGUOUS):
            continue
        if m >= R or m == r or int(mate[m]) != r:
            return False
    return True


def _one_read(hap_nodes, row, cand_off, cand_hap, cand_w):
    """-> (C(r) as candidate entries, the entry of the assigned strain or None) of one counted read, through the read support reference"""
    hap = sup.read_support(hap_nodes, [row], cand_off, cand_hap, cand_w)[0]
    comp = [c for c in range(len(hap)) if hap[c, sup.COMPATIBLE, 0]]
    best = [c for c in range(len(hap)) if hap[c, sup.ASSIGNED, 0]]
    assert len(best) == (1 if comp else 0)
    return comp, (best[0] if best else None)


def strain_fragments(hap_nodes, reads, cand_off, cand_hap, cand_w, mate, fill=-2):
    """hap_nodes, reads = list of (species or -1, counted, nodes, pstart, pend), cand_off / cand_hap / cand_w as for read_support_ref.read_support; mate [R].
    -> hap [C][4][3], species [S][9][3] (uint64), status [S] (int32), pair_off [S+1], pair [pair_off[S]] (uint64), frag_n [R] (int32; entries of reads
    that are not binned keep `fill`); last axis {n, n_steps, span}.  ValueError for a mate array that does not pass check_mates."""
    if not check_mates(mate):
        raise ValueError("mate")
    reads = list(reads)
    S, R = len(hap_nodes), len(reads)
    assert len(mate) == R
    C = int(cand_off[S])
    hap = [[[0, 0, 0] for _ in range(4)] for _ in range(C)]
    species = [[[0, 0, 0] for _ in range(9)] for _ in range(S)]
    K = [int(cand_off[s + 1]) - int(cand_off[s]) for s in range(S)]
    status = [1 if K[s] == 0 else E_LIMIT if K[s] > 64 else 0 for s in range(S)]
    pair_off = [0]
    for s in range(S):
        pair_off.append(pair_off[-1] + (K[s] * K[s] if K[s] <= 64 else 0))
    pair = [0] * pair_off[S]
    frag_n = [fill] * R

    def add(dst, q):
        for i in range(3):
            dst[i] += q[i]

    def Q(row):
        return (1, len(row[2]), int(row[4]) - int(row[3]) if int(row[4]) >= int(row[3]) else 0)

    for r, row in enumerate(reads):
        s, counted = int(row[0]), bool(row[1])
        if s < 0:
            continue
        frag_n[r] = -1
        if not counted:
            continue
        add(species[s][COUNTED], Q(row))
        m = int(mate[r])
        if m == MATE_NONE:
            add(species[s][SINGLE], Q(row))
            continue
        if m == MATE_AMBIGUOUS:
            add(species[s][MULTI], Q(row))
            continue
        other = reads[m]
        if not (int(other[0]) == s and bool(other[1])):
            add(species[s][ELSEWHERE], Q(row))
            continue
        served = status[s] == 0
        if served:
            cr, ar = _one_read(hap_nodes, row, cand_off, cand_hap, cand_w)
            cm, am = _one_read(hap_nodes, other, cand_off, cand_hap, cand_w)
            F = [c for c in cr if c in cm]
            frag_n[r] = len(F)
        if m < r:
            continue                                                          # the fragment is accounted once
        q = (1, Q(row)[1] + Q(other)[1], Q(row)[2] + Q(other)[2])
        add(species[s][PAIRED], q)
        if not served:
            continue
        if F:
            add(species[s][CONCORDANT], q)
        elif cr and cm:
            add(species[s][DISCORDANT], q)
            a, b = ar - int(cand_off[s]), am - int(cand_off[s])
            pair[pair_off[s] + a * K[s] + b] += 1
            pair[pair_off[s] + b * K[s] + a] += 1
        elif cr or cm:
            add(species[s][HALF], q)
        else:
            add(species[s][UNEXPLAINED], q)
        for c in F:
            add(hap[c][COMPATIBLE], q)
        if len(F) == 1:
            add(hap[F[0]][UNIQUE], q)
            if len(cr) != 1 and len(cm) != 1:
                add(hap[F[0]][UNIQUE_BY_PAIR], q)
        if F:
            wmax = max(float(cand_w[c]) for c in F)
            best = min((c for c in F if float(cand_w[c]) == wmax), key=lambda c: int(cand_hap[c]))   # ties: the smallest haplotype index
            add(hap[best][ASSIGNED], q)
    u = lambda x, shape: np.array(x, dtype=np.uint64).reshape(shape)
    return (u(hap, (C, 4, 3)), u(species, (S, 9, 3)), np.array(status, dtype=np.int32), u(pair_off, (S + 1,)), u(pair, (pair_off[S],)),
            np.array(frag_n, dtype=np.int32))


def check_identities(hap, species, status, pair_off, pair, cand_off, sup_species=None):
    """the identities of the contract (all three numbers of a sum unless noted); sup_species: species_out of the read support call on the same candidates"""
    S = len(species)
    for s in range(S):
        sp = species[s].astype(np.int64)
        c0, c1 = int(cand_off[s]), int(cand_off[s + 1])
        K = c1 - c0
        if sup_species is not None:
            assert np.array_equal(species[s, COUNTED], sup_species[s, 0])
        twice = sp[PAIRED] * np.array([2, 1, 1])
        assert np.array_equal(sp[COUNTED], sp[SINGLE] + sp[MULTI] + sp[ELSEWHERE] + twice)
        assert status[s] == (1 if K == 0 else E_LIMIT if K > 64 else 0)
        h = hap[c0:c1].astype(np.int64)
        if status[s] != 0:
            assert not sp[CONCORDANT:UNEXPLAINED + 1].any() and not h.any()
            assert pair_off[s + 1] == pair_off[s] + (0 if K > 64 else K * K)
            continue
        assert np.array_equal(sp[PAIRED], sp[CONCORDANT] + sp[DISCORDANT] + sp[HALF] + sp[UNEXPLAINED])
        assert np.array_equal(h[:, ASSIGNED].sum(axis=0), sp[CONCORDANT])
        assert np.all(h[:, UNIQUE_BY_PAIR] <= h[:, UNIQUE]) and np.all(h[:, UNIQUE] <= h[:, ASSIGNED]) and np.all(h[:, ASSIGNED] <= h[:, COMPATIBLE])
        m = pair[int(pair_off[s]):int(pair_off[s + 1])].reshape(K, K)
        assert np.array_equal(m, m.T) and not np.diag(m).any()
        assert int(m.sum()) == 2 * int(sp[DISCORDANT, 0])


def report_rows(names, strain_rows, seq, hap, species, status, pair_off, pair, cand_off):
    """The rows of the --strain-fragments report as lists of cells (None = "-", np.float64 = a fraction).  names[s] = the species taxid; strain_rows =
    [(s, candidate entry, strain_taxid, genome_ID)] in the order of strain_abundance.txt; seq = the species in the order they went through the device."""
    frac = lambda n, of: np.float64(n) / np.float64(of) if int(of) else None
    rows = []
    for s, c, taxid, genome in strain_rows:
        for j, cls in enumerate(HAP_NAMES):
            q = hap[c, j]
            if status[s] == 0:
                rows.append([names[s], taxid, genome, cls, int(q[0]), 2 * int(q[0]), int(q[1]), int(q[2]), frac(q[0], species[s, PAIRED, 0]), None, None])
            else:
                rows.append([names[s], taxid, genome, cls] + [None] * 7)
    for s in seq:
        for j, cls in enumerate(NAMES):
            of_reads = j in (COUNTED, SINGLE, MULTI, ELSEWHERE)
            if CONCORDANT <= j <= UNEXPLAINED and status[s] != 0:
                continue
            q = species[s, j]
            n_reads = int(q[0]) if of_reads else 2 * int(q[0])
            rows.append([names[s], None, None, cls, None if of_reads else int(q[0]), n_reads, int(q[1]), int(q[2]), frac(n_reads, species[s, COUNTED, 0]), None, None])
        if status[s] == E_LIMIT:
            rows.append([names[s], None, None, "skipped"] + [None] * 7)
    first = {}
    for s, c, taxid, genome in strain_rows:
        first.setdefault(c, (taxid, genome))
    for s in seq:
        K = int(cand_off[s + 1]) - int(cand_off[s])
        if K < 2 or status[s] != 0:
            continue
        m = pair[int(pair_off[s]):int(pair_off[s + 1])].reshape(K, K)
        for a in range(K):
            for b in range(a + 1, K):
                ea, eb = int(cand_off[s]) + a, int(cand_off[s]) + b
                if not int(m[a, b]) or ea not in first or eb not in first:
                    continue
                rows.append([names[s], first[ea][0], first[ea][1], "discordant_pair", int(m[a, b]), 2 * int(m[a, b]), None, None,
                             frac(m[a, b], species[s, DISCORDANT, 0]), first[eb][0], first[eb][1]])
    return rows
