"""GPU tests of the read classes and the read-based estimate (pantax_hip_strain_read_em, --strain-em).  The expected classes and the expected estimate come
from the row-by-row reading of the contract in tests/read_em_ref.py (pinned by hand in tests/test_read_em_ref.py); every comparison is exact, the
estimate's bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import seam_lines as _lines, seam_profile as _profile, seam_world
from tests.read_em_ref import read_classes, read_em, species_estimates

pytestmark = pytest.mark.gpu

WALK_STEPS = (1, 2, 63, 64, 65, 130)   # in-group decide, a walk that ends on lane 63, the long kernel with two and three partials
HOT = 2000                             # copies of one walk: the hot class
WIDE = 6                               # the 64-haplotype species, all 64 as candidates


def _build():
    """The species of tests/test_gpu_read_support.py -- four tiny ones (their reads share one 64-step group), K_s = 0, 1, 2 and 3, a 64-haplotype species
    with all 64 as candidates (bit 63), a 70-haplotype species with 66 candidates (skipped), a species without candidates and one left out of the db --
    with its hand walks, plus one-step reads on every node of the 64-haplotype species whose membership mask no earlier node had (many distinct keys
    in one wave, more classes than twice the slots of the small-table option) and HOT copies of one walk."""
    import synthdata as synth
    rng = np.random.default_rng(5)
    shapes = [(2, 250), (3, 250), (2, 250), (3, 250), (1, 8000), (4, 8000), (64, 8000), (70, 8000), (3, 6000), (3, 6000)]
    species, start = [], 1
    for i, (H, glen) in enumerate(shapes):
        g = synth.make_species(rng, str(1000 + i), H, glen, start, "GCF_%06d" % (i + 1), present_frac=0.6)
        species.append(g)
        start = g.range_end + 1
    rd = synth.make_reads(rng, species[4:], 2500, adversarial_frac=0.0)
    walks, ps, pe = [], [], []

    def add(g, local_nodes, pstart=3, pend=40):
        walks.append(np.asarray(local_nodes, dtype=np.uint32) + np.uint32(g.range_start))
        ps.append(pstart)
        pe.append(pend)

    def stretch(g, h, k, at=0):
        b = int(g.path_off[h])
        assert int(g.path_off[h + 1]) - b >= at + k
        return g.path_nodes[b + at:b + at + k]

    for g in species[:4]:                                # three or more species inside the first 64-step group
        add(g, stretch(g, 0, 1), 0, 11)
        add(g, stretch(g, g.n_paths - 1, 2, at=3), 5, 9)
    for g in (species[5], species[6], species[7]):
        for k in WALK_STEPS:
            for h in (0, g.n_paths - 1):
                add(g, stretch(g, h, k, at=7), 2, 2 + 31 * k)
    two = species[5]
    a, b = stretch(two, 1, 2, at=20)
    add(two, [a, b, a, b, a])                            # a walk that visits a node twice (and more)
    add(two, stretch(two, 0, 3), 90, 10)                 # pend < pstart: span 0
    add(two, [0, two.n_nodes - 1, two.n_nodes // 2])     # unlikely to fit any candidate
    add(species[4], stretch(species[4], 0, 4))
    wide = species[WIDE]
    member = np.zeros(wide.n_nodes, dtype=np.uint64)     # node -> the haplotypes that walk it
    for h in range(wide.n_paths):
        member[np.unique(wide.path_nodes[int(wide.path_off[h]):int(wide.path_off[h + 1])])] |= np.uint64(1) << np.uint64(h)
    seen = set()
    for v in range(wide.n_nodes):
        m = int(member[v])
        if m and m not in seen:
            seen.add(m)
            add(wide, [v], 10, 10 + 7 * (len(seen) % 5))
    hot = stretch(wide, 3, 3, at=40)
    for _ in range(HOT):
        add(wide, hot, 1, 90)
    k = np.array([len(w) for w in walks], dtype=np.uint64)
    n = len(walks)
    one = lambda v: np.full(n, v, dtype=np.int64)
    reads = synth.PackedReads(np.concatenate([rd.step_off, rd.step_off[-1] + np.cumsum(k)]), np.concatenate([rd.node_id] + walks), None,
                              np.concatenate([rd.pstart, np.array(ps, dtype=np.int64)]), np.concatenate([rd.pend, np.array(pe, dtype=np.int64)]),
                              np.concatenate([rd.qlen, one(30000)]), np.concatenate([rd.mapq, one(60)]), np.concatenate([rd.plen, one(30000)]))
    R = reads.n_reads
    flags = np.zeros(R, dtype=np.uint8)
    flags[rng.choice(R - n, size=60, replace=False)] = rng.choice([1, 2], size=60).astype(np.uint8)
    flags[R - 3] = 1                                      # a dropped hand-placed read
    db = species[:9]                                      # the last species is not in the db
    picks = [[0, 1], [1], [], [2, 0, 1], [0], [2, 0], list(range(63, -1, -1)), sorted(rng.choice(70, size=66, replace=False).tolist()), []]
    off = np.cumsum([0] + [len(x) for x in picks]).astype(np.uint64)
    ch = np.array(sum(picks, []), dtype=np.uint32)
    lens = []                                             # G: the bases of the distinct nodes the candidate walks
    for s, hs in enumerate(picks):
        g = db[s]
        for h in hs:
            lens.append(int(np.asarray(g.node_len)[np.unique(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])])].sum()))
    return db, reads, flags, (off, ch, np.array(lens, dtype=np.uint64)), len(seen)


def _rows(db, reads, flags):
    from oracle import oracle as orc
    sp = orc.bin_reads(reads.step_off, reads.node_id, [g.range_start for g in db], [g.range_end for g in db])
    hap_nodes = [[set(g.path_nodes[int(g.path_off[h]):int(g.path_off[h + 1])].tolist()) for h in range(g.n_paths)] for g in db]
    so = reads.step_off.astype(np.int64)
    rows = []
    for r in range(reads.n_reads):
        s = int(sp[r])
        nodes = (reads.node_id[so[r]:so[r + 1]].astype(np.int64) - db[s].range_start).tolist() if s >= 0 else []
        rows.append((s, flags[r] == 0, nodes, int(reads.pstart[r]), int(reads.pend[r])))
    return sp, hap_nodes, rows


def _check_preconditions(db, reads, cands, exp, per_read, n_masks):
    """asserted on the reference before anything runs on the device, so that the tests cannot pass by leaving cases out"""
    species, cls_off, mask, q = exp
    off = cands[0]
    j0, j1 = int(cls_off[WIDE]), int(cls_off[WIDE + 1])
    print("classes per species", np.diff(cls_off.astype(np.int64)).tolist(), "distinct node masks of the wide species", n_masks)
    assert n_masks >= 100 and j1 - j0 >= 100                                   # many keys in one wave; more than 2 x 4 x 8 slots: two growth reruns at read_class_slots=2
    assert q[j0:j1, 0].max() >= HOT                                            # the hot class
    assert (mask[j0:j1] >> np.uint64(63)).any()                                # bit 63 is used
    k = np.diff(reads.step_off.astype(np.int64))
    for steps in WALK_STEPS:
        assert len(set(per_read[r] for r in np.nonzero(k == steps)[0] if per_read[r] is not None and per_read[r][1])) >= 2
    assert species[:, 1, 0].sum() > 0                                          # unexplained reads
    pop = np.array([bin(int(m)).count("1") for m in mask])
    assert any((pop[int(cls_off[s]):int(cls_off[s + 1])] >= 2).sum() >= 2 for s in range(len(db)))
    assert species[2, 0, 0] == 2 and not species[2, 1].any() and cls_off[3] == cls_off[2]      # K_s = 0: counted only
    assert species[7, 0, 0] > 10 and not species[7, 1].any() and cls_off[8] == cls_off[7]      # 66 candidates: skipped, counted only
    assert int(off[8]) - int(off[7]) == 66 and species[8, 0, 0] > 10 and cls_off[9] == cls_off[8]


@pytest.fixture(scope="module")
def stage():
    from pantax_amd.engine import Engine
    db, reads, flags, cands, n_masks = _build()
    sp, hap_nodes, rows = _rows(db, reads, flags)
    per_read = []
    exp = read_classes(hap_nodes, rows, cands[0], cands[1], per_read)
    _check_preconditions(db, reads, cands, exp, per_read, n_masks)
    eng = Engine(0)
    eng.upload_db(db)
    eng.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
    eng.rcls_profile(want_species=False)
    yield eng, db, reads, flags, cands, sp, exp, (hap_nodes, rows)
    eng.close()


def _same(got, exp):
    for g, e in zip(got, exp):
        assert g.dtype == np.uint64 and g.shape == e.shape
        assert np.array_equal(g, e)


def test_classes_equal_reference(stage, set_opt):
    eng, db, reads, flags, cands, sp, exp, _ = stage
    assert (sp < 0).sum() > 5 and ((sp >= 0) & (flags != 0)).sum() > 10          # "U" reads, dropped reads
    _same(eng.strain_read_em(*cands)[:4], exp)
    set_opt(eng, "read_strain_route", "walk")                                    # every species through the compact walk masks
    _same(eng.strain_read_em(*cands)[:4], exp)
    set_opt(eng, "read_strain_route", None)
    set_opt(eng, "read_class_slots", "2")                                        # tables of 2 and 4 slots: the wide species is rerun, eight times the slots each time
    eng.timing_enable(True)
    eng.timing_reset()
    _same(eng.strain_read_em(*cands)[:4], exp)
    t = eng.timing_get()
    eng.timing_enable(False)
    passes = 1                                                                   # a table overflows exactly when the species has more classes than slots
    for slots in (4, 32, 256, 2048):
        passes += int(exp[1][WIDE + 1] - exp[1][WIDE]) > slots
    assert passes >= 3 and t["read_class_kernel"][0] == passes, t
    set_opt(eng, "read_strain_route", "walk")
    _same(eng.strain_read_em(*cands)[:4], exp)


def test_shuffled_candidate_lists(stage):
    """the caller's order decides only where a candidate's x lands"""
    eng, db, reads, flags, cands, sp, exp, _ = stage
    off, ch, cl = cands
    rng = np.random.default_rng(77)
    perm = np.concatenate([int(off[s]) + rng.permutation(int(off[s + 1]) - int(off[s])) for s in range(len(db))]).astype(np.int64)
    assert (perm != np.arange(len(ch))).sum() > 60
    base = eng.strain_read_em(*cands)
    got = eng.strain_read_em(off, ch[perm], cl[perm])
    _same(got[:4], exp)
    assert np.array_equal(got[4].view(np.uint64), base[4][perm].view(np.uint64))
    for a, b in zip(got[5:], base[5:]):
        assert np.array_equal(a, b)


def test_cross_check_with_read_support(stage):
    """the class table against the counters of pantax_hip_strain_read_support on the same inputs: compatible, unique, the pair matrix, counted"""
    eng, db, reads, flags, cands, sp, exp, _ = stage
    off, ch, cl = cands
    species, cls_off, mask, q = eng.strain_read_em(*cands)[:4]
    hap, sup_species, pair_off, pair = eng.strain_read_support(off, ch, np.ones(len(ch)))
    assert np.array_equal(species[:, 0], sup_species[:, 0])
    checked = 0
    for s in range(len(db)):
        c0, c1 = int(off[s]), int(off[s + 1])
        K = c1 - c0
        m, qq = mask[int(cls_off[s]):int(cls_off[s + 1])], q[int(cls_off[s]):int(cls_off[s + 1])]
        if K == 0 or K > 64:
            assert len(m) == 0 and not species[s, 1].any()
            continue
        assert np.array_equal(species[s, 1], sup_species[s, 1])
        assert np.array_equal(qq.sum(axis=0) + species[s, 1], species[s, 0])     # the classes and unexplained make up counted
        order = sorted(range(c0, c1), key=lambda c: int(ch[c]))                  # bit i -> the caller's entry
        pm = pair[int(pair_off[s]):int(pair_off[s + 1])].reshape(K, K)
        pop = np.array([bin(int(v)).count("1") for v in m])
        for i, c in enumerate(order):
            has = ((m >> np.uint64(i)) & np.uint64(1)) == 1
            assert np.array_equal(qq[has].sum(axis=0), hap[c, 0])                # compatible
            assert np.array_equal(qq[has & (pop == 1)].sum(axis=0), hap[c, 1])   # unique
            for i2, c2 in enumerate(order):
                both = has & (((m >> np.uint64(i2)) & np.uint64(1)) == 1)
                assert qq[both, 0].sum() == pm[c - c0, c2 - c0]
                checked += 1
    assert checked > 4000


CASES = [(1, 0.0), (1, 1e-6), (7, 0.0), (7, 1e-6), (1000, 1e-6), (1000, 0.0)]


def test_estimate_equals_reference_bit_for_bit(stage, set_opt):
    eng, db, reads, flags, cands, sp, exp, _ = stage
    off, ch, cl = cands
    zero = cl.copy()
    zero[int(off[WIDE]) + 5] = 0                                                 # one candidate of the wide species without length
    zero[int(off[5])] = 0
    ran = 0
    for lens in (cl, zero):
        for max_iter, tol in CASES:
            ex, en, ec, ed = species_estimates(off, ch, lens, exp[1], exp[2], exp[3], max_iter, tol)
            got = eng.strain_read_em(off, ch, lens, max_iter, tol)
            _same(got[:4], exp)
            gx, gn, gc, gd = got[4:]
            assert gx.dtype == np.float64 and gn.dtype == np.uint32 and gc.dtype == np.int32 and gd.dtype == np.float64
            assert np.array_equal(gn, en) and np.array_equal(gc, ec), (max_iter, tol, gn, en)
            assert np.array_equal(gx.view(np.uint64), ex.view(np.uint64)), (max_iter, tol, np.nonzero(gx != ex)[0][:5])
            assert np.array_equal(gd.view(np.uint64), ed.view(np.uint64))
            ran += 1
            if max_iter == 1000 and tol > 0:
                print("iterations", gn.tolist(), "converged", gc.tolist())
                assert gc[3] == 1 and 7 < gn[3] < 1000 and gn[WIDE] > 7              # a run that converges between the caps, and a long one
                assert gn[2] == 0 and gn[7] == 0 and not gx[int(off[7]):int(off[8])].any()   # K_s = 0 and skipped: zeros
                assert gx[int(off[WIDE]):int(off[WIDE + 1])].max() > 0
                if lens is zero:
                    assert gx[int(off[WIDE]) + 5] == 0.0 and gx[int(off[5])] == 0.0
                # the classes of the wide species from global memory, not LDS: the same bits
                set_opt(eng, "read_em_lds_classes", "64")
                g2 = eng.strain_read_em(off, ch, lens, max_iter, tol)
                set_opt(eng, "read_em_lds_classes", None)
                assert np.array_equal(g2[4].view(np.uint64), gx.view(np.uint64)) and np.array_equal(g2[5], gn) and np.array_equal(g2[7].view(np.uint64), gd.view(np.uint64))
    assert ran == 12


def _raw(eng, cands, n_species=None, cls_cap=None, n_cls=0, max_iter=7, tol=1e-6):
    from pantax_amd import _ffi
    from pantax_amd.engine import p
    off, ch, cl = cands
    S = eng.S
    cs = _ffi.ReadEmSet(S if n_species is None else n_species, off.ctypes.data, ch.ctypes.data, cl.ctypes.data, max_iter, tol)
    species = np.full((S, 2, 3), 77, dtype=np.uint64)
    cls_off = np.full(S + 1, 77, dtype=np.uint64)
    cap = n_cls if cls_cap is None else cls_cap
    mask = np.full(max(n_cls, 1), 77, dtype=np.uint64)
    q = np.full((max(n_cls, 1), 3), 77, dtype=np.uint64)
    x = np.full(len(ch), 77.0)
    n_iter = np.full(S, 77, dtype=np.uint32)
    conv = np.full(S, 77, dtype=np.int32)
    delta = np.full(S, 77.0)
    rc = eng.lib.pantax_hip_strain_read_em(eng.ctx, eng.db, eng.reads, C.byref(cs), p(species), p(cls_off), cap, p(mask) if cap else None, p(q) if cap else None,
                                           p(x), p(n_iter), p(conv), p(delta))
    return rc, species, cls_off, mask, q, x, n_iter, conv, delta


def test_sizing_and_arguments(stage):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    eng, db, reads, flags, cands, sp, exp, _ = stage
    J = int(exp[1][-1])
    ex = species_estimates(cands[0], cands[1], cands[2], exp[1], exp[2], exp[3], 7, 1e-6)
    # cls_cap = 0 with null arrays: the sizes and the estimate, no classes
    rc, species, cls_off, mask, q, x, n_iter, conv, delta = _raw(eng, cands, cls_cap=0)
    assert rc == 0 and np.array_equal(cls_off, exp[1]) and np.array_equal(species, exp[0])
    assert np.array_equal(x.view(np.uint64), ex[0].view(np.uint64)) and np.array_equal(n_iter, ex[1]) and np.array_equal(conv, ex[2])
    # a short cls_cap: E_LIMIT, the sizes are out and nothing else is touched
    rc, species, cls_off, mask, q, x, n_iter, conv, delta = _raw(eng, cands, cls_cap=J - 1, n_cls=J)
    assert rc == _ffi.E_LIMIT and np.array_equal(cls_off, exp[1])
    assert np.all(species == 77) and np.all(mask == 77) and np.all(q == 77) and np.all(x == 77.0) and np.all(n_iter == 77) and np.all(conv == 77) and np.all(delta == 77.0)
    rc, species, cls_off, mask, q, x, n_iter, conv, delta = _raw(eng, cands, n_cls=J)
    assert rc == 0
    _same((species, cls_off, mask, q), exp)
    assert np.array_equal(x.view(np.uint64), ex[0].view(np.uint64)) and np.array_equal(delta.view(np.uint64), ex[3].view(np.uint64))
    off, ch, cl = cands
    twice = ch.copy()
    twice[int(off[3]) + 1] = twice[int(off[3])]                                       # a haplotype twice within a species
    far = ch.copy()
    far[int(off[0])] = 2                                                              # species 0 has two haplotypes
    for bad in ((off, twice, cl), (off, far, cl)):
        with pytest.raises(PantaxHipError) as e:
            eng.strain_read_em(*bad)
        assert e.value.code == -1
    assert _raw(eng, cands, n_species=eng.S + 1)[0] == -1
    for max_iter, tol in ((0, 1e-6), (5, -1.0), (5, float("nan")), (5, float("inf"))):
        assert _raw(eng, cands, max_iter=max_iter, tol=tol)[0] == -1
    # an empty candidate set: counted is still written
    S = len(db)
    got = eng.strain_read_em(np.zeros(S + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    assert np.array_equal(got[0][:, 0], exp[0][:, 0]) and not got[0][:, 1].any() and not got[1].any() and len(got[2]) == 0 and len(got[4]) == 0 and not got[5].any()


def test_state(stage):
    """reads that are not binned, or binned against another db, are refused as by pantax_hip_read_strains"""
    from pantax_amd._ffi import PantaxHipError
    from pantax_amd.engine import Engine
    eng, db, reads, flags, cands, sp, exp, _ = stage
    with Engine(0) as e2:
        e2.upload_db(db)
        e2.upload_reads(reads.step_off, reads.node_id, reads.pstart, reads.pend, reads.qlen, reads.mapq, flags)
        with pytest.raises(PantaxHipError) as e:
            e2.strain_read_em(*cands)                      # not binned yet
        assert e.value.code == -7
        e2.rcls_profile(want_species=False)
        e2.upload_db(db)                                   # a new db: the reads were binned against the previous one
        with pytest.raises(PantaxHipError) as e:
            e2.strain_read_em(*cands)
        assert e.value.code == -7


# ---- the file seam -----------------------------------------------------------------------------------------------------------

HEADER = ["species_taxid", "strain_taxid", "genome_ID", "class", "rank", "n_members", "members", "n_reads", "n_steps", "span", "share", "len", "em_coverage",
          "em_bases", "em_share", "predicted_coverage", "n_classes", "n_iter", "converged", "delta"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    yield from seam_world(tmp_path_factory, "pantax_em", 37, 2, 5, 12000, 30000, present_frac=0.6, with_ids=True)


def _f(x):
    return np.float64(x)


def _expected_rows(sset, db, wd, eng, n_classes, max_iter, order):
    """the report rebuilt from the stage calls (node evidence for G, then read classes and the estimate) and the run's tables; `order`: the species in the
    order the run took them"""
    table = _lines(wd / "strain_abundance.txt")[1:]
    names = [g.name for g in sset.species]
    genome_hap = {r[0]: r[0].split("_ASM")[0] for r in _lines(db / "genomes_info.txt")[1:]}
    picked = [[] for _ in names]                                             # per species: (haplotype, row of the table), ascending haplotype
    for i, t in enumerate(table):
        s = names.index(t[0])
        picked[s].append((sset.species[s].hap_names.index(genome_hap[t[2]]), i))
    for pk in picked:
        pk.sort()
    off = np.concatenate([[0], np.cumsum([len(pk) for pk in picked])]).astype(np.uint64)
    ch = np.array([h for pk in picked for h, _ in pk], dtype=np.uint32)
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    eng.get_node_abundances(fetch=False)
    ev, _ = eng.strain_evidence(off, ch)
    G = ev[:, 0, 1].copy()
    species, cls_off, mask, q, x, n_iter, conv, delta = eng.strain_read_em(off, ch, G, max_iter, 1e-6)
    sup_hap = eng.strain_read_support(off, ch, np.ones(len(ch)))[0]
    entry_of_row = {i: int(off[s]) + k for s, pk in enumerate(picked) for k, (_, i) in enumerate(pk)}
    dash = ["-"]
    out = []
    for i, t in enumerate(table):
        s = names.index(t[0])
        e = entry_of_row[i]
        c0, c1 = int(off[s]), int(off[s + 1])
        bases = [_f(x[c]) * _f(int(G[c])) for c in range(c0, c1)]
        total = _f(0.0)
        for v in bases:
            total = total + v
        m, qq = mask[int(cls_off[s]):int(cls_off[s + 1])], q[int(cls_off[s]):int(cls_off[s + 1])]
        has = ((m >> np.uint64(e - c0)) & np.uint64(1)) == 1
        sums = qq[has].sum(axis=0).tolist() if has.any() else [0, 0, 0]
        assert sums == sup_hap[e, 0].tolist()                                # = compatible of read support
        out.append(t[:3] + ["strain"] + dash * 3 + sums + dash + [int(G[e]), _f(x[e]), bases[e - c0], bases[e - c0] / total if total != 0 else "-", _f(t[3])] + dash * 4)
    for s in order:
        head = [names[s], "-", "-"]
        j0, j1 = int(cls_off[s]), int(cls_off[s + 1])
        ranked = sorted(range(j0, j1), key=lambda j: (-int(q[j, 2]), int(mask[j])))
        share = lambda v: _f(int(v)) / _f(int(species[s, 0, 2])) if species[s, 0, 2] else "-"
        for rank, j in enumerate(ranked[:n_classes]):
            bits = [b for b in range(64) if (int(mask[j]) >> b) & 1]
            members = ",".join(table[picked[s][b][1]][2] for b in bits)
            out.append(head + ["read_class", rank + 1, len(bits), members] + q[j].tolist() + [share(q[j, 2])] + dash * 9)
        rest = ranked[n_classes:]
        if rest:
            tot = q[rest].sum(axis=0)
            out.append(head + ["other", "-", len(rest), "-"] + tot.tolist() + [share(tot[2])] + dash * 9)
        out.append(head + ["unexplained"] + dash * 3 + species[s, 1].tolist() + [share(species[s, 1, 2])] + dash * 9)
        out.append(head + ["species"] + dash * 3 + species[s, 0].tolist() + dash * 6 + [j1 - j0, int(n_iter[s]), int(conv[s]), _f(delta[s])])
    return out, (species, cls_off, mask, q, x)


def _same_rows(body, exp):
    assert len(body) == len(exp)
    for row, e in zip(body, exp):
        assert len(row) == len(HEADER) == len(e)
        for got, want in zip(row, e):
            if isinstance(want, np.floating):
                assert got != "-" and np.float64(got) == want, (row, e)
            else:
                assert got == str(want), (row, e)


def _species_order(sset, body):
    names = [g.name for g in sset.species]
    seq = [r[0] for r in body if r[3] in ("species", "skipped")]
    assert sorted(seq) == sorted(names)
    return [names.index(v) for v in seq]


def test_profile_seam_read_em(world, capfd, monkeypatch):
    from pantax_amd import _ffi
    from pantax_amd._ffi import PantaxHipError
    sset, root, db, gaf, eng = world
    plain = root / "wd_plain"
    _profile(eng, db, plain, gaf)
    wd = root / "wd_em"
    _profile(eng, db, wd, gaf, strain_em_file=str(wd / "em.tsv"))
    for f in ("species_abundance.txt", "strain_abundance.txt", "ori_strain_abundance.txt"):       # the option changes none of the tables
        assert open(wd / f, "rb").read() == open(plain / f, "rb").read()
    assert not os.path.exists(plain / "em.tsv")
    rows = _lines(wd / "em.tsv")
    assert rows[0] == HEADER
    body = rows[1:]
    order = _species_order(sset, body)
    exp, (species, cls_off, mask, q, x) = _expected_rows(sset, db, wd, eng, 10, 1000, order)
    _same_rows(body, exp)
    assert x.max() > 0 and species[:, 0, 0].min() > 0 and len(mask) > len(sset.species)
    assert any(r[3] == "read_class" and int(r[5]) >= 2 for r in body)
    full = open(wd / "em.tsv", "rb").read()
    # beside the reports whose calls it shares: the evidence report (G comes from its arrays) and read support; their files and this one do not change
    wb = root / "wd_em_both"
    _profile(eng, db, wb, gaf, strain_em_file=str(wb / "em.tsv"), strain_evidence_file=str(wb / "ev.tsv"), strain_read_support_file=str(wb / "sup.tsv"))
    assert open(wb / "em.tsv", "rb").read() == full
    wo = root / "wd_em_others"
    _profile(eng, db, wo, gaf, strain_evidence_file=str(wo / "ev.tsv"), strain_read_support_file=str(wo / "sup.tsv"))
    for f in ("ev.tsv", "sup.tsv", "strain_abundance.txt"):
        assert open(wb / f, "rb").read() == open(wo / f, "rb").read()
    # --strain-em-classes 1: one class a species and an `other` row; --strain-em-iterations 3
    w1 = root / "wd_em_one"
    _profile(eng, db, w1, gaf, strain_em_file=str(w1 / "em.tsv"), strain_em_classes=1, strain_em_iterations=3)
    body1 = _lines(w1 / "em.tsv")[1:]
    exp1, _ = _expected_rows(sset, db, w1, eng, 1, 3, _species_order(sset, body1))
    _same_rows(body1, exp1)
    assert any(r[3] == "other" for r in body1) and all(r[4] == "1" for r in body1 if r[3] == "read_class") and all(int(r[17]) <= 3 for r in body1 if r[3] == "species")
    # a species-only run writes nothing; the strain-only resume behind it writes the same file
    wr = root / "wd_em_resume"
    capfd.readouterr()
    _profile(eng, db, wr, gaf, species=True, strain=False, out_binning_file=str(wr / "reads_classification.tsv"), strain_em_file=str(wr / "em_species_only.tsv"))
    assert not os.path.exists(wr / "em_species_only.tsv") and "no strain step" in capfd.readouterr().err
    _profile(eng, db, wr, gaf, species=False, strain=True, strain_em_file=str(wr / "em.tsv"))
    assert open(wr / "em.tsv", "rb").read() == full
    # the command-line front end
    exe = os.path.join(ROOT, "pantax_amd", "lib", "pantax-hip")
    wc = root / "wd_em_cli"
    wc.mkdir()
    r = subprocess.run([exe, "-db", str(db), "-T", str(wc), "--gaf", str(gaf), "--species", "--strain", "--short-read", "--sample", "0",
                        "--strain-em", str(wc / "em.tsv")], cwd=str(wc), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(wc / "em.tsv", "rb").read() == full
    # several ranks: refused on every rank with the table's wording, before any collective
    for rank in range(2):
        wn = root / ("wd_em_ranks_%d" % rank)
        with pytest.raises(PantaxHipError) as e:
            _profile(eng, db, wn, gaf, rank=rank, world_size=2, allreduce=lambda buf: None, strain_em_file=str(wn / "em.tsv"))
        assert e.value.code == -1 and "the read class report (strain_em_file) needs one rank and an unsharded ingest (world_size 2)" in str(e.value)
        assert not os.path.exists(wn / "em.tsv")
    # a caller compiled against the header before these fields: its struct ends behind strain_addin_top, the report reads as off
    real = _ffi.ProfileExt

    class OldExt(real):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.struct_size = 64

    monkeypatch.setattr(_ffi, "ProfileExt", OldExt)
    wold = root / "wd_em_old"
    _profile(eng, db, wold, gaf, strain_fit_file=str(wold / "fit.tsv"), strain_em_file=str(wold / "em.tsv"))
    monkeypatch.setattr(_ffi, "ProfileExt", real)
    assert os.path.exists(wold / "fit.tsv") and not os.path.exists(wold / "em.tsv")
    assert open(wold / "strain_abundance.txt", "rb").read() == open(wd / "strain_abundance.txt", "rb").read()


def test_profile_seam_read_em_skips_a_species_of_65_rows(tmp_path_factory):
    """a species with more rows in strain_abundance.txt than a class mask has bits prints `skipped`: counted, no classes, no estimate; the species beside
    it is served (the inputs of test_profile_seam_addin_skips_a_species_of_65_rows)"""
    import synthdata as synth
    from pantax_amd.engine import Engine
    rng = np.random.default_rng(944)
    wide = synth.make_species(rng, "7000", 100, 30000, 1, "GCF_W", present_frac=1.0)
    small = synth.make_species(rng, "7001", 3, 8000, wide.range_end + 1, "GCF_S", present_frac=1.0)
    sset = synth.SyntheticSet([wide, small], synth.make_reads(rng, [wide, small], 60000, adversarial_frac=0.0, with_ids=True))
    root = tmp_path_factory.mktemp("pantax_em_wide")
    db = root / "db"
    db.mkdir()
    synth.write_db(sset, str(db))
    gaf = root / "gfa_mapped.gaf"
    synth.write_gaf(sset.reads, str(gaf))
    eng = Engine(0)
    try:
        wd = root / "wd"
        _profile(eng, db, wd, gaf, fr=0.0, fc=1e9, sd=1e9, strain_em_file=str(wd / "em.tsv"))
    finally:
        eng.close()
    table = _lines(wd / "strain_abundance.txt")[1:]
    n_wide = sum(1 for t in table if t[0] == "7000")
    print("rows of the wide species in the strain table: %d" % n_wide)
    assert n_wide >= 65
    rows = _lines(wd / "em.tsv")
    assert rows[0] == HEADER and all(len(r) == len(HEADER) for r in rows)
    strain = [r for r in rows[1:] if r[3] == "strain"]
    assert [r[:3] for r in strain] == [t[:3] for t in table]
    for r in strain:
        if r[0] == "7000":                                                   # len and predicted_coverage alone
            assert r[7:11] == ["-"] * 4 and int(r[11]) > 0 and r[12:15] == ["-"] * 3 and float(r[15]) >= 0
        else:
            assert int(r[7]) > 0 and int(r[11]) > 0 and float(r[12]) > 0 and 0 < float(r[14]) <= 1
    assert not any(r[0] == "7000" and r[3] in ("read_class", "other") for r in rows[1:])
    by = {(r[0], r[3]): r for r in rows[1:] if r[3] in ("species", "skipped", "unexplained")}
    assert ("7000", "species") not in by and int(by[("7000", "skipped")][7]) > 1000 and by[("7000", "skipped")][16:] == ["-"] * 4
    assert by[("7000", "unexplained")][7:10] == ["0", "0", "0"]
    sp = by[("7001", "species")]
    assert int(sp[7]) > 0 and int(sp[16]) >= 1 and int(sp[17]) >= 1 and sp[18] in ("0", "1") and float(sp[19]) >= 0
    assert sum(int(r[7]) for r in rows[1:] if r[0] == "7001" and r[3] in ("read_class", "other", "unexplained")) == int(sp[7])
