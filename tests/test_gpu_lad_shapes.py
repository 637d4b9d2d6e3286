"""The LDS shapes of the <= 16-column LAD solver (stage_lad.hip LadRoomy / LadCompact, option lad_shape): the shape sizes the row index, the cache of a
line search's candidate rows and the number of patterns whose state lives in LDS -- it decides how many solver workgroups share a CU and nothing about the
result.  Every case here runs under lad_shape=roomy and lad_shape=compact: x, status and iterations equal bit for bit, objectives equal to the stored HiGHS
value (golden LPs) or the oracle's (crafted LPs) to 1e-9 relative; a small resident step gives the same tables and stats under auto / roomy / compact, and
the host rule (Engine.lad_shape_name) takes the roomy shape for fewer species than the device has CUs."""
import os

import numpy as np
import pytest

SHAPES = ("roomy", "compact")
# the sizes the crafted LPs straddle (stage_lad.hip): samples of the row index / patterns with LDS state of the two shapes, cached candidate rows, LAD_KWIDE
IDX_N = {"roomy": 4096, "compact": 1024}
KLDS = {"roomy": 256, "compact": 32}
CACHE_N = {"roomy": 2048, "compact": 1024}
KWIDE = 16


def _paths_from_masks(mask, p):
    offs, nodes = [0], []
    for k in range(p):
        sel = np.nonzero((mask >> np.uint64(k)) & np.uint64(1))[0]
        nodes.append(sel.astype(np.uint32))
        offs.append(offs[-1] + len(sel))
    return np.array(offs, dtype=np.uint64), (np.concatenate(nodes) if nodes else np.zeros(0, dtype=np.uint32))


def _species(mask, a, p):
    po, pn = _paths_from_masks(mask, p)
    return (np.ones(len(a), dtype=np.int64), np.asarray(a, dtype=np.float64), None, po, pn, np.arange(p, dtype=np.uint32))


def _random_lp(seed, n, p, n_pat, fixed=()):
    """n rows over n_pat distinct membership patterns of p columns, integer abundances (massive ties) around a sparse truth"""
    rng = np.random.default_rng(seed)
    pats = set()
    for k in range(min(p, n_pat)):
        pats.add(1 << k)                          # every column has a row of its own: no free column
    while len(pats) < n_pat:
        pats.add(int(rng.integers(1, 1 << p)))
    pats = np.array(sorted(pats), dtype=np.uint64)
    assert len(pats) == n_pat and n >= n_pat
    mask = np.concatenate([pats, pats[rng.integers(0, n_pat, n - n_pat)]])
    truth = np.where(rng.random(p) < 0.6, rng.integers(2, 30, p), 0).astype(np.float64)
    A = np.stack([((mask >> np.uint64(k)) & np.uint64(1)).astype(np.float64) for k in range(p)], 1)
    a = np.maximum(np.rint(A @ truth + rng.normal(0, 2.0, n)), 1.0)
    fz = np.zeros(p, dtype=np.uint8)
    fz[list(fixed)] = 1
    return dict(mask=mask, a=a, p=p, fixed=fz, separable=False)


def _separable_lp(seed, counts):
    """column k only in the pattern {k}, an odd number of rows with an unrepeated middle value: the optimum is the single point x_k = median_k"""
    rng = np.random.default_rng(seed)
    mask, a = [], []
    for k, n in enumerate(counts):
        assert n % 2 == 1
        v = np.sort(rng.integers(1, 40, n)).astype(np.float64)
        v[n // 2 + 1:] += 1.0
        v[n // 2:] += 1.0                          # strictly between its neighbours
        mask.append(np.full(n, 1 << k, dtype=np.uint64)); a.append(rng.permutation(v))
    return dict(mask=np.concatenate(mask), a=np.concatenate(a), p=len(counts), fixed=np.zeros(len(counts), dtype=np.uint8), separable=True)


def _tie_plateau_lp(n, tie):
    """Three columns, four patterns, n rows; `tie` rows of the heaviest pattern share the value its weighted median falls on, so the sample-only rounds of
    the line search (every sample inside the plateau is the same number) leave about `tie` candidates for the exact rounds"""
    rng = np.random.default_rng(tie)
    n0 = n // 2
    side = (n0 - tie) // 2
    a0 = np.concatenate([rng.integers(1, 20, side), np.full(tie, 20), rng.integers(21, 40, n0 - tie - side)]).astype(np.float64)
    rest = n - n0
    m_rest = np.array([2, 4, 6], dtype=np.uint64)[rng.integers(0, 3, rest)]
    a_rest = np.where(m_rest == 2, rng.integers(3, 9, rest), np.where(m_rest == 4, rng.integers(10, 16, rest), rng.integers(14, 24, rest))).astype(np.float64)
    return dict(mask=np.concatenate([np.full(n0, 1, dtype=np.uint64), m_rest]), a=np.concatenate([a0, a_rest]), p=3, fixed=np.zeros(3, dtype=np.uint8),
                separable=False)


def _crafted():
    c = {}
    for shape in SHAPES:                                        # patterns at the LDS capacity of each shape and one above it (global-scratch body)
        c["pat_%d" % KLDS[shape]] = _random_lp(100 + KLDS[shape], 3000, 10, KLDS[shape])
        c["pat_%d" % (KLDS[shape] + 1)] = _random_lp(101 + KLDS[shape], 3000, 10, KLDS[shape] + 1)
    c["pat_64"] = _random_lp(164, 3000, 9, 64)                  # between the two capacities
    c["pat_65"] = _random_lp(165, 3000, 9, 65)
    c["pat_kwide"] = _random_lp(16, 2500, 8, KWIDE)             # cooperative searches and wide rounds ...
    c["pat_kwide+1"] = _random_lp(17, 2500, 8, KWIDE + 1)       # ... and one above: a thread per pattern
    for shape in SHAPES:                                        # rows at the index size (stride 1) and one more (stride 2)
        c["rows_%d" % IDX_N[shape]] = _random_lp(200 + IDX_N[shape], IDX_N[shape], 6, 9)
        c["rows_%d" % (IDX_N[shape] + 1)] = _random_lp(201 + IDX_N[shape], IDX_N[shape] + 1, 6, 9)
    c["rows_20000"] = _random_lp(20000, 20000, 10, 12)          # a stride of 8 (roomy) / 32 (compact) rows
    c["rows_20000_16col"] = _random_lp(20016, 20000, 16, 40)    # every column of the instance in use
    c["rows_37"] = _random_lp(37, 37, 3, 5)                     # fewer rows than a wave
    c["separable_3"] = _separable_lp(3, [41, 1501, 6001])
    assert CACHE_N["compact"] < 1500 < CACHE_N["roomy"]
    c["tie_1500"] = _tie_plateau_lp(20000, 1500)                # candidates beyond the compact cache, inside the roomy one
    c["tie_3000"] = _tie_plateau_lp(20000, 3000)                # beyond both
    c["pinned"] = _random_lp(77, 3000, 8, 20, fixed=(1, 4))     # fixed_zero columns
    c["pinned_all"] = _random_lp(78, 500, 3, 5, fixed=(0, 1, 2))
    return c


@pytest.fixture(scope="module")
def crafted():
    """name -> LP, with the oracle's solution: made once, shared, never changed"""
    from oracle import oracle as orc
    cases = _crafted()
    for name, lp in cases.items():
        ub = np.where(lp["fixed"] == 1, 0.0, 1.05 * lp["a"].max())
        lp["x_o"], lp["obj_o"], _, lp["st_o"] = orc.lad_solve(lp["mask"], lp["a"], lp["p"], ub)
        lp["ub"] = ub
    return cases


def test_crafted_lps_are_what_the_cases_need(crafted):
    """CPU only: the oracle solves every crafted LP, the sizes sit where they should, the separable optimum is the medians"""
    for name, lp in crafted.items():
        assert lp["st_o"] == 0, name
        assert lp["p"] <= 16 and lp["mask"].min() >= 1 and lp["a"].min() >= 1.0 and np.array_equal(lp["a"], np.rint(lp["a"])), name
    npat = lambda n: len(np.unique(crafted[n]["mask"]))
    assert [npat("pat_%d" % k) for k in (32, 33, 64, 65, 256, 257)] == [32, 33, 64, 65, 256, 257]
    assert npat("pat_kwide") == KWIDE and npat("pat_kwide+1") == KWIDE + 1
    assert [len(crafted["rows_%d" % n]["a"]) for n in (1024, 1025, 4096, 4097, 20000, 37)] == [1024, 1025, 4096, 4097, 20000, 37]
    sep = crafted["separable_3"]
    med = [np.median(sep["a"][sep["mask"] == np.uint64(1 << k)]) for k in range(3)]
    assert np.allclose(sep["x_o"], med, rtol=0, atol=1e-9)
    tie = crafted["tie_1500"]
    a0 = np.sort(tie["a"][tie["mask"] == 1])
    assert (a0 == 20).sum() == 1500 and a0[len(a0) // 2] == 20


@pytest.fixture(scope="module")
def eng():
    from pantax_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _solve_under_shapes(eng, set_opt, species, fixed):
    out = {}
    for shape in SHAPES:
        set_opt(eng, "lad_shape", shape)
        out[shape] = eng.pao_solve_batch(species, fixed)
    for i, (r, c) in enumerate(zip(out["roomy"], out["compact"])):
        print("LP %d: status %d/%d iterations %d/%d objective %.17g/%.17g" % (i, r[3], c[3], r[4], c[4], r[2], c[2]))
        assert r[3] == c[3] and r[4] == c[4], i                                  # status, iterations
        assert np.array_equal(r[0], c[0]), (i, r[0], c[0])                       # x: the same bits
        assert r[2] == c[2], i                                                   # the objective is summed from x outside the solver: the same bits too
    return out["roomy"]


@pytest.mark.gpu
def test_golden_lps_under_both_shapes(eng, set_opt, golden_dir):
    z = np.load(os.path.join(golden_dir, "lp_cases.npz"))
    for i in range(int(z["n_cases"])):
        mask, a, ub, objh = z["mask_%d" % i], z["a_%d" % i], z["ub_%d" % i], float(z["obj_%d" % i])
        (x, ratio, obj, st, it), = _solve_under_shapes(eng, set_opt, [_species(mask, a, len(ub))], [(ub == 0).astype(np.uint8)])
        assert st == 0 and obj == pytest.approx(objh, rel=1e-9, abs=1e-12), i
    z = np.load(os.path.join(golden_dir, "lp_milp_cases.npz"))
    for i in range(int(z["n_cases"])):
        mask, a, fixed, objm = z["mask_%d" % i], z["a_%d" % i], z["fixed_%d" % i], float(z["obj_milp_%d" % i])
        (x, ratio, obj, st, it), = _solve_under_shapes(eng, set_opt, [_species(mask, a, len(fixed))], [fixed.astype(np.uint8)])
        assert st == 0 and obj == pytest.approx(objm, rel=1e-9, abs=1e-12), str(z["name_%d" % i])
        assert np.all(x[fixed == 1] == 0.0)


@pytest.mark.gpu
def test_crafted_lps_under_both_shapes(eng, set_opt, crafted):
    """one batch of all crafted LPs plus a species without candidates; the batch has fewer species than a device has CUs, so only the option decides"""
    from oracle import oracle as orc
    names = list(crafted)
    species = [_species(crafted[n]["mask"], crafted[n]["a"], crafted[n]["p"]) for n in names]
    fixed = [crafted[n]["fixed"] for n in names]
    po, pn = _paths_from_masks(np.array([1, 3, 2], dtype=np.uint64), 2)
    species.append((np.ones(3, dtype=np.int64), np.array([1.0, 2.0, 3.0]), None, po, pn, np.zeros(0, dtype=np.uint32)))      # no candidates
    fixed.append(np.zeros(0, dtype=np.uint8))
    assert eng.lad_shape_name(len(species), 16) == "roomy"                       # (option at its default here: auto)
    res = _solve_under_shapes(eng, set_opt, species, fixed)
    assert res[-1][3] == 0 and len(res[-1][0]) == 0 and res[-1][4] == 0
    for n, (x, ratio, obj, st, it) in zip(names, res):
        lp = crafted[n]
        assert st == 0, n
        assert obj == pytest.approx(lp["obj_o"], rel=1e-9), n
        assert orc.lad_objective(lp["mask"], lp["a"], x) == pytest.approx(lp["obj_o"], rel=1e-9), n
        assert np.all(x >= 0.0) and np.all(x <= lp["ub"]) and np.all(x[lp["fixed"] == 1] == 0.0), n
        if lp["separable"]:
            assert np.abs(x - lp["x_o"]).sum() <= 1e-6 * max(1.0, np.abs(lp["x_o"]).sum()), (n, x, lp["x_o"])
    assert max(r[4] for r in res) > 3                                            # (the solver pivoted)


# (haplotypes, genome length[, fraction of the strains present]): a few species of 3-10 strains -- the 16-column instance, fewer species than CUs
STEP_SET = (20261101, [(5, 90000), (4, 70000), (3, 40000), (10, 120000, 0.7), (6, 66000), (8, 80000, 0.5)], 90000)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.gpu
def test_resident_step_same_under_every_option_value(eng, set_opt):
    import synthdata as synth
    from pantax_amd.pipeline import StepConfig, profile_step
    seed, spec, n_reads = STEP_SET
    rng = np.random.default_rng(seed)
    species, start = [], 1
    for s, (h, gl, *pf) in enumerate(spec):
        g = synth.make_species(rng, str(2000 + s), h, gl, start, "GCF_%06d" % (s + 1), present_frac=pf[0] if pf else 0.4)
        species.append(g)
        start = g.range_end + 1
    sset = synth.SyntheticSet(species, synth.make_reads(rng, species, n_reads))
    avg = np.array(sset.avg_len(), dtype=np.float64)
    names = [g.name for g in species]
    haps = [h for g in species for h in g.hap_names]
    S, pmax = len(species), max(g.n_paths for g in species)
    assert pmax <= 16
    eng.upload_db(species)
    eng.upload_packed(sset.reads)
    out = {}
    for value, expect in ((None, "roomy"), ("auto", "roomy"), ("roomy", "roomy"), ("compact", "compact")):
        set_opt(eng, "lad_shape", value)
        assert eng.lad_shape_name(S, pmax) == expect                             # fewer species than CUs: auto takes the roomy shape
        assert eng.lad_shape_name(S, 17) == "roomy"                              # the 64-column instance has one shape
        assert eng.lad_shape_name(100000, pmax) == ("roomy" if value == "roomy" else "compact")   # more species than any device has CUs
        eng.timing_enable(True)
        eng.timing_reset()
        try:
            out[value] = profile_step(eng, names, haps, avg, StepConfig())
            ran = set(eng.timing_get())
        finally:
            eng.timing_enable(False)
        assert "lad_pair_kernel" in ran                                          # the label does not change with the shape
    sp0, st0, stats0 = out[None]
    assert len(st0) > 3 and max(max(i) for i in stats0["iters"]) > 3             # strains were reported and the LPs pivoted
    for value in ("auto", "roomy", "compact"):
        sp, st, stats = out[value]
        assert _same(sp, sp0) and _same(st, st0), value
        assert _same(stats, stats0), value


@pytest.mark.gpu
def test_unknown_shape_is_an_error(eng, set_opt):
    from pantax_amd._ffi import PantaxHipError
    lp = _random_lp(5, 200, 3, 5)
    set_opt(eng, "lad_shape", "tiny")
    with pytest.raises(PantaxHipError, match="lad_shape"):
        eng.pao_solve_batch([_species(lp["mask"], lp["a"], lp["p"])], [lp["fixed"]])
