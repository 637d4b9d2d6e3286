"""The LPs whose pivots are pinned in tests/golden/lad_pivots.npz (tools/record_lad_pivots.py writes it, tests/test_gpu_lad_pivots.py compares with it):
the smallest cases that reach every body of the LAD solver (stage_lad.hip / lad_solver.hpp) -- the <= 16-column instance with LDS and with global-scratch
pattern state, the 64-column instance (line-search cache in G), the four-word and the run-time-word instances -- grouped so that one pao_solve_batch
call solves a group.  x is recorded as raw uint64 bit patterns: the solver promises the same bits under every shape, and the file extends that to
"the same as when the file was recorded"."""
import json
import os

import numpy as np

from tests.test_gpu_lad_shapes import STEP_SET, _crafted, _random_lp, _tie_plateau_lp

GOLDEN = "lad_pivots.npz"
# which solver instance a group's batch runs on (the widest species decides between the 16- and the 64-column instance; wide and huge species of a
# batch go to their own launches beside it)
GROUPS = ("crafted16", "cols64", "golden16", "golden64", "golden_wide", "golden_huge", "mixed")
FAMILY = {"crafted16": "16", "cols64": "64", "golden16": "16", "golden64": "64", "golden_wide": "wide", "golden_huge": "huge"}


def paths_from_masks(mask, p):
    """mask: (n,) uint64, or (n, nw) words for more than 64 columns -> (path_off, path_nodes)"""
    m2 = np.asarray(mask, dtype=np.uint64).reshape(len(mask), -1)
    offs, nodes = [0], []
    for k in range(p):
        sel = np.nonzero((m2[:, k >> 6] >> np.uint64(k & 63)) & np.uint64(1))[0]
        nodes.append(sel.astype(np.uint32))
        offs.append(offs[-1] + len(sel))
    return np.array(offs, dtype=np.uint64), (np.concatenate(nodes) if nodes else np.zeros(0, dtype=np.uint32))


def _lp(mask, a, p, fixed=None):
    return dict(mask=np.asarray(mask, dtype=np.uint64), a=np.asarray(a, dtype=np.float64), p=int(p),
                fixed=np.zeros(p, dtype=np.uint8) if fixed is None else np.asarray(fixed, dtype=np.uint8))


def _tie_plateau_20():
    """the tie plateau of 3 000 rows (three columns) with seventeen more columns of five rows each: 20 columns, the 64-column instance"""
    lp = _tie_plateau_lp(20000, 3000)
    rng = np.random.default_rng(3020)
    mask, a = [lp["mask"]], [lp["a"]]
    for k in range(3, 20):
        mask.append(np.full(5, 1 << k, dtype=np.uint64))
        a.append(rng.integers(1, 40, 5).astype(np.float64))
    return _lp(np.concatenate(mask), np.concatenate(a), 20)


def _random_lp_64(seed, n, n_pat):
    """_random_lp at 64 columns: its pattern draw (integers below 1 << p) does not fit numpy's int64 there, so the patterns are drawn as uint64 words"""
    p = 64
    rng = np.random.default_rng(seed)
    pats = {1 << k for k in range(min(p, n_pat))}
    while len(pats) < n_pat:
        pats.add(int(rng.integers(1, 2 ** 64 - 1, dtype=np.uint64, endpoint=True)))
    pats = np.array(sorted(pats), dtype=np.uint64)
    mask = np.concatenate([pats, pats[rng.integers(0, n_pat, n - n_pat)]])
    truth = np.where(rng.random(p) < 0.6, rng.integers(2, 30, p), 0).astype(np.float64)
    A = np.stack([((mask >> np.uint64(k)) & np.uint64(1)).astype(np.float64) for k in range(p)], 1)
    return dict(mask=mask, a=np.maximum(np.rint(A @ truth + rng.normal(0, 2.0, n)), 1.0), p=p)


def generated_cases():
    """group -> [(name, lp)]: the LPs made here (the oracle solves every one of them; test_generated_cases_are_solved)"""
    g = {"crafted16": [(n, _lp(lp["mask"], lp["a"], lp["p"], lp["fixed"])) for n, lp in _crafted().items()], "cols64": []}
    for p in (17, 40, 64):
        for n_pat in (12, 100, 257):      # cooperative searches and wide rounds / a thread per pattern / the global-scratch body
            lp = _random_lp(6400 + 10 * p + n_pat, 3000, p, n_pat) if p < 64 else _random_lp_64(6400 + 10 * p + n_pat, 3000, n_pat)
            g["cols64"].append(("p%d_pat%d" % (p, n_pat), _lp(lp["mask"], lp["a"], p)))
    g["cols64"].append(("tie_3000_p20", _tie_plateau_20()))
    return g


def _golden_file(golden_dir, stem):
    z = np.load(os.path.join(golden_dir, stem + ".npz"))
    out = []
    for i in range(int(z["n_cases"])):
        mask, a = z["mask_%d" % i], z["a_%d" % i]
        fixed = z["fixed_%d" % i] if "fixed_%d" % i in z.files else (z["ub_%d" % i] == 0)
        out.append(("%s_%d" % (stem, i), _lp(mask, a, len(fixed), np.asarray(fixed).astype(np.uint8))))
    return out


def all_cases(golden_dir):
    """group -> [(name, lp)], every group of GROUPS"""
    g = generated_cases()
    small = _golden_file(golden_dir, "lp_cases") + _golden_file(golden_dir, "lp_milp_cases")
    g["golden16"] = [c for c in small if c[1]["p"] <= 16]      # a batch runs on the instance of its widest species
    g["golden64"] = [c for c in small if c[1]["p"] > 16]
    g["golden_wide"] = _golden_file(golden_dir, "lp_wide_cases") + _golden_file(golden_dir, "lp_wide_unique_cases")
    g["golden_huge"] = _golden_file(golden_dir, "lp_huge_cases")
    # one batch with a species for every launch of the ladder, and one without candidates (lad_instance_takes, the need / skip paths)
    g["mixed"] = [g["crafted16"][0], g["cols64"][0], g["golden_wide"][0], g["golden_huge"][0]]
    return g


def solve_group(eng, lps, no_candidates=True):
    """one pao_solve_batch call -> dict(x_bits, x_off, status, iters, obj) over the LPs (the species without candidates is checked and dropped)"""
    species, fixed = [], []
    for _, lp in lps:
        po, pn = paths_from_masks(lp["mask"], lp["p"])
        species.append((np.ones(len(lp["a"]), dtype=np.int64), lp["a"], None, po, pn, np.arange(lp["p"], dtype=np.uint32)))
        fixed.append(lp["fixed"])
    if no_candidates:
        po, pn = paths_from_masks(np.array([1, 3, 2], dtype=np.uint64), 2)
        species.append((np.ones(3, dtype=np.int64), np.array([1.0, 2.0, 3.0]), None, po, pn, np.zeros(0, dtype=np.uint32)))
        fixed.append(np.zeros(0, dtype=np.uint8))
    res = eng.pao_solve_batch(species, fixed)
    if no_candidates:
        assert res[-1][3] == 0 and len(res[-1][0]) == 0 and res[-1][4] == 0
        res = res[:-1]
    x = np.concatenate([r[0] for r in res]).astype(np.float64)
    return dict(x_bits=np.ascontiguousarray(x).view(np.uint64), x_off=np.cumsum([0] + [len(r[0]) for r in res]).astype(np.int64),
                status=np.array([r[3] for r in res], dtype=np.int32), iters=np.array([r[4] for r in res], dtype=np.int32),
                obj=np.array([r[2] for r in res], dtype=np.float64))


def run_step(eng):
    """the resident step of STEP_SET (both solves in lad_pair_kernel) -> what test_resident_step_same_under_every_option_value compares"""
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
    eng.upload_db(species)
    eng.upload_packed(sset.reads)
    return profile_step(eng, [g.name for g in species], [h for g in species for h in g.hap_names], np.array(sset.avg_len(), dtype=np.float64), StepConfig())


def to_json(obj):
    """a step's (species rows, strain rows, stats) as text: floats round-trip exactly through their repr"""
    def plain(o):
        if isinstance(o, dict):
            return {str(k): plain(v) for k, v in o.items()}
        if isinstance(o, np.ndarray):
            return {"__nd__": str(o.dtype), "shape": list(o.shape), "data": o.ravel().tolist()}
        if isinstance(o, (list, tuple)):
            return [plain(v) for v in o]
        if isinstance(o, np.generic):
            return o.item()
        return o
    return json.dumps(plain(obj))


def from_json(text):
    def back(o):
        if isinstance(o, dict):
            if "__nd__" in o:
                return np.array(o["data"], dtype=o["__nd__"]).reshape(o["shape"])
            return {k: back(v) for k, v in o.items()}
        if isinstance(o, list):
            return [back(v) for v in o]
        return o
    return back(json.loads(text))
