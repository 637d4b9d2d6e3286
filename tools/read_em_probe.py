#!/usr/bin/env python3
"""Measurement: the read classes and the read-based estimate (pantax_hip_strain_read_em) on resident reads.  Three sets, those of tools/addin_probe.py:
"long" is the long-read set of tests/test_gpu_fit.py (synthdata.make_set(925, 2, 6, 400, 300000, long_reads=True), haplotypes 0 .. 2 of a species as the
candidates); "mid" is a synthetic short-read set of 16 species of 12 haplotypes (synthdata.make_set(926, 16, 12, 200000, 600000, present_frac=0.6),
haplotypes 0 .. 3); any other name is a bench workload built as bench.py builds it, one resident step, its rows (the a15 pass bits) as the candidates.  G is
the len of the candidate's `all` class of strain_evidence, as in the file seam.  Behind a warm-up call of each, strain_read_support and strain_read_em are
called `runs` times in turn on the same resident reads in the same process; the kernels are timed through timing_get (device events).  The yardstick of
read_class_kernel is read_support_kernel, which reads the same bytes; the record also holds the growth reruns of the class pass (launches of
read_class_kernel beyond the first), the time of read_em_kernel, the largest J of a species and the largest n_iter.
usage: read_em_probe.py [set (long | mid | cfg4_share | ...)] [runs (5)] [read_class_slots (0: default)] [record.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from pantax_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "long"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
slots = int(sys.argv[3]) if len(sys.argv) > 3 else 0
record = sys.argv[4] if len(sys.argv) > 4 else None
eng = Engine(0)
t0 = time.perf_counter()
if name in ("long", "mid"):
    import synthdata as synth
    sset = synth.make_set(925, 2, 6, 400, 300000, long_reads=True) if name == "long" else synth.make_set(926, 16, 12, 200000, 600000, present_frac=0.6)
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    reported = [list(range(3 if name == "long" else 4)) for _ in sset.species]
else:
    import bench
    spec = bench.workload_spec(name)
    ns = bench.native_set(spec, threads=min(16, os.cpu_count() or 1))
    rd, species, avg = ns.reads(), ns.graphs(), ns.avg_len()
    eng.upload_db(species)
    eng.upload_packed(rd)
    fr = 0.5 if spec.get("long_reads") else 0.3
    keep, absolute, met, info, passed, _, _ = eng.profile_step(avg, fr=fr)
    hap_off = eng.hap_off.astype(np.int64)
    reported = [[int(h - hap_off[s]) for h in range(hap_off[s], hap_off[s + 1]) if passed[h]] for s in range(eng.S)]
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind, for G
off = np.concatenate([[0], np.cumsum([len(r) for r in reported])]).astype(np.uint64)
hap = np.array([h for r in reported for h in r], dtype=np.uint32)
G = eng.strain_evidence(off, hap)[0][:, 0, 1].copy()
w = np.ones(len(hap))
print("%s: %d species, %d candidates, set up in %.1f s" % (name, eng.S, len(hap), time.perf_counter() - t0), flush=True)
if slots:
    eng.set_option("read_class_slots", slots)
eng.strain_read_support(off, hap, w)                 # warm-up
eng.strain_read_em(off, hap, G)
SUP = ["read_support_kernel", "read_support_long_kernel"]
CLS = ["read_class_kernel", "read_class_long_kernel"]
ORDER = ["read_class_flag_kernel", "read_class_gather_kernel"]
per_run = []
for _ in range(runs):
    r = {}
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    sup = eng.strain_read_support(off, hap, w)
    r["support_call_ms_wall"] = (time.perf_counter() - t0) * 1e3
    t = eng.timing_get()
    r["read_support"] = sum(t.get(n, (0, 0.0))[1] for n in SUP)
    r["read_support_main"] = t.get(SUP[0], (0, 0.0))[1]
    eng.timing_reset()
    t0 = time.perf_counter()
    species, cls_off, mask, q, x, n_iter, conv, delta = eng.strain_read_em(off, hap, G)
    r["em_call_ms_wall"] = (time.perf_counter() - t0) * 1e3
    t = eng.timing_get()
    eng.timing_enable(False)
    passes = t.get(CLS[0], (0, 0.0))[0]
    r["passes"] = passes
    r["read_class"] = sum(t.get(n, (0, 0.0))[1] for n in CLS)
    r["read_class_main_per_pass"] = t.get(CLS[0], (0, 0.0))[1] / max(passes, 1)
    r["ordering"] = sum(v[1] for n, v in t.items() if n in ORDER or n.startswith("scan"))
    r["read_em"] = t.get("read_em_kernel", (0, 0.0))[1]
    per_run.append(r)
eng.set_option("read_class_slots", None)
assert np.array_equal(species[:, 0], sup[1][:, 0])    # the two calls count the same reads
med = lambda k: float(np.median([r[k] for r in per_run]))
rng_ = lambda k: [float(min(r[k] for r in per_run)), float(max(r[k] for r in per_run))]
keys = [k for k in per_run[0] if k != "passes"]
J = np.diff(cls_off.astype(np.int64))
res = {"set": name, "species": eng.S, "candidates": len(hap), "k_max": int(np.diff(off.astype(np.int64)).max()), "counted_reads": int(species[:, 0, 0].sum()),
       "unexplained_reads": int(species[:, 1, 0].sum()), "classes": int(J.sum()), "j_max": int(J.max()) if len(J) else 0, "largest_class_reads": int(q[:, 0].max()) if len(q) else 0,
       "n_iter_max": int(n_iter.max()) if len(n_iter) else 0, "converged_species": int(conv.sum()), "species_with_classes": int((J > 0).sum()),
       "read_class_slots": slots, "growth_reruns": per_run[0]["passes"] - 1, "runs": runs, "median_ms": {k: med(k) for k in keys}, "range_ms": {k: rng_(k) for k in keys},
       "per_run_ms": per_run,
       "class_over_support_main_kernel": med("read_class_main_per_pass") / med("read_support_main") if med("read_support_main") else None,
       "class_over_support_with_long": med("read_class") / med("read_support") if med("read_support") else None}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
