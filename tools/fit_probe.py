#!/usr/bin/env python3
"""Measurement: the model fit per strain (pantax_hip_strain_fit) beside the node evidence (pantax_hip_strain_evidence) in one process, on the same
resident coverage result and the same selection.  Two sets: "long" is the long-read set of tests/test_gpu_fit.py (synthdata.make_set(925, 2, 6, 400,
300000, long_reads=True), a hand-picked selection); any other name is a bench workload built as bench.py builds it, one resident step, its rows (the a15
pass bits) as the selection with their second_sol as weights.  The two calls alternate behind a warm-up call each; the node passes are timed through
timing_get: ms a launch, algorithmic bytes and the fraction of 8 TB/s.
usage: fit_probe.py [set (long | cfg4_share | ...)] [repeats (5)] [route (node | walk)] [record.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from pantax_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "long"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 5
route = sys.argv[3] if len(sys.argv) > 3 else "node"
record = sys.argv[4] if len(sys.argv) > 4 else None
eng = Engine(0)
t0 = time.perf_counter()
if name == "long":
    import synthdata as synth
    sset = synth.make_set(925, 2, 6, 400, 300000, long_reads=True)
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    picks = [[(1, 0.8), (4, 0.05), (2, 1.9)], [(h, 0.4 * (h + 1)) for h in range(6)]]
    sel_off = np.cumsum([0] + [len(p) for p in picks]).astype(np.uint64)
    sel_hap = np.array([h for p in picks for h, _ in p], dtype=np.uint32)
    sel_w = np.array([w for p in picks for _, w in p], dtype=np.float64)
else:
    import bench
    spec = bench.workload_spec(name)
    ns = bench.native_set(spec, threads=min(16, os.cpu_count() or 1))
    rd, species, avg = ns.reads(), ns.graphs(), ns.avg_len()
    eng.upload_db(species)
    eng.upload_packed(rd)
    keep, absolute, met, info, passed, _, _ = eng.profile_step(avg, fr=0.5 if spec.get("long_reads") else 0.3)
    hap_off = eng.hap_off.astype(np.int64)
    off, hp, w = [0], [], []
    for s in range(eng.S):
        for h in range(hap_off[s], hap_off[s + 1]):
            if passed[h]:
                hp.append(int(h - hap_off[s]))
                w.append(float(met[h].second_sol))
        off.append(len(hp))
    sel_off, sel_hap, sel_w = np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32), np.array(w, dtype=np.float64)
V, C, S = int(eng.node_off[-1]), len(sel_hap), eng.S
print("%s: %d species, %d nodes, %d selected strains, set up in %.1f s" % (name, S, V, C, time.perf_counter() - t0), flush=True)
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
if route == "walk":
    eng.set_option("fit_route", "walk")
    eng.set_option("evidence_route", "walk")
fit = eng.strain_fit(sel_off, sel_hap, sel_w)        # warm-up of both
ev = eng.strain_evidence(sel_off, sel_hap)
eng.timing_enable(True)
eng.timing_reset()
wall_fit, wall_ev = [], []
for _ in range(N):                                   # alternating
    t0 = time.perf_counter()
    fit = eng.strain_fit(sel_off, sel_hap, sel_w)
    t1 = time.perf_counter()
    ev = eng.strain_evidence(sel_off, sel_hap)
    wall_fit.append((t1 - t0) * 1e3)
    wall_ev.append((time.perf_counter() - t1) * 1e3)
rows = eng.timing_get()
eng.timing_enable(False)
eng.set_option("fit_route", None)
eng.set_option("evidence_route", None)
per = lambda k: rows.get(k, (0, 0.0))[1] / max(rows.get(k, (0, 0.0))[0], 1)
ms_fit, ms_ev = per("fit_node_kernel"), per("evidence_node_kernel")
b_fit = 20 * V + 128 * C + 192 * S                   # len 4 + bases 8 + membership word 8 per node; the two output blocks
b_ev = 24 * V + 64 * C + 96 * S                      # ... + cov 4
hap, sp = fit
assert np.array_equal(hap[:, :, :3], ev[0][:, :, [0, 1, 3]]) and np.array_equal(sp[:, 0, :3], ev[1][:, 0][:, [0, 1, 3]])
tot = sp[:, 0].sum(axis=0, dtype=np.uint64)
res = {"set": name, "route": route, "strains": C, "species": S, "nodes": V, "repeats": N,
       "fit_node_kernel_ms": ms_fit, "fit_node_kernel_gb": b_fit / 1e9, "fit_node_kernel_of_8TBs": b_fit / ms_fit / 1e6 / 8000 if ms_fit else None,
       "evidence_node_kernel_ms": ms_ev, "evidence_node_kernel_gb": b_ev / 1e9, "evidence_node_kernel_of_8TBs": b_ev / ms_ev / 1e6 / 8000 if ms_ev else None,
       "fit_over_evidence": ms_fit / ms_ev if ms_ev else None, "fit_call_ms_wall": sorted(wall_fit), "evidence_call_ms_wall": sorted(wall_ev),
       "total": {k: int(x) for k, x in zip(("n_nodes", "len", "bases", "expected", "excess", "deficit", "blind_nodes", "blind_expected"), tot)}}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
