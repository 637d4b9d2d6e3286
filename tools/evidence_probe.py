#!/usr/bin/env python3
"""Measurement: the per-strain node evidence (pantax_hip_strain_evidence) on a bench workload.  Builds the set as bench.py does, runs one
resident step, selects its rows (the a15 pass bits: the strains of strain_abundance.txt), runs the coverage pass as a stage call and times
the node pass through timing_get: ms, algorithmic bytes and the fraction of 8 TB/s.  With route "walk" the membership comes from the selected
walks (evidence_route=walk): the mask pass is timed too.
usage: evidence_probe.py [workload (cfg4)] [repeats (3)] [route (node | walk)] [record.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from pantax_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3
route = sys.argv[3] if len(sys.argv) > 3 else "node"
record = sys.argv[4] if len(sys.argv) > 4 else None
spec = bench.workload_spec(name)
t0 = time.perf_counter()
ns = bench.native_set(spec, threads=min(16, os.cpu_count() or 1))
rd = ns.reads()
species = ns.graphs()
avg = ns.avg_len()
print("%s: %d species, %d reads, %d steps, generated in %.1f s" % (name, len(species), rd.n_reads, len(rd.node_id), time.perf_counter() - t0), flush=True)
eng = Engine(0)
eng.upload_db(species)
eng.upload_packed(rd)
fr = 0.5 if spec.get("long_reads") else 0.3
keep, absolute, met, info, passed, _, _ = eng.profile_step(avg, fr=fr)
hap_off = eng.hap_off.astype(np.int64)
sel_off, sel_hap, p_sel = [0], [], 0
for s, g in enumerate(species):
    for h in range(hap_off[s], hap_off[s + 1]):
        if passed[h]:
            k = int(h - hap_off[s])
            sel_hap.append(k)
            p_sel += int(g.path_off[k + 1]) - int(g.path_off[k])
    sel_off.append(len(sel_hap))
sel = (np.array(sel_off, dtype=np.uint64), np.array(sel_hap, dtype=np.uint32))
V = int(eng.node_off[-1])
print("selected: %d strains over %d species, %d nodes, %d path steps of the selected walks" % (len(sel_hap), eng.S, V, p_sel), flush=True)
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
if route == "walk":
    eng.set_option("evidence_route", "walk")
out = eng.strain_evidence(sel[0], sel[1])            # warm-up
eng.timing_enable(True)
eng.timing_reset()
t0 = time.perf_counter()
for _ in range(N):
    out = eng.strain_evidence(sel[0], sel[1])
wall = (time.perf_counter() - t0) / N
rows = eng.timing_get()
eng.timing_enable(False)
eng.set_option("evidence_route", None)
per = lambda k: rows.get(k, (0, 0.0))[1] / max(rows.get(k, (0, 0.0))[0], 1)
ms_node, ms_mask = per("evidence_node_kernel"), per("read_strain_mask_kernel")
C, S = len(sel_hap), eng.S
b_node = 24 * V + 64 * C + 96 * S                    # len 4 + cov 4 + bases 8 + membership word 8 per node; the two output blocks
hap, sp = out
res = {"workload": name, "route": route, "strains": C, "species": S, "nodes": V, "call_ms_wall": wall * 1e3,
       "evidence_node_kernel_ms": ms_node, "evidence_node_kernel_gb": b_node / 1e9, "evidence_node_kernel_of_8TBs": b_node / ms_node / 1e6 / 8000 if ms_node else None,
       "read_strain_mask_kernel_ms": ms_mask if route == "walk" else None, "selected_path_steps": p_sel,
       "private_nodes": int(hap[:, 1, 0].sum()), "core_nodes": int(sp[:, 2, 0].sum()), "orphan_nodes": int(sp[:, 1, 0].sum()),
       "orphan_bases": int(sp[:, 1, 3].sum()), "total_bases": int(sp[:, 0, 3].sum())}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
