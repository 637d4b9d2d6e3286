#!/usr/bin/env python3
"""Measurement: the per-strain windowed coverage track (pantax_hip_strain_cov_track) on a bench workload.  Builds the set as bench.py does,
runs one resident step, selects its rows (the a15 pass bits: the strains of strain_abundance.txt), runs the coverage pass as a stage call
and times the two kernels of the track through timing_get: ms, algorithmic bytes and the fraction of 8 TB/s.
usage: cov_track_probe.py [workload (cfg4)] [repeats (3)] [window (10000)] [record.json]"""
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
W = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
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
h_all = 0
for s, g in enumerate(species):
    for h in range(hap_off[s], hap_off[s + 1]):
        if passed[h]:
            k = int(h - hap_off[s])
            sel_hap.append(k)
            p_sel += int(g.path_off[k + 1]) - int(g.path_off[k])
    sel_off.append(len(sel_hap))
sel = (np.array(sel_off, dtype=np.uint64), np.array(sel_hap, dtype=np.uint32))
print("selected: %d strains over %d species, %d path steps" % (len(sel_hap), eng.S, p_sel), flush=True)
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
out = eng.strain_cov_track(sel[0], sel[1], W)        # warm-up
eng.timing_enable(True)
eng.timing_reset()
t0 = time.perf_counter()
for _ in range(N):
    out = eng.strain_cov_track(sel[0], sel[1], W)
wall = (time.perf_counter() - t0) / N
rows = eng.timing_get()
eng.timing_enable(False)
n_win = len(out[1])
# Engine.strain_cov_track makes two calls (sizing, then the arrays): the length pass runs twice a repeat, the accumulation once
ms_len = rows.get("cov_track_len_kernel", (0, 0.0))
ms_len = ms_len[1] / max(ms_len[0], 1)
ms_acc = rows.get("cov_track_accum_kernel", (0, 0.0))
ms_acc = ms_acc[1] / max(ms_acc[0], 1)
b_len = 8 * p_sel
b_acc = 20 * p_sel + 28 * n_win
res = {"workload": name, "window": W, "strains": len(sel_hap), "path_steps": p_sel, "windows": n_win, "call_ms_wall": wall * 1e3,
       "cov_track_len_kernel_ms": ms_len, "cov_track_len_kernel_gb": b_len / 1e9, "cov_track_len_kernel_of_8TBs": b_len / ms_len / 1e6 / 8000 if ms_len else None,
       "cov_track_accum_kernel_ms": ms_acc, "cov_track_accum_kernel_gb": b_acc / 1e9, "cov_track_accum_kernel_of_8TBs": b_acc / ms_acc / 1e6 / 8000 if ms_acc else None,
       "windows_with_nodes": int((out[1] > 0).sum()), "sum_len": int(out[2].sum()), "sum_bases": int(out[4].sum())}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
