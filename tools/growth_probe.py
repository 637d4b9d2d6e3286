#!/usr/bin/env python3
"""Measurement: the own-node windows of the replication index report (pantax_hip_strain_growth) on a bench workload.  Builds the set as bench.py does,
runs one resident step, selects its rows (the a15 pass bits: the strains of strain_abundance.txt), runs the coverage pass as a stage call and times the
kernels of the call through timing_get: ms, algorithmic bytes and the fraction of 8 TB/s.  With route "walk" the membership comes from the selected
walks (growth_route=walk): the mask pass is timed too.  The fit of every strain (growth_fit, host) is timed as wall time and its statuses are counted.
usage: growth_probe.py [workload (cfg4)] [repeats (3)] [window (5000)] [route (node|walk)] [record.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from pantax_amd.engine import Engine, growth_fit

name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3
W = int(sys.argv[3]) if len(sys.argv) > 3 else 5000
route = sys.argv[4] if len(sys.argv) > 4 else "node"
record = sys.argv[5] if len(sys.argv) > 5 else None
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
sel_off, sel_hap, p_sel, words = [0], [], 0, 0
for s, g in enumerate(species):
    k_s = 0
    for h in range(hap_off[s], hap_off[s + 1]):
        if passed[h]:
            k = int(h - hap_off[s])
            sel_hap.append(k)
            p_sel += int(g.path_off[k + 1]) - int(g.path_off[k])
            k_s += 1
    sel_off.append(len(sel_hap))
    nw = (k_s + 63) // 64 if (route == "walk" or g.n_paths > 64) else (1 if k_s else 0)   # membership words per node of the species
    words += nw * sum(int(g.path_off[k + 1]) - int(g.path_off[k]) for k in sel_hap[sel_off[-2]:])
sel = (np.array(sel_off, dtype=np.uint64), np.array(sel_hap, dtype=np.uint32))
print("selected: %d strains over %d species, %d path steps" % (len(sel_hap), eng.S, p_sel), flush=True)
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
if route == "walk":
    eng.set_option("growth_route", "walk")
out = eng.strain_growth(sel[0], sel[1], W)           # warm-up
eng.timing_enable(True)
eng.timing_reset()
t0 = time.perf_counter()
for _ in range(N):
    out = eng.strain_growth(sel[0], sel[1], W)
wall = (time.perf_counter() - t0) / N
rows = eng.timing_get()
eng.timing_enable(False)
eng.set_option("growth_route", None)
n_win = len(out[1])
# Engine.strain_growth makes two calls (sizing, then the arrays): the length pass runs twice a repeat, the accumulation and the mask pass once


def per_launch(label):
    r = rows.get(label, (0, 0.0))
    return r[1] / max(r[0], 1)


ms_len, ms_acc, ms_mask = per_launch("cov_track_len_kernel"), per_launch("growth_accum_kernel"), per_launch("read_strain_mask_kernel")
b_len = 8 * p_sel
b_acc = 16 * p_sel + 8 * words + 28 * n_win          # ids, len, bases; the membership words; the four output arrays
t0 = time.perf_counter()
min_own = max(1, W * 500 // 1000)
status = {}
for c in range(len(sel_hap)):
    lo, hi = int(out[0][c]), int(out[0][c + 1])
    f = growth_fit(out[3][lo:hi], out[4][lo:hi], min_own)
    status[f["status"]] = status.get(f["status"], 0) + 1
fit_wall = time.perf_counter() - t0
res = {"workload": name, "window": W, "route": route, "strains": len(sel_hap), "path_steps": p_sel, "windows": n_win, "call_ms_wall": wall * 1e3,
       "cov_track_len_kernel_ms": ms_len, "cov_track_len_kernel_gb": b_len / 1e9, "cov_track_len_kernel_of_8TBs": b_len / ms_len / 1e6 / 8000 if ms_len else None,
       "growth_accum_kernel_ms": ms_acc, "growth_accum_kernel_gb": b_acc / 1e9, "growth_accum_kernel_of_8TBs": b_acc / ms_acc / 1e6 / 8000 if ms_acc else None,
       "read_strain_mask_kernel_ms": ms_mask, "own_steps": int(out[1].sum()), "sum_len": int(out[2].sum()), "sum_len_own": int(out[3].sum()),
       "sum_bases_own": int(out[4].sum()), "fit_ms_wall": fit_wall * 1e3, "fit_status": status}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
