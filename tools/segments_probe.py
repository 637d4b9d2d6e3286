#!/usr/bin/env python3
"""Measurement: the segments along a strain (pantax_hip_strain_segments) beside the coverage track (pantax_hip_strain_cov_track) on the SAME selection of a
bench workload.  Builds the set as bench.py does, runs one resident step, selects its rows (the a15 pass bits: the strains of strain_abundance.txt) with the
report's peak_depth = max(2, ceil(F x second_sol)), runs the coverage pass as a stage call and times the kernels of both calls through timing_get (device
events): ms a launch, algorithmic bytes and the fraction of 8 TB/s.  The yardstick of segments_tile_kernel + segments_emit_kernel is cov_track_len_kernel +
cov_track_accum_kernel: the gathers of the track's accumulation pass, made twice.
usage: segments_probe.py [workload (cfg4)] [repeats (3)] [min_len (101)] [factor (10)] [record.json]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from pantax_amd.engine import Engine
from pantax_amd.pipeline import _MET_DT

name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3
min_len = int(sys.argv[3]) if len(sys.argv) > 3 else 101           # the report's seeds at its defaults: min(1000, 100 + 1)
F = int(sys.argv[4]) if len(sys.argv) > 4 else 10
record = sys.argv[5] if len(sys.argv) > 5 else None
W = 10000
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
second_sol = np.frombuffer(met, dtype=_MET_DT)["second_sol"]
hap_off = eng.hap_off.astype(np.int64)
sel_off, sel_hap, peak, p_sel = [0], [], [], 0
for s, g in enumerate(species):
    for h in range(hap_off[s], hap_off[s + 1]):
        if passed[h]:
            k = int(h - hap_off[s])
            sel_hap.append(k)
            v = F * float(second_sol[h])
            peak.append(min(max(2, math.ceil(v)) if v == v else 2, 2 ** 31))
            p_sel += int(g.path_off[k + 1]) - int(g.path_off[k])
    sel_off.append(len(sel_hap))
sel = (np.array(sel_off, dtype=np.uint64), np.array(sel_hap, dtype=np.uint32))
peak = np.array(peak, dtype=np.uint64)
print("selected: %d strains over %d species, %d path steps" % (len(sel_hap), eng.S, p_sel), flush=True)
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
eng.strain_cov_track(sel[0], sel[1], W)              # warm-up
seg = eng.strain_segments(sel[0], sel[1], peak, min_len)
KERNELS = ["cov_track_len_kernel", "cov_track_accum_kernel", "segments_tile_kernel", "segments_emit_kernel"]
per_run = []
for _ in range(N):                                   # the two calls in turn, in one process
    r = {}
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    trk = eng.strain_cov_track(sel[0], sel[1], W)
    r["cov_track_call_ms_wall"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    seg = eng.strain_segments(sel[0], sel[1], peak, min_len)
    r["segments_call_ms_wall"] = (time.perf_counter() - t0) * 1e3
    rows = eng.timing_get()
    eng.timing_enable(False)
    for k in KERNELS:                                # both bindings make a sizing call first: the first pass of either runs twice a call
        n, ms = rows.get(k, (0, 0.0))
        r[k] = ms / max(n, 1)
    per_run.append(r)
med = lambda k: float(np.median([r[k] for r in per_run]))
n_win, n_seg = len(trk[1]), len(seg[5])
n_tiles = -(-p_sel // 1024) + len(sel_hap)           # at most: a walk begins and ends inside a tile
gb = {"cov_track_len_kernel": 8 * p_sel, "cov_track_accum_kernel": 20 * p_sel + 28 * n_win, "segments_tile_kernel": 20 * p_sel + 104 * n_tiles,
      "segments_emit_kernel": 20 * p_sel + 37 * n_seg}
ms = {k: med(k) for k in KERNELS}
track_ms, seg_ms = ms["cov_track_len_kernel"] + ms["cov_track_accum_kernel"], ms["segments_tile_kernel"] + ms["segments_emit_kernel"]
res = {"workload": name, "min_len": min_len, "factor": F, "strains": len(sel_hap), "path_steps": p_sel, "windows": n_win, "segments": n_seg,
       "gap_runs": int(seg[2][:, 0].sum()), "peak_runs": int(seg[2][:, 1].sum()), "gap_len": int(seg[3][:, 0].sum()), "peak_len": int(seg[3][:, 1].sum()),
       "sum_hap_len": int(seg[1].sum()), "repeats": N, "median_ms": {k: med(k) for k in per_run[0]}, "per_run_ms": per_run,
       "gb": {k: v / 1e9 for k, v in gb.items()}, "of_8TBs": {k: gb[k] / ms[k] / 1e6 / 8000 if ms[k] else None for k in KERNELS},
       "segments_over_cov_track_kernels": seg_ms / track_ms if track_ms else None,
       "segments_tile_over_cov_track_accum": ms["segments_tile_kernel"] / ms["cov_track_accum_kernel"] if ms["cov_track_accum_kernel"] else None,
       "segments_emit_over_cov_track_accum": ms["segments_emit_kernel"] / ms["cov_track_accum_kernel"] if ms["cov_track_accum_kernel"] else None}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
