#!/usr/bin/env python3
"""Measurement: the per-read strain assignment (pantax_hip_read_strains) on a bench workload.  Builds the set as bench.py does,
runs one resident step, takes the candidates from its rows (the a15 pass bits, weight = predicted_coverage) and times the
kernels of the pass through timing_get: ms, algorithmic bytes and the fraction of 8 TB/s.
usage: read_strains_probe.py [workload (cfg4)] [repeats (3)]"""
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
cand_off, cand_hap, cand_w = [0], [], []
for s in range(eng.S):
    for h in range(hap_off[s], hap_off[s + 1]):
        if passed[h]:
            cand_hap.append(h - hap_off[s])
            cand_w.append(met[h].second_sol)
    cand_off.append(len(cand_hap))
cands = (np.array(cand_off, dtype=np.uint64), np.array(cand_hap, dtype=np.uint32), np.array(cand_w, dtype=np.float64))
R, T = rd.n_reads, len(rd.node_id)
fill = (np.full(R, 0xFFFFFFFF, dtype=np.uint32), np.full(R, -1, dtype=np.int32), np.zeros(R))
print("candidates: %d over %d species (widest %d)" % (len(cand_hap), eng.S, int(np.diff(cands[0]).max())), flush=True)
for route in (None, "walk"):
    eng.set_option("read_strain_route", route)
    out = eng.read_strains(*cands, fill=fill)                     # warm-up
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    for _ in range(N):
        out = eng.read_strains(*cands, fill=fill)
    wall = (time.perf_counter() - t0) / N
    rows = eng.timing_get()
    eng.timing_enable(False)
    print("route %s: call %.1f ms wall (host arrays of %d reads up and down included)" % (route or "default", wall * 1e3, R))
    for k, (launches, ms) in sorted(rows.items()):
        if k.startswith("read_strain"):
            print("  %-28s %9.3f ms" % (k, ms / N))
    # ruler of read_strain_kernel: 4 B node id + 8 B mask word per step, 16 B read record + 16 B result per slot (the padded stream
    # T' >= T is not visible from here: T stands in for it)
    byt = 4 * T + 8 * T + 16 * R + 16 * R
    ms = rows.get("read_strain_kernel", (0, 0.0))[1] / N
    if ms > 0:
        print("  read_strain_kernel: %.2f GB algorithmic, %.0f GB/s = %.3f of 8 TB/s" % (byt / 1e9, byt / ms / 1e6, byt / ms / 1e6 / 8000))
    n = out[1]
    print("  reads: assigned %d, none compatible %d, not counted %d" % ((n > 0).sum(), (n == 0).sum(), (n < 0).sum()), flush=True)
eng.set_option("read_strain_route", None)
eng.close()
