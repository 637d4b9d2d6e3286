#!/usr/bin/env python3
"""Measurement: the per-strain depth distribution (pantax_hip_strain_depth) on a bench workload, beside the node evidence pass
(pantax_hip_strain_evidence) on the same selection.  Builds the set as bench.py does, runs one resident step, selects its rows (the a15 pass bits:
the strains of strain_abundance.txt), runs the coverage pass as a stage call and times both node passes through timing_get: ms, algorithmic bytes
and the fraction of 8 TB/s.  With route "walk" the membership comes from the selected walks (depth_route=walk / evidence_route=walk).
usage: depth_probe.py [workload (cfg4)] [repeats (3)] [route (node | walk)] [record.json]"""
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
sel_off, sel_hap, tiles_v = [0], [], 0
for s, g in enumerate(species):
    k_s = 0
    for h in range(hap_off[s], hap_off[s + 1]):
        if passed[h]:
            sel_hap.append(int(h - hap_off[s]))
            k_s += 1
    sel_off.append(len(sel_hap))
    tiles_v += max(1, (k_s + 7) // 8) * int(eng.node_off[s + 1] - eng.node_off[s])   # a species is read once per tile of eight selected haplotypes
sel = (np.array(sel_off, dtype=np.uint64), np.array(sel_hap, dtype=np.uint32))
V = int(eng.node_off[-1])
print("selected: %d strains over %d species, %d nodes, %d node reads of the depth pass" % (len(sel_hap), eng.S, V, tiles_v), flush=True)
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
if route == "walk":
    eng.set_option("depth_route", "walk")
    eng.set_option("evidence_route", "walk")


def timed(call, kernel):
    call(sel[0], sel[1])                             # warm-up
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    for _ in range(N):
        out = call(sel[0], sel[1])
    wall = (time.perf_counter() - t0) / N
    rows = eng.timing_get()
    eng.timing_enable(False)
    n, ms = rows.get(kernel, (0, 0.0))
    return out, wall * 1e3, ms / max(n, 1)


(hap, sp), wall_dp, ms_dp = timed(eng.strain_depth, "depth_hist_kernel")
(ev_hap, ev_sp), wall_ev, ms_ev = timed(eng.strain_evidence, "evidence_node_kernel")
assert np.array_equal(hap.sum(axis=2), ev_hap[:, :, :2]) and np.array_equal(sp.sum(axis=2), ev_sp[:, :2, :2])   # the two passes count the same nodes
eng.set_option("depth_route", None)
eng.set_option("evidence_route", None)
C, S = len(sel_hap), eng.S
b_dp = 20 * tiles_v                                  # len 4 + bases 8 + membership word 8 per node read (route node)
b_ev = 24 * V + 64 * C + 96 * S
tot = sp[:, 0].sum(axis=0)
res = {"workload": name, "route": route, "strains": C, "species": S, "nodes": V, "depth_node_reads": tiles_v,
       "depth_call_ms_wall": wall_dp, "depth_hist_kernel_ms": ms_dp, "depth_hist_kernel_gb": b_dp / 1e9,
       "depth_hist_kernel_of_8TBs": b_dp / ms_dp / 1e6 / 8000 if ms_dp else None,
       "evidence_call_ms_wall": wall_ev, "evidence_node_kernel_ms": ms_ev, "evidence_node_kernel_gb": b_ev / 1e9,
       "evidence_node_kernel_of_8TBs": b_ev / ms_ev / 1e6 / 8000 if ms_ev else None,
       "depth_over_evidence_kernel": ms_dp / ms_ev if ms_ev else None,
       "nonzero_bins_total": int((tot[:, 0] > 0).sum()), "nodes_at_depth_0": int(tot[0, 0]), "nodes_beyond_exact_bins": int(tot[32:, 0].sum())}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
