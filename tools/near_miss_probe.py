#!/usr/bin/env python3
"""Measurement: the unreported-strain near misses (pantax_hip_strain_near_miss) on a bench workload, beside the node evidence pass
(pantax_hip_strain_evidence) on the same reported strains -- the ruler: route 1 of both kernels reads the same 24 bytes of a node it counts.  Builds the
set as bench.py does, runs one resident step, takes its rows (the a15 pass bits: the strains of strain_abundance.txt) as Sel and every other haplotype as
Cand, runs the coverage pass as a stage call and times both node passes through timing_get, in this one process.
usage: near_miss_probe.py [workload (cfg4)] [repeats (3)] [route (node | walk)] [record.json]"""
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
sel_off, sel_hap, cand_off, cand_hap = [0], [], [0], []
for s in range(len(species)):
    for h in range(hap_off[s], hap_off[s + 1]):
        (sel_hap if passed[h] else cand_hap).append(int(h - hap_off[s]))
    sel_off.append(len(sel_hap))
    cand_off.append(len(cand_hap))
sets = (np.array(sel_off, dtype=np.uint64), np.array(sel_hap, dtype=np.uint32), np.array(cand_off, dtype=np.uint64), np.array(cand_hap, dtype=np.uint32))
V = int(eng.node_off[-1])
print("reported: %d strains, candidates: %d haplotypes over %d species, %d nodes" % (len(sel_hap), len(cand_hap), eng.S, V), flush=True)
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
if route == "walk":
    eng.set_option("near_miss_route", "walk")
    eng.set_option("evidence_route", "walk")


def timed(call, args, kernel):
    call(*args)                                      # warm-up
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    for _ in range(N):
        out = call(*args)
    wall = (time.perf_counter() - t0) / N
    rows = eng.timing_get()
    eng.timing_enable(False)
    n, ms = rows.get(kernel, (0, 0.0))
    return out, wall * 1e3, ms / max(n, 1)


(cand, sp), wall_nm, ms_nm = timed(eng.strain_near_miss, sets, "near_miss_node_kernel")
(ev_hap, ev_sp), wall_ev, ms_ev = timed(eng.strain_evidence, sets[:2], "evidence_node_kernel")
assert np.array_equal(sp[:, 0], ev_sp[:, 1])         # the two passes agree on the orphan nodes
eng.set_option("near_miss_route", None)
eng.set_option("evidence_route", None)
J, C, S = len(cand_hap), len(sel_hap), eng.S
b_ev = 24 * V + 64 * C + 96 * S                      # len 4 + cov 4 + bases 8 + membership word 8 per node; the two output blocks
b_nm_max = 24 * V + 64 * J + 96 * S                  # every tile holds an orphan; a tile without one stops behind its 8-byte words
res = {"workload": name, "route": route, "repeats": N, "reported": C, "candidates": J, "species": S, "nodes": V,
       "near_miss_call_ms_wall": wall_nm, "near_miss_node_kernel_ms": ms_nm, "near_miss_node_kernel_gb_at_most": b_nm_max / 1e9,
       "evidence_call_ms_wall": wall_ev, "evidence_node_kernel_ms": ms_ev, "evidence_node_kernel_gb": b_ev / 1e9,
       "near_miss_over_evidence_kernel": ms_nm / ms_ev if ms_ev else None,
       "orphan_nodes": int(sp[:, 0, 0].sum()), "claimed_nodes": int(sp[:, 1, 0].sum()), "contested_nodes": int(sp[:, 2, 0].sum()),
       "orphan_bases": int(sp[:, 0, 3].sum()), "claimed_bases": int(sp[:, 1, 3].sum()), "contested_bases": int(sp[:, 2, 3].sum()),
       "candidates_with_novel_bases": int((cand[:, 0, 3] > 0).sum()), "candidates_with_exclusive_bases": int((cand[:, 1, 3] > 0).sum())}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
