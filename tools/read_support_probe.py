#!/usr/bin/env python3
"""Measurement: the per-strain read support (pantax_hip_strain_read_support) on a bench workload, beside the per-read assignment
(pantax_hip_read_strains) on the same candidates in the same session.  Builds the set as bench.py does, runs one resident step, takes the
candidates from its rows (the a15 pass bits, weight = predicted_coverage) and times the kernels of both calls through timing_get.
usage: read_support_probe.py [workload (cfg4)] [repeats (3)] [record.json]"""
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
record = sys.argv[3] if len(sys.argv) > 3 else None
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


def timed(call):
    out = call()                                                  # warm-up
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    for _ in range(N):
        out = call()
    wall = (time.perf_counter() - t0) / N
    rows = eng.timing_get()
    eng.timing_enable(False)
    return out, wall * 1e3, {k: ms / N for k, (launches, ms) in rows.items()}


sup, sup_wall, sup_ms = timed(lambda: eng.strain_read_support(*cands))
rs, rs_wall, rs_ms = timed(lambda: eng.read_strains(*cands, fill=fill))
hap, sp, pair_off, pair = sup
# ruler of read_support_kernel: 4 B node id + 1 B step code + 8 B mask word per step, 16 B read record + 8 B slot record per slot (T stands in for T')
byt = 13 * T + 24 * R
k_sup = sup_ms.get("read_support_kernel", 0.0)
res = {"workload": name, "reads": R, "steps": T, "candidates": len(cand_hap), "species": eng.S,
       "read_support_kernel_ms": k_sup, "read_support_long_kernel_ms": sup_ms.get("read_support_long_kernel", 0.0),
       "read_support_kernel_gb": byt / 1e9, "read_support_kernel_of_8TBs": byt / k_sup / 1e6 / 8000 if k_sup else None,
       "read_strain_kernel_ms": rs_ms.get("read_strain_kernel", 0.0), "read_strain_gather_kernel_ms": rs_ms.get("read_strain_gather_kernel", 0.0),
       "strain_read_support_call_ms_wall": sup_wall, "read_strains_call_ms_wall": rs_wall,
       "counted": int(sp[:, 0, 0].sum()), "unexplained": int(sp[:, 1, 0].sum()), "ambiguous": int(sp[:, 2, 0].sum()),
       "uninformative": int(sp[:, 3, 0].sum()), "unique": int(hap[:, 1, 0].sum()), "assigned": int(hap[:, 2, 0].sum()), "pair_entries": int(pair_off[-1])}
n = rs[1]
assert res["assigned"] == int((n > 0).sum()) and res["unexplained"] == int((n == 0).sum()), "the summary and the per-read arrays disagree"
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
