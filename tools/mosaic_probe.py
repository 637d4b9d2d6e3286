#!/usr/bin/env python3
"""Measurement: the mosaic read pass (pantax_hip_strain_mosaic) on a bench workload, beside the per-strain read support
(pantax_hip_strain_read_support) on the same candidates in the same session.  Builds the set as bench.py does, runs one resident step, takes the
candidates from its rows (the a15 pass bits, weight = predicted_coverage) and times the kernels of both calls through timing_get; the mosaic call is
timed with junctions collected (sized inside) and with junction_cap = 0.  The largest k bounds the rounds of a wave's cut: it is read off the classes
(1 round without a mosaic read, 2 with mosaic1 only, ... at least 4 with mosaic3plus).
usage: mosaic_probe.py [workload (cfg4)] [repeats (3)] [record.json]"""
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
mo, mo_wall, mo_ms = timed(lambda: eng.strain_mosaic(*cands))
mo0, mo0_wall, mo0_ms = timed(lambda: eng.strain_mosaic(*cands, junction_cap=0))
species_q, extra, hap, pair_off, pair, jn, jc, n_breaks = mo
_, sup_species, _, _ = sup
# ruler of mosaic_kernel: that of read_support_kernel -- 4 B node id + 1 B step code + 8 B mask word per step, 16 B read record + 8 B slot record per slot
byt = 13 * T + 24 * R
k_mo, k_sup = mo_ms.get("mosaic_kernel", 0.0), sup_ms.get("read_support_kernel", 0.0)
cls = species_q[:, :, 0].sum(axis=0)
res = {"workload": name, "reads": R, "steps": T, "candidates": len(cand_hap), "species": eng.S,
       "mosaic_kernel_ms": k_mo, "mosaic_kernel_no_junctions_ms": mo0_ms.get("mosaic_kernel", 0.0), "read_support_kernel_ms": k_sup,
       "read_support_long_kernel_ms": sup_ms.get("read_support_long_kernel", 0.0), "mosaic_over_read_support": k_mo / k_sup if k_sup else None,
       "mosaic_kernel_gb": byt / 1e9, "mosaic_kernel_of_8TBs": byt / k_mo / 1e6 / 8000 if k_mo else None,
       "strain_mosaic_call_ms_wall": mo_wall, "strain_mosaic_call_no_junctions_ms_wall": mo0_wall, "strain_read_support_call_ms_wall": sup_wall,
       "counted": int(cls[0]), "compatible": int(cls[1]), "mosaic1": int(cls[2]), "mosaic2": int(cls[3]), "mosaic3plus": int(cls[4]), "foreign": int(cls[5]),
       "rounds_at_least": 4 if cls[4] else 3 if cls[3] else 2 if cls[2] else 1,
       "n_segments": int(extra[:, 0].sum()), "n_breaks": int(n_breaks), "foreign_steps": int(extra[:, 2].sum()), "distinct_junctions": int(len(jc))}
served = np.diff(cands[0].astype(np.int64))
served = (served >= 1) & (served <= 64)
assert np.array_equal(species_q[:, 0], sup_species[:, 0]), "counted differs from the read support pass"
assert np.array_equal(species_q[served, 2:].sum(axis=1), sup_species[served, 1]), "mosaic + foreign differs from unexplained of the read support pass"
assert int(jc.sum()) == n_breaks == int(extra[:, 1].sum()) == int(pair.sum()), "the breaks do not add up"
assert all(np.array_equal(a, b) for a, b in zip(mo[:5], mo0[:5])), "the counters differ without junctions"
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
