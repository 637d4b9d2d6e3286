#!/usr/bin/env python3
"""Measurement: the read rescue pass (pantax_hip_strain_read_rescue) on a bench workload, beside the per-strain read support
(pantax_hip_strain_read_support) and the mosaic read pass (pantax_hip_strain_mosaic) on the reported strains in the same session.  Builds the set as
bench.py does, runs one resident step, takes Sel from its rows (the a15 pass bits, weight = predicted_coverage) and Cand = the other haplotypes of every
species in ascending index, cut to 64 - K_s (the near-miss rank of the file seam needs a coverage result of the stage kind, which a resident step
does not leave), and times the kernels of the three calls through timing_get.  The three kernels read the same stream behind the same dependent gather.
usage: rescue_probe.py [workload (cfg4)] [repeats (3)] [record.json]"""
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
sel_off, sel_hap, sel_w, cand_off, cand_hap = [0], [], [], [0], []
for s in range(eng.S):
    rest = []
    for h in range(hap_off[s], hap_off[s + 1]):
        if passed[h]:
            sel_hap.append(h - hap_off[s])
            sel_w.append(met[h].second_sol)
        else:
            rest.append(h - hap_off[s])
    sel_off.append(len(sel_hap))
    cand_hap += rest[:max(0, 64 - (sel_off[-1] - sel_off[-2]))]
    cand_off.append(len(cand_hap))
sel = (np.array(sel_off, dtype=np.uint64), np.array(sel_hap, dtype=np.uint32))
cands = (np.array(cand_off, dtype=np.uint64), np.array(cand_hap, dtype=np.uint32))
sel_w = np.array(sel_w, dtype=np.float64)
R, T = rd.n_reads, len(rd.node_id)
K, J = np.diff(sel[0].astype(np.int64)), np.diff(cands[0].astype(np.int64))
print("reported: %d, candidates: %d over %d species (widest list %d)" % (len(sel_hap), len(cand_hap), eng.S, int((K + J).max())), flush=True)


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


sup, sup_wall, sup_ms = timed(lambda: eng.strain_read_support(*sel, sel_w))
mo, mo_wall, mo_ms = timed(lambda: eng.strain_mosaic(*sel, sel_w, junction_cap=0))
rc, rc_wall, rc_ms = timed(lambda: eng.strain_read_rescue(*sel, *cands))
species_q, step, cand_q, cand_steps = rc
# ruler of rescue_kernel: that of read_support_kernel -- 4 B node id + 1 B step code + 8 B mask word per step, 16 B read record + 8 B slot record per slot
byt = 13 * T + 24 * R
k_rc, k_sup, k_mo = rc_ms.get("rescue_kernel", 0.0), sup_ms.get("read_support_kernel", 0.0), mo_ms.get("mosaic_kernel", 0.0)
cls = species_q[:, :, 0].sum(axis=0)
names = ("counted", "compatible", "foreign", "foreign_rescued", "foreign_patchwork", "foreign_novel", "mosaic", "mosaic_rescued", "contested")
res = {"workload": name, "reads": R, "steps": T, "reported": len(sel_hap), "candidates": len(cand_hap), "species": eng.S, "skipped_species": int((K + J > 64).sum()),
       "rescue_kernel_ms": k_rc, "rescue_long_kernel_ms": rc_ms.get("rescue_long_kernel", 0.0), "read_support_kernel_ms": k_sup, "mosaic_kernel_ms": k_mo,
       "rescue_over_read_support": k_rc / k_sup if k_sup else None, "rescue_over_mosaic": k_rc / k_mo if k_mo else None,
       "rescue_kernel_gb": byt / 1e9, "rescue_kernel_of_8TBs": byt / k_rc / 1e6 / 8000 if k_rc else None,
       "strain_read_rescue_call_ms_wall": rc_wall, "strain_read_support_call_ms_wall": sup_wall, "strain_mosaic_call_ms_wall": mo_wall}
res.update({n: int(c) for n, c in zip(names, cls)})
res.update({"foreign_steps": int(step[:, 0].sum()), "claimed_steps": int(step[:, 1].sum()), "novel_steps": int(step[:, 2].sum()),
            "candidates_that_rescue": int((cand_q[:, 0, 0] > 0).sum())})
mo_species, mo_extra = mo[0], mo[1]
open_k = (K + J <= 64) & (K >= 1)
assert np.array_equal(species_q[:, 0], sup[1][:, 0]) and np.array_equal(species_q[:, 0], mo_species[:, 0]), "counted differs between the passes"
assert np.array_equal(species_q[open_k, 1], mo_species[open_k, 1]) and np.array_equal(species_q[open_k, 2], mo_species[open_k, 5]), "compatible / foreign differ from the mosaic pass"
assert np.array_equal(species_q[open_k, 6], mo_species[open_k, 2:5].sum(axis=1)) and np.array_equal(step[open_k, 0], mo_extra[open_k, 2]), "mosaic / foreign_steps differ from the mosaic pass"
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
