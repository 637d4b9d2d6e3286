#!/usr/bin/env python3
"""Measurement: the bootstrap of the strain fit (pantax_hip_strain_bootstrap), 100 replicates, on a resident coverage result.  Two sets: "long" is the
long-read set of tests/test_gpu_fit.py (synthdata.make_set(925, 2, 6, 400, 300000, long_reads=True), every haplotype selected); any other name is a bench
workload built as bench.py builds it, one resident step (its lad_pair_kernel time is recorded beside: the step's own two solves per species), its rows
(the a15 pass bits) as the selection.  The passes are timed through timing_get, one launch of each per chunk of replicates: per chunk the time of the
weight + scan, the expand, the pattern scan + finalise, the solver and the objective pass, the expanded rows and the algorithmic bytes of the weight +
scan + expand passes with their fraction of 8 TB/s.
usage: bootstrap_probe.py [set (long | cfg4_share | ...)] [replicates (100)] [bootstrap_rows_max (0: default)] [record.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from pantax_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "long"
n_rep = int(sys.argv[2]) if len(sys.argv) > 2 else 100
cap = int(sys.argv[3]) if len(sys.argv) > 3 else 0
record = sys.argv[4] if len(sys.argv) > 4 else None
eng = Engine(0)
t0 = time.perf_counter()
pair_ms = None
if name == "long":
    import synthdata as synth
    sset = synth.make_set(925, 2, 6, 400, 300000, long_reads=True)
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    sel_off = np.array([0, 6, 12], dtype=np.uint64)
    sel_hap = np.array(list(range(6)) * 2, dtype=np.uint32)
else:
    import bench
    spec = bench.workload_spec(name)
    ns = bench.native_set(spec, threads=min(16, os.cpu_count() or 1))
    rd, species, avg = ns.reads(), ns.graphs(), ns.avg_len()
    eng.upload_db(species)
    eng.upload_packed(rd)
    fr = 0.5 if spec.get("long_reads") else 0.3
    eng.profile_step(avg, fr=fr)                     # warm-up
    eng.timing_enable(True)
    eng.timing_reset()
    keep, absolute, met, info, passed, _, _ = eng.profile_step(avg, fr=fr)
    t = eng.timing_get()
    eng.timing_enable(False)
    pair_ms = t.get("lad_pair_kernel", (0, 0.0))[1]
    hap_off = eng.hap_off.astype(np.int64)
    off, hp = [0], []
    for s in range(eng.S):
        hp.extend(int(h - hap_off[s]) for h in range(hap_off[s], hap_off[s + 1]) if passed[h])
        off.append(len(hp))
    sel_off, sel_hap = np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)
V, C, S = int(eng.node_off[-1]), len(sel_hap), eng.S
keys = np.arange(1000, 1000 + S, dtype=np.uint64)
print("%s: %d species, %d nodes, %d selected strains, set up in %.1f s" % (name, S, V, C, time.perf_counter() - t0), flush=True)
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
if cap:
    eng.set_option("bootstrap_rows_max", cap)
eng.strain_bootstrap(sel_off, sel_hap, keys, n_replicates=1)   # warm-up
eng.timing_enable(True)
eng.timing_reset()
t0 = time.perf_counter()
x, obj, rows, status = eng.strain_bootstrap(sel_off, sel_hap, keys, n_replicates=n_rep)
wall = (time.perf_counter() - t0) * 1e3
t = eng.timing_get()
eng.timing_enable(False)
eng.set_option("bootstrap_rows_max", None)
cnt = lambda k: t.get(k, (0, 0.0))[0]
ms = lambda k: t.get(k, (0, 0.0))[1]
n_chunks = max(cnt("boot_expand_kernel"), 1)
R = n_rep + 1
N = int(rows[0].sum())                               # the rows of the sample: every weight 1 in replicate 0
expanded = int(rows.sum())
items = R * N
b_weight = 12 * items + 4 * items                    # species word 8 + v_local 4 read, the prefix 4 written
b_expand = 12 * items + 8 * expanded                 # two prefixes' worth (4) and the abundance (8) read per item, 8 written per expanded row
ms_w, ms_e = ms("scan_chained_kernel<BootWeights>"), ms("boot_expand_kernel")
res = {"set": name, "species": S, "nodes": V, "strains": C, "replicates": n_rep, "rows": N, "expanded_rows": expanded, "chunks": n_chunks,
       "replicates_per_chunk": -(-R // n_chunks), "call_ms_wall": wall,
       "per_chunk_ms": {"weight_scan": ms_w / n_chunks, "expand": ms_e / n_chunks,
                        "pattern_scan_finalize": (ms("scan_chained_kernel<BootLive>") + ms("boot_finalize_kernel")) / n_chunks,
                        "solver": ms("lad_solve_kernel<bootstrap>") / n_chunks, "objective": ms("boot_objective_kernel") / n_chunks},
       "per_chunk_expanded_rows": expanded / n_chunks,
       "per_chunk_bytes": {"weight_scan": b_weight / n_chunks, "expand": b_expand / n_chunks},
       "weight_scan_of_8TBs": b_weight / ms_w / 1e6 / 8000 if ms_w else None, "expand_of_8TBs": b_expand / ms_e / 1e6 / 8000 if ms_e else None,
       "once_per_call_ms": {"rows_scan": ms("scan_chained_kernel<BootRows>"), "pattern_scan": ms("scan_chained_kernel<BootPat>")},
       "solver_ms_per_replicate": ms("lad_solve_kernel<bootstrap>") / R, "step_lad_pair_kernel_ms": pair_ms,
       "solved": int((status == 0).sum()), "not_solved": int((status < 0).sum()),
       "sd_over_refit_median": float(np.median(x[1:].std(axis=0, ddof=1)[x[0] > 0] / x[0][x[0] > 0])) if (x[0] > 0).any() and n_rep > 1 else None}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
