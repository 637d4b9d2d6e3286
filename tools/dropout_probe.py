#!/usr/bin/env python3
"""Measurement: the leave-one-out test of the strain fit (pantax_hip_strain_dropout) on a resident coverage result.  Two sets: "long" is the long-read set
of tests/test_gpu_fit.py (synthdata.make_set(925, 2, 6, 400, 300000, long_reads=True), every haplotype selected); any other name is a bench workload built
as bench.py builds it, one resident step, its rows (the a15 pass bits) as the selection.  Behind a warm-up call the call is repeated `runs` times with the
option dropout_yardstick on: the phases are timed through timing_get (device events), and beside the objective pass of the call (dropout_objective_kernel,
both instances, and dropout_finish_kernel) stands the yardstick it is compared with -- boot_objective_kernel over every round's entries, the E_s passes the
bootstrap's kernel would make over the same rows.  The algorithmic bytes of the objective pass: 16 per row of a narrow species ({mask, a}), 8 per row and
12 per pattern of a wide one, the entries' x once per slice, the partials written and read; their fraction of 8 TB/s.
usage: dropout_probe.py [set (long | cfg4_share | ...)] [runs (5)] [dropout_patterns_max (0: default)] [record.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from pantax_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "long"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cap = int(sys.argv[3]) if len(sys.argv) > 3 else 0
record = sys.argv[4] if len(sys.argv) > 4 else None
NARROW_E, SLICE_NARROW, SLICE_WIDE = 8, 16384, 4096      # dropout_plan.hpp
eng = Engine(0)
t0 = time.perf_counter()
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
    keep, absolute, met, info, passed, _, _ = eng.profile_step(avg, fr=fr)
    hap_off = eng.hap_off.astype(np.int64)
    off, hp = [0], []
    for s in range(eng.S):
        hp.extend(int(h - hap_off[s]) for h in range(hap_off[s], hap_off[s + 1]) if passed[h])
        off.append(len(hp))
    sel_off, sel_hap = np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32)
V, C, S = int(eng.node_off[-1]), len(sel_hap), eng.S
print("%s: %d species, %d nodes, %d selected strains, set up in %.1f s" % (name, S, V, C, time.perf_counter() - t0), flush=True)
eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
if cap:
    eng.set_option("dropout_patterns_max", cap)
eng.set_option("dropout_yardstick", 1)
eng.strain_dropout(sel_off, sel_hap)                 # warm-up
PHASES = {"rows_scan": ["scan_chained_kernel<BootRows>"], "pattern_scan": ["scan_chained_kernel<BootPat>"], "species": ["drop_species_kernel"], "fill": ["drop_fill_kernel"],
          "solver": ["lad_solve_kernel<dropout>"], "objective_narrow": ["dropout_objective_kernel<narrow>"], "objective_wide": ["dropout_objective_kernel<wide>"],
          "objective_finish": ["dropout_finish_kernel"], "yardstick_boot_objective": ["boot_objective_kernel<dropout>"]}
per_run = []
for _ in range(runs):
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    x, obj, status, rows, count = eng.strain_dropout(sel_off, sel_hap)
    wall = (time.perf_counter() - t0) * 1e3
    t = eng.timing_get()
    eng.timing_enable(False)
    r = {k: sum(t.get(n, (0, 0.0))[1] for n in names) for k, names in PHASES.items()}
    r["objective_pass"] = r["objective_narrow"] + r["objective_wide"] + r["objective_finish"]
    r["chunks"] = t.get("drop_fill_kernel", (0, 0.0))[0]
    r["call_ms_wall"] = wall
    per_run.append(r)
eng.set_option("dropout_yardstick", None)
eng.set_option("dropout_patterns_max", None)
K = np.diff(sel_off.astype(np.int64))
E = K + 1
served = (K >= 1) & (K <= 64) & (rows > 0)
narrow = served & (E <= NARROW_E)
wide = served & (E > NARROW_E)
n_rows = rows.astype(np.int64)
slices = np.where(narrow, -(-n_rows // SLICE_NARROW), np.where(wide, -(-n_rows // SLICE_WIDE), 0))
b_rows = int(16 * n_rows[narrow].sum() + 8 * n_rows[wide].sum())
b_x = int((slices * E * K * 8)[served].sum())
b_part = int((slices * E * (8 + 16) * 2)[served].sum())
b_total = b_rows + b_x + b_part                      # (the pattern tables of the wide species are not known from the outputs: 12 bytes a pattern more)
med = lambda k: float(np.median([r[k] for r in per_run]))
res = {"set": name, "species": S, "nodes": V, "strains": C, "entries": int(C + S), "rows": int(n_rows.sum()), "served_species": int(served.sum()), "narrow_species": int(narrow.sum()),
       "wide_species": int(wide.sum()), "k_max": int(K[served].max()) if served.any() else 0, "slices": int(slices.sum()), "runs": runs,
       "median_ms": {k: med(k) for k in list(PHASES) + ["objective_pass", "call_ms_wall"]}, "chunks": per_run[0]["chunks"], "per_run_ms": per_run,
       "objective_bytes": {"rows": b_rows, "x": b_x, "partials": b_part, "total": b_total},
       "objective_of_8TBs": b_total / med("objective_pass") / 1e6 / 8000 if med("objective_pass") else None,
       "yardstick_over_objective": med("yardstick_boot_objective") / med("objective_pass") if med("objective_pass") else None,
       "solved": int((status == 0).sum()), "nothing_to_solve": int((status == 1).sum()), "not_solved": int((status < 0).sum()),
       "needed_strains": int(sum(obj[int(sel_off[s]) + s + 1 + k] > obj[int(sel_off[s]) + s] * (1 + 1e-9) for s in range(S) if served[s] for k in range(int(K[s])))),
       "free_strains": int(sum(obj[int(sel_off[s]) + s + 1 + k] <= obj[int(sel_off[s]) + s] * (1 + 1e-9) for s in range(S) if served[s] for k in range(int(K[s]))))}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
