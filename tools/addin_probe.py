#!/usr/bin/env python3
"""Measurement: the add-one test of the strain fit (pantax_hip_strain_addin) on a resident coverage result.  Three sets: "long" is the long-read set of
tests/test_gpu_fit.py (synthdata.make_set(925, 2, 6, 400, 300000, long_reads=True), haplotypes 0 .. 2 of a species reported, the others offered as
candidates); "mid" is a synthetic short-read set of 16 species of 12 haplotypes (synthdata.make_set(926, 16, 12, 200000, 600000, present_frac=0.6),
haplotypes 0 .. 3 reported: with four or five candidates a species has more than seven columns, the <few> instance); any other name is a bench workload
built as bench.py builds it, one resident step, its rows (the a15 pass bits) as the reported strains and every other haplotype of a species of at most 64 haplotypes as a candidate.  As in the file seam the candidates are scored by strain_near_miss, ranked by
near_miss_rank with `top` (5) and cut to 64 - K.  Behind a warm-up call the call is repeated `runs` times with the option addin_yardstick on: the phases are
timed through timing_get (device events), and beside the objective pass of the call (addin_objective_kernel, its three instances, and addin_finish_kernel)
stands the yardstick it is compared with -- boot_objective_kernel over every round's entries, the E_s passes the bootstrap's kernel would make over the same
rows.  The algorithmic bytes of the objective pass: 16 per row of a table or few species ({mask, a}), 8 per row and 12 per pattern of a wide one, the
entries' x once per slice, the partials written and read; their fraction of 8 TB/s.
usage: addin_probe.py [set (long | mid | cfg4_share | ...)] [runs (5)] [addin_patterns_max (0: default)] [record.json] [top (5)]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from pantax_amd.engine import Engine, near_miss_rank

name = sys.argv[1] if len(sys.argv) > 1 else "long"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cap = int(sys.argv[3]) if len(sys.argv) > 3 else 0
record = sys.argv[4] if len(sys.argv) > 4 else None
top = int(sys.argv[5]) if len(sys.argv) > 5 else 5
TABLE_W, FEW_E, SLICE_TABLE, SLICE_FEW, SLICE_WIDE = 7, 8, 16384, 4096, 4096      # addin_plan.hpp
eng = Engine(0)
t0 = time.perf_counter()
if name == "long":
    import synthdata as synth
    sset = synth.make_set(925, 2, 6, 400, 300000, long_reads=True)
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    reported = [[0, 1, 2], [0, 1, 2]]
    others = [[3, 4, 5], [3, 4, 5]]
elif name == "mid":
    import synthdata as synth
    sset = synth.make_set(926, 16, 12, 200000, 600000, present_frac=0.6)
    eng.upload_db(sset.species)
    eng.upload_packed(sset.reads)
    eng.rcls_profile(want_species=False)
    eng.trio_nodes_info()
    reported = [[0, 1, 2, 3] for _ in sset.species]
    others = [list(range(4, g.n_paths)) for g in sset.species]
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
    reported, others = [], []
    for s in range(eng.S):
        hs = range(hap_off[s], hap_off[s + 1])
        reported.append([int(h - hap_off[s]) for h in hs if passed[h]])
        others.append([int(h - hap_off[s]) for h in hs if not passed[h]] if len(hs) <= 64 else [])


def sets(cands):
    so = np.concatenate([[0], np.cumsum([len(r) for r in reported])]).astype(np.uint64)
    co = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.uint64)
    return so, np.array([h for r in reported for h in r], dtype=np.uint32), co, np.array([h for c in cands for h in c], dtype=np.uint32)


eng.get_node_abundances(fetch=False)                 # the coverage result of the stage kind (a resident step keeps none)
all_sets = sets(others)
score, _ = eng.strain_near_miss(*all_sets)
tested = []
for s in range(eng.S):
    c0, c1 = int(all_sets[2][s]), int(all_sets[2][s + 1])
    order = near_miss_rank(all_sets[3][c0:c1], score[c0:c1], top) if c1 > c0 else []
    tested.append([others[s][int(c)] for c in order][:max(0, 64 - len(reported[s]))])
sel_off, sel_hap, cand_off, cand_hap = sets(tested)
V, C, J, S = int(eng.node_off[-1]), len(sel_hap), len(cand_hap), eng.S
print("%s: %d species, %d nodes, %d reported strains, %d tested candidates, set up in %.1f s" % (name, S, V, C, J, time.perf_counter() - t0), flush=True)
if cap:
    eng.set_option("addin_patterns_max", cap)
eng.set_option("addin_yardstick", 1)
eng.strain_addin(sel_off, sel_hap, cand_off, cand_hap)   # warm-up
PHASES = {"rows_scan": ["scan_chained_kernel<BootRows>"], "pattern_scan": ["scan_chained_kernel<BootPat>"], "species": ["addin_species_kernel"], "fill": ["addin_fill_kernel"],
          "solver": ["lad_solve_kernel<addin>"], "objective_table": ["addin_objective_kernel<table>"], "objective_few": ["addin_objective_kernel<few>"],
          "objective_wide": ["addin_objective_kernel<wide>"], "objective_finish": ["addin_finish_kernel"], "yardstick_boot_objective": ["boot_objective_kernel<addin>"]}
per_run = []
for _ in range(runs):
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    x, obj, status, rows, count = eng.strain_addin(sel_off, sel_hap, cand_off, cand_hap)
    wall = (time.perf_counter() - t0) * 1e3
    t = eng.timing_get()
    eng.timing_enable(False)
    r = {k: sum(t.get(n, (0, 0.0))[1] for n in names) for k, names in PHASES.items()}
    r["objective_pass"] = r["objective_table"] + r["objective_few"] + r["objective_wide"] + r["objective_finish"]
    r["front"] = sum(v[1] for n, v in t.items() if n not in sum(PHASES.values(), [])) + r["rows_scan"] + r["pattern_scan"] + r["species"]   # scans, the radix sort, the tables
    r["chunks"] = t.get("addin_fill_kernel", (0, 0.0))[0]
    r["call_ms_wall"] = wall
    per_run.append(r)
eng.set_option("addin_yardstick", None)
eng.set_option("addin_patterns_max", None)
K, Jn = np.diff(sel_off.astype(np.int64)), np.diff(cand_off.astype(np.int64))
W, E = K + Jn, Jn + 1
served = (W >= 1) & (W <= 64) & (rows > 0)
wide = served & (E > FEW_E)
table = served & ~wide & (W <= TABLE_W)
few = served & ~wide & (W > TABLE_W)
n_rows = rows.astype(np.int64)
slices = np.where(wide, -(-n_rows // SLICE_WIDE), np.where(few, -(-n_rows // SLICE_FEW), np.where(table, -(-n_rows // SLICE_TABLE), 0)))
b_rows = int(16 * n_rows[table | few].sum() + 8 * n_rows[wide].sum())
b_x = int((slices * E * W * 8)[served].sum())
b_part = int((slices * E * (8 + 16) * 2)[served].sum())
b_total = b_rows + b_x + b_part                      # (the pattern tables of the wide species are not known from the outputs: 12 bytes a pattern more)
med = lambda k: float(np.median([r[k] for r in per_run]))
rng_ = lambda k: [float(min(r[k] for r in per_run)), float(max(r[k] for r in per_run))]
keys = list(PHASES) + ["front", "objective_pass", "call_ms_wall"]
gains = [float(obj[int(cand_off[s]) + s] - obj[int(cand_off[s]) + s + 1 + c]) for s in range(S) if served[s] for c in range(int(Jn[s]))
         if status[int(cand_off[s]) + s] == 0 and status[int(cand_off[s]) + s + 1 + c] == 0]
res = {"set": name, "species": S, "nodes": V, "reported": C, "candidates": J, "top": top, "entries": int(J + S), "rows": int(n_rows.sum()), "served_species": int(served.sum()),
       "table_species": int(table.sum()), "few_species": int(few.sum()), "wide_species": int(wide.sum()), "w_max": int(W[served].max()) if served.any() else 0,
       "slices": int(slices.sum()), "runs": runs, "median_ms": {k: med(k) for k in keys}, "range_ms": {k: rng_(k) for k in keys}, "chunks": per_run[0]["chunks"],
       "per_run_ms": per_run, "objective_bytes": {"rows": b_rows, "x": b_x, "partials": b_part, "total": b_total},
       "objective_of_8TBs": b_total / med("objective_pass") / 1e6 / 8000 if med("objective_pass") else None,
       "yardstick_over_objective": med("yardstick_boot_objective") / med("objective_pass") if med("objective_pass") else None,
       "solved": int((status == 0).sum()), "nothing_to_solve": int((status == 1).sum()), "not_solved": int((status < 0).sum()),
       "candidates_with_gain": int(sum(g > 0 for g in gains)), "largest_gain": max(gains) if gains else None}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
