#!/usr/bin/env python3
"""Measurement: the rarefaction of the strain fit (pantax_hip_strain_rarefy) on a bench workload with the report's defaults (5 levels, 5 replicates), beside
the coverage pass of the same set -- the yardstick: the bases pass reads the same stream and issues fewer adds.  Builds the set as bench.py does, runs one
resident step, takes Sel from its rows (the a15 pass bits), then a coverage pass of the stage kind under the library's timers, then the stage call.
Prints per launch the time of rarefy_depth_kernel and rarefy_bases_kernel, the pass's algorithmic bytes and an estimate of its atomics (the counted steps
times the kept share of the reads per level: the kernel counts reads and bases, not adds), and the refit chain's share per entry.
usage: rarefy_probe.py [workload (cfg4)] [levels (5)] [replicates (5)] [record.json]"""
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
L = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B = int(sys.argv[3]) if len(sys.argv) > 3 else 5
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
eng.rcls_profile(want_species=False)
eng.trio_nodes_info()
fr = 0.5 if spec.get("long_reads") else 0.3
keep, absolute, met, info, passed, _, _ = eng.profile_step(avg, fr=fr)
hap_off = eng.hap_off.astype(np.int64)
off, hp = [0], []
for s in range(eng.S):
    hp.extend(int(h - hap_off[s]) for h in range(hap_off[s], hap_off[s + 1]) if passed[h])
    off.append(len(hp))
sel = (np.array(off, dtype=np.uint64), np.array(hp, dtype=np.uint32))
R, T, V = rd.n_reads, len(rd.node_id), int(eng.node_off[-1])
K = np.diff(sel[0].astype(np.int64))
print("reported: %d over %d species (widest list %d), %d nodes" % (len(hp), eng.S, int(K.max()), V), flush=True)


def timed(call):
    eng.timing_enable(True)
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    rows = eng.timing_get()
    eng.timing_enable(False)
    return out, wall, rows


is_cov = lambda k: k.startswith("coverage_") or k in ("walk_sum_kernel", "zero_fill_kernel", "popcount_kernel")
eng.get_node_abundances(fetch=False, with_trio=False)                  # warm-up
_, _, cov_t = timed(lambda: eng.get_node_abundances(fetch=False, with_trio=False))
cov_plain = {k: ms for k, (n, ms) in cov_t.items() if is_cov(k)}       # bases and bit vectors, no trio sums
_, _, cov_t = timed(lambda: eng.get_node_abundances(fetch=False))   # ... and the coverage result of the stage kind (a resident step keeps none)
cov_kernels = {k: ms for k, (n, ms) in cov_t.items() if is_cov(k)}
eng.strain_rarefy(*sel, n_levels=1, n_replicates=1)                     # warm-up
res = {"workload": name, "reads": R, "steps": T, "nodes": V, "species": eng.S, "reported": len(hp), "skipped_species": int((K > 64).sum()), "levels": L,
       "replicates": B, "entries": 1 + L * B, "coverage_pass_kernels_ms": cov_kernels, "coverage_pass_without_trio_kernels_ms": cov_plain,
       "coverage_pass_atomics_upper_bound": T}
for layout in ("level",):                                             # (the level arrays are level-major)
    out, wall, t = timed(lambda: eng.strain_rarefy(*sel, n_levels=L, n_replicates=B))
    cnt = lambda k: t.get(k, (0, 0.0))[0]
    ms = lambda k: t.get(k, (0, 0.0))[1]
    own = ("rarefy_depth_kernel", "rarefy_bases_kernel", "rarefy_member_kernel")
    refit_ms = sum(v for k, (n, v) in t.items() if k not in own)
    x, obj, rows, status, reads, member = out
    kept = reads[:, :, 0].sum(axis=1).astype(np.float64)                # counted reads per entry
    share = [float(np.mean([kept[1 + b * L + (l - 1)] for b in range(B)]) / kept[0]) if kept[0] else 0.0 for l in range(1, L + 1)]
    n_pass = max(cnt("rarefy_bases_kernel"), 1)
    res[layout] = {"call_ms_wall": wall, "passes": n_pass, "rarefy_depth_kernel_ms_per_launch": ms("rarefy_depth_kernel") / max(cnt("rarefy_depth_kernel"), 1),
                   "rarefy_bases_kernel_ms_per_pass": ms("rarefy_bases_kernel") / n_pass,
                   "rarefy_member_kernel_ms_per_entry": ms("rarefy_member_kernel") / max(cnt("rarefy_member_kernel"), 1),
                   "refit_kernels_ms_per_entry": refit_ms / (1 + L * B), "refit_kernels_share_of_kernel_time": refit_ms / max(refit_ms + sum(ms(k) for k in own), 1e-9),
                   "kept_share_of_reads_per_level": share,
                   "bases_pass_bytes": {"stream": 5 * T, "slot_records": 25 * R, "node_lengths_estimate": int(4 * T * share[0])},
                   "bases_pass_atomics_estimate": int(T * sum(share)),
                   "solved": int((status == 0).sum()), "nothing_to_solve": int((status == 1).sum()), "not_solved": int((status < 0).sum())}
lv = res["level"]
pass_bytes = sum(lv["bases_pass_bytes"].values())
res["bases_pass_of_8TBs"] = pass_bytes / lv["rarefy_bases_kernel_ms_per_pass"] / 1e6 / 8000 if lv["rarefy_bases_kernel_ms_per_pass"] else None
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
