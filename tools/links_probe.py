#!/usr/bin/env python3
"""Measurement: the link support pass (pantax_hip_strain_links) on a bench workload, beside the per-strain read support
(pantax_hip_strain_read_support) and the segment pass (pantax_hip_strain_segments) on the reported strains in the same session.  Builds the set as
bench.py does, runs one resident step, takes Sel from its rows (the a15 pass bits), then a coverage pass of the stage kind (the link and the segment
pass read bases_per_node as pantax_hip_node_coverage leaves it; a resident step keeps none), and times the kernels of the three calls through
timing_get.  Prints the kernels' times, the sort's share of the link table, P_sel (the selected path positions) and the number of distinct links.
usage: links_probe.py [workload (cfg4)] [repeats (3)] [record.json]"""
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
eng.rcls_profile(want_species=False)
eng.trio_nodes_info()
fr = 0.5 if spec.get("long_reads") else 0.3
keep, absolute, met, info, passed, _, _ = eng.profile_step(avg, fr=fr)
eng.get_node_abundances(fetch=False)                             # the coverage result of the stage kind
hap_off = eng.hap_off.astype(np.int64)
sel_off, sel_hap, sel_w, p_sel = [0], [], [], 0
for s in range(eng.S):
    po = species[s].path_off.astype(np.int64)
    for h in range(hap_off[s], hap_off[s + 1]):
        if passed[h]:
            sel_hap.append(h - hap_off[s])
            sel_w.append(met[h].second_sol)
            p_sel += int(po[h - hap_off[s] + 1] - po[h - hap_off[s]])
    sel_off.append(len(sel_hap))
sel = (np.array(sel_off, dtype=np.uint64), np.array(sel_hap, dtype=np.uint32))
sel_w = np.array(sel_w, dtype=np.float64)
R, T = rd.n_reads, len(rd.node_id)
K = np.diff(sel[0].astype(np.int64))
print("reported: %d over %d species (widest list %d), P_sel %d" % (len(sel_hap), eng.S, int(K.max()), p_sel), flush=True)


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
seg, seg_wall, seg_ms = timed(lambda: eng.strain_segments(*sel, 10, 1000))
lk, lk_wall, lk_ms = timed(lambda: eng.strain_links(*sel))
sp, link, hap, brk_off = lk[:4]
sort_ms = sum(ms for k, ms in lk_ms.items() if k.startswith("sort_"))
kernels = ("links_key_kernel", "links_table_kernel", "links_off_kernel", "links_read_kernel", "links_count_kernel", "links_walk_kernel", "links_emit_kernel")
total_ms = sort_ms + sum(lk_ms.get(k, 0.0) for k in kernels)
res = {"workload": name, "reads": R, "steps": T, "reported": len(sel_hap), "species": eng.S, "skipped_species": int((K > 64).sum()), "P_sel": p_sel,
       "distinct_links": int(link[:, 0].sum()), "distinct_links_crossed": int(link[:, 1].sum()), "core_links": int(link[:, 2].sum()),
       "sort_ms": sort_ms, "sort_share_of_link_kernels": sort_ms / total_ms if total_ms else None, "link_kernels_ms": total_ms,
       "read_support_kernel_ms": sup_ms.get("read_support_kernel", 0.0), "segments_tile_kernel_ms": seg_ms.get("segments_tile_kernel", 0.0),
       "segments_emit_kernel_ms": seg_ms.get("segments_emit_kernel", 0.0),
       "strain_links_call_ms_wall": lk_wall, "strain_read_support_call_ms_wall": sup_wall, "strain_segments_call_ms_wall": seg_wall}
res.update({k + "_ms": lk_ms.get(k, 0.0) for k in kernels})
res.update({n: int(c) for n, c in zip(("counted_reads", "crossings", "known", "skip", "switch", "foreign"), sp.sum(axis=0))})
res.update({n: int(c) for n, c in zip(("links", "crossed", "open", "broken", "private", "private_crossed", "private_broken", "support"), hap.sum(axis=0))})
res["longest_selected_walk"] = int(hap[:, 0].max()) + 1 if len(hap) else 0
open_k = K <= 64
counted = sup[1][:, 0]
assert np.array_equal(sp[:, 0], counted[:, 0]) and np.array_equal(sp[:, 1], counted[:, 1] - counted[:, 0]), "counted / crossings differ from the read support pass"
assert np.array_equal(sp[open_k, 1], sp[open_k, 2:].sum(axis=1)) and int(brk_off[-1]) == int(hap[:, 3].sum()), "the identities of the contract"
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
