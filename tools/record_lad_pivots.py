#!/usr/bin/env python3
"""Record the pivots of the LAD solver: tests/golden/lad_pivots.npz, the file tests/test_gpu_lad_pivots.py compares with.

Run it on a checkout of the commit whose results are to be KEPT (the parent of a change to the solver), never on the code under test:
    python tools/record_lad_pivots.py [--out tests/golden/lad_pivots.npz]
Every group of tests/lad_pivot_cases.py goes through Engine.pao_solve_batch once at the default lad_shape; the call is repeated under roomy and compact
and has to give the same bits (the file holds one record per case, not one per shape).  The resident step of STEP_SET is recorded as JSON text."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from pantax_amd.engine import Engine
    from tests import lad_pivot_cases as lc
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", lc.GOLDEN))
    args = ap.parse_args()
    cases = lc.all_cases(os.path.join(ROOT, "tests", "golden"))
    out = {}
    with Engine(0) as eng:
        for group in lc.GROUPS:
            lps = cases[group]
            t0 = time.time()
            rec = lc.solve_group(eng, lps)
            dt = time.time() - t0
            for shape in ("roomy", "compact"):
                eng.set_option("lad_shape", shape)
                again = lc.solve_group(eng, lps)
                eng.set_option("lad_shape", None)
                for k in rec:
                    assert np.array_equal(rec[k], again[k]), (group, shape, k)
            out[group + "/names"] = np.array([n for n, _ in lps])
            for k, v in rec.items():
                out[group + "/" + k] = v
            print("%-12s %2d LPs  %.2f s  status %s  iterations %s" % (group, len(lps), dt, rec["status"].tolist(), rec["iters"].tolist()), flush=True)
        t0 = time.time()
        step = lc.run_step(eng)
        print("step         %.2f s  iterations %s" % (time.time() - t0, step[2]["iters"]), flush=True)
        out["step/json"] = np.array(lc.to_json(step))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
